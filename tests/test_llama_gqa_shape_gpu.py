"""GPU: the LLaMA shape module's fused forward with grouped-query attention (shapes/llama.py on
`ecoflap_causal_attention_gqa`: 4 query heads on 2 key / value heads, k / v read in place at their
own width) against the same weights' fp32 CPU logits, with the module's own torch path on the GPU —
the fp16 op chain tests/test_llama_gqa_shape_golden.py pins to transformers — as the yardstick: the
criterion and the factor of tests/test_llama_shape_gpu.py, the fused forward at most 1.5 x as far
from fp32 as the chain it replaces."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from ecoflap_amd.shapes import llama as L
    torch.manual_seed(13)
    model = L.llama_tiny(hidden_size=256, heads=4, kv_heads=2, head_dim=128, intermediate_size=688, layers=2,
                         vocab_size=320, dtype=torch.float16).eval()
    ids = torch.randint(0, 320, (2, 160), generator=torch.Generator().manual_seed(14))
    with torch.no_grad():
        exact = copy.deepcopy(model).float()(ids, labels=ids)
    return model.cuda(), ids.cuda(), exact


def test_fused_forward_is_as_close_to_fp32_as_the_torch_chain(setup, monkeypatch):
    from ecoflap_amd.shapes import fused
    model, ids, exact = setup
    calls, refused, widths = [0], [0], []
    real = fused.causal_attention

    def counting(q, k, v, heads, scale, **kwargs):
        y = real(q, k, v, heads, scale, **kwargs)
        calls[0] += 1
        refused[0] += y is None
        widths.append((q.shape[-1], k.shape[-1], v.shape[-1], heads, kwargs.get("kv_heads")))
        return y

    with monkeypatch.context() as m:
        m.setattr(fused, "causal_attention", counting)
        with torch.no_grad():
            got = model(ids, labels=ids)
    assert calls == [2] and refused == [0]              # once per layer, never None
    assert widths == [(512, 256, 256, 4, 2)] * 2        # k / v at their own width: nothing was expanded
    assert got.logits.dtype == torch.float16 and bool(torch.isfinite(got.logits).all())

    # the module's torch path on the GPU: the attention switched off, every other fused op refused
    with monkeypatch.context() as m:
        m.setenv("ECOFLAP_NO_FUSED_ATTENTION", "1")
        for name in ("t5_rmsnorm", "t5_add_rmsnorm", "silu_mul", "linear"):
            m.setattr(fused, name, lambda *a, **k: None)
        with torch.no_grad():
            chain = model(ids, labels=ids)

    want = exact.logits.double()
    d_fused = (got.logits.cpu().double() - want).abs().max().item()
    d_chain = (chain.logits.cpu().double() - want).abs().max().item()
    print(f"max|logits - fp32|: fused {d_fused:.3e}, torch chain {d_chain:.3e} (ratio {d_fused / d_chain:.2f}), "
          f"max|logits| {want.abs().max().item():.3f}; loss fused {float(got.loss):.6f}, "
          f"torch chain {float(chain.loss):.6f}, fp32 {float(exact.loss):.6f}")
    assert d_chain > 0 and d_fused <= 1.5 * d_chain
