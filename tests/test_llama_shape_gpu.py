"""GPU: the LLaMA shape module's fused forward (shapes/llama.py on csrc/causal_attention.hip and
`ecoflap_silu_mul`) against the same weights' fp32 CPU logits, with the module's own torch path
on the GPU — the fp16 op chain tests/test_llama_shape_golden.py pins to transformers — as the
yardstick: both are fp16 paths that round at different points, and the fused one may be at most
1.5 x as far from fp32 as the chain it replaces."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from ecoflap_amd.shapes import llama as L
    torch.manual_seed(13)
    model = L.llama_tiny(hidden_size=256, heads=2, head_dim=128, intermediate_size=688, layers=2,
                         vocab_size=320, dtype=torch.float16).eval()
    ids = torch.randint(0, 320, (2, 160), generator=torch.Generator().manual_seed(14))
    with torch.no_grad():
        exact = copy.deepcopy(model).float()(ids, labels=ids)
    return model.cuda(), ids.cuda(), exact


def test_fused_forward_is_as_close_to_fp32_as_the_torch_chain(setup, monkeypatch):
    from ecoflap_amd.shapes import fused
    model, ids, exact = setup
    calls = {"causal_attention": 0, "silu_mul": 0}

    def counting(name):
        real = getattr(fused, name)

        def wrapped(*args, **kwargs):
            y = real(*args, **kwargs)
            calls[name] += y is not None
            return y
        return wrapped

    with monkeypatch.context() as m:
        for name in calls:
            m.setattr(fused, name, counting(name))
        with torch.no_grad():
            got = model(ids, labels=ids)
    assert calls == {"causal_attention": 2, "silu_mul": 2}         # every block took both kernels
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
    scale = want.abs().max().item()
    print(f"max|logits - fp32|: fused {d_fused:.3e}, torch chain {d_chain:.3e} (ratio {d_fused / d_chain:.2f}), "
          f"max|logits| {scale:.3f}")
    assert d_chain > 0 and d_fused <= 1.5 * d_chain
    # the losses of the two paths agree to the same relative distance (the logits' bound relative
    # to their scale).  A cross entropy moves by at most twice the largest logit error, so two paths
    # within d_fused + d_chain <= 2.5 d_chain of each other differ by <= 5 d_chain in the loss;
    # with loss / max|logits| >= 10 / 3 here (ln 320 against logits of order 1) this holds for any
    # pair of paths that meets the bound above, and a path that reads the labels differently misses it
    rel = 1.5 * d_chain / scale
    loss_f, loss_c, loss_x = float(got.loss), float(chain.loss), float(exact.loss)
    print(f"loss: fused {loss_f:.6f}, torch chain {loss_c:.6f}, fp32 {loss_x:.6f}; relative bound {rel:.3e}")
    assert loss_x / scale >= 10 / 3
    assert abs(loss_f - loss_c) / abs(loss_x) <= rel
