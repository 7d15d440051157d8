"""GPU: the OpenAI-CLIP shape module's blocks take `fused.mha_attention` (csrc/mha_attention.hip)
for fp16 under `no_grad` at ViT-B/16's true widths, fall back to `nn.MultiheadAttention` when the
fused path is switched off, and lose nothing against an fp32 evaluation of the same block."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _model():
    from ecoflap_amd.shapes import clip as C
    torch.manual_seed(0)
    return C.clip_slice(1, 1).eval().cuda()


def _inputs(batch=4):
    g = torch.Generator().manual_seed(1)
    img = torch.randn(batch, 3, 224, 224, generator=g).cuda()
    text = torch.randint(1, 49000, (batch, 77), generator=g)
    text[torch.arange(batch), torch.randint(5, 77, (batch,), generator=g)] = 49407
    return img, text.cuda()


def test_forward_runs_both_towers_through_the_kernel(monkeypatch):
    from ecoflap_amd.shapes import fused
    model = _model()
    img, text = _inputs()
    calls = []
    real = fused.mha_attention

    def counted(qkv, heads, scale, causal=False, seq_first=True):
        out = real(qkv, heads, scale, causal=causal, seq_first=seq_first)
        calls.append((tuple(qkv.shape), heads, causal, seq_first, out is not None))
        return out

    monkeypatch.setattr(fused, "mha_attention", counted)
    with torch.no_grad():
        per_image, per_text = model(img, text)
    assert calls == [((197, 4, 2304), 12, False, True, True), ((77, 4, 1536), 8, True, True, True)]
    assert per_image.shape == (4, 4) and per_image.dtype == torch.float16 and torch.isfinite(per_image).all()
    # switched off: the same model on nn.MultiheadAttention, logits close (fp16 towers: the
    # normalised features agree to a few fp16 ulps, the logits are 14.3 x their cosine)
    monkeypatch.setenv("ECOFLAP_NO_FUSED_ATTENTION", "1")
    del calls[:]
    with torch.no_grad():
        lib_image, _ = model(img, text)
    assert [c[-1] for c in calls] == [False, False]
    diff = (per_image.float() - lib_image.float()).abs().max().item()
    print(f"logits fused vs library: max|diff| {diff:.3e}")
    assert diff <= 14.3 * 16 * 2.0 ** -10, diff
    # with autograd the block does not ask for the kernel at all
    monkeypatch.delenv("ECOFLAP_NO_FUSED_ATTENTION")
    del calls[:]
    model(img, text)
    assert calls == []


@pytest.mark.parametrize("tower", ["visual", "text"])
def test_block_attention_is_no_further_from_fp32_than_the_library_path(tower, monkeypatch):
    """`block.attention(x)` in fp16 through the kernel and through nn.MultiheadAttention, both
    against the same block evaluated in fp32: the two fp16 paths share the projections' roundings
    and differ only in the attention between them, where the kernel keeps fp32 scores.  Bound:
    twice the library path's own error plus one fp16 ulp of the largest output."""
    model = _model()
    blk = (model.visual.transformer if tower == "visual" else model.transformer).resblocks[0]
    L, D = (197, 768) if tower == "visual" else (77, 512)
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(L, 16, D, device="cuda", generator=g).half()
    ref = copy.deepcopy(blk).float()
    with torch.no_grad():
        want = ref.attention(x.float())
        got = blk.attention(x)
        monkeypatch.setenv("ECOFLAP_NO_FUSED_ATTENTION", "1")
        lib = blk.attention(x)
    top = want.abs().max().item()
    err, err_lib = (got.float() - want).abs().max().item(), (lib.float() - want).abs().max().item()
    print(f"{tower}: fused {err:.3e}, library {err_lib:.3e}, max|want| {top:.3e}")
    assert err <= 2 * err_lib + 2.0 ** -10 * max(1.0, top), (err, err_lib)
