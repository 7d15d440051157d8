"""GPU: the two kernels whose arithmetic is csrc/attention_tile.h — `ecoflap_vit_attention`
(`fused.vit_attention`, EVA ViT-g) and `ecoflap_mha_attention` / `ecoflap_mha_attention_colsq`
(`fused.mha_attention`, `fused.mha_attention_colsq`, the CLIP towers) — against the fp64 attention of
the same fp16 inputs, element by element within the a-priori bound of
`attention_reference.exact_and_bound` (derived from the steps the tile documents; nothing in it is
measured on a kernel, and tests/test_attention_bound.py shows on the CPU that flushed subnormal
probabilities and a padded key leaking into the row sum both leave it).

Shapes: every path of the ViT-g schedule (the first tile edge at both ends of the head width, query
tiles split over workgroups, the largest token count each head width admits, a second unit per
workgroup with K by LDS DMA and with K through registers, the latter also with nine tiles), and for
CLIP every tile count at and next to its edges with a last workgroup that is not full.  Inputs: the
builders of tests/attention_reference.py.  Every case prints worst = max |out - exact| / bound.

Measured maxima of `worst` on an MI355X, 329 cases, none above 1:
    ecoflap_vit_attention   0.648  ((65, 257, 4, 64), gauss 1.7); `subnormal_p` at most 0.505
    ecoflap_mha_attention   0.826  (L = 161, causal, `subnormal_p`); gauss 1.7 at most 0.714
The CPU restatement of the tile's arithmetic reaches 0.78 on the cases of
tests/test_attention_bound.py (`subnormal_p`, 77 tokens, causal), where flushed subnormal
probabilities sit at 168 times the bound: fp16-subnormal probabilities survive the packed convert
and v_mfma_f32_32x32x16_f16 on gfx950.
"""
import ctypes
import functools

import pytest
import torch

import attention_reference as ref

pytestmark = pytest.mark.gpu

ALL = list(ref.BUILDERS)
FEW = ["gauss1.7", "equal_keys", "subnormal_p"]

# (B, N, H, D)
VIT_SMALL = [(1, 1, 1, 8),                                                  # smallest
             (1, 31, 2, 96), (1, 32, 2, 8), (1, 33, 2, 96),                 # the first tile edge at both ends of D
             (1, 257, 2, 88),                                               # nine parts: each tile in its own workgroup
             (3, 257, 16, 88),                                              # five parts, the last one short
             (1, 261, 2, 88), (1, 288, 3, 72), (1, 221, 2, 96), (1, 288, 2, 64)]    # largest N per D (96: pitch 208)
VIT_WALKS = [(17, 65, 16, 88),                                              # 272 items: second unit, K by DMA
             (33, 33, 8, 64),                                               # 264 items: second unit, K through registers
             (65, 257, 4, 64)]                                              # 260 items, nine tiles, busy = 1, registers
VIT_CASES = ([(s, n) for s in VIT_SMALL for n in ALL] + [(s, n) for s in VIT_WALKS for n in FEW])

CLIP_B, CLIP_H, CLIP_D = 3, 3, 64        # 9 heads: no multiple of the 2 or 4 a workgroup holds
CLIP_L = [1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 161, 193, 224]
# (L, causal, seq_first)
CLIP_LAYOUTS = ([(L, c, True) for L in CLIP_L for c in (False, True)]
                + [(L, c, False) for L in (77, 197) for c in (False, True)])


@functools.lru_cache(maxsize=None)
def _case(name, B, H, N, D, causal):
    """Inputs (fp16 [B, H, N, D]), the fp64 result and its bound, computed once on the CPU."""
    q, k, v = ref.build(name, B, H, N, D, causal=causal)
    scale = D ** -0.5
    A, bound = ref.exact_and_bound(q, k, v, scale, causal)
    return q, k, v, scale, A, bound


def _pack(q, k, v):
    """[B, H, N, D] x 3 -> the batch-first qkv rows [B, N, 3 * H * D] = [B, N, 3, H, D]."""
    B, H, N, D = q.shape
    return torch.stack((q, k, v)).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * H * D).contiguous()


def _heads(out, H):
    """merged heads [B, N, H * D] -> [B, H, N, D]."""
    B, N, C = out.shape
    return out.view(B, N, H, C // H).permute(0, 2, 1, 3)


def _vit(qkv, H, scale):
    from ecoflap_amd.shapes import fused
    with torch.no_grad():
        out = fused.vit_attention(qkv, H, scale)
    assert out is not None and out.dtype == torch.float16 and out.shape == (qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3)
    return out


def _mha(qkv_bf, H, scale, causal, seq_first, colsq=False):
    """`mha_attention` (or `mha_attention_colsq(out=True)`) on batch-first data in the asked row
    order -> the batch-first result."""
    from ecoflap_amd.shapes import fused
    x = qkv_bf.transpose(0, 1).contiguous() if seq_first else qkv_bf
    with torch.no_grad():
        if colsq:
            got = fused.mha_attention_colsq(x, H, scale, out=True, seq_first=seq_first)
            assert got is not None
            out = got[0]
        else:
            out = fused.mha_attention(x, H, scale, causal=causal, seq_first=seq_first)
    assert out is not None and out.dtype == torch.float16
    return out.transpose(0, 1) if seq_first else out


def _within_bound(label, out, A, bound):
    out = out.cpu()
    assert not torch.isnan(out).any(), label
    err = (out.double() - A).abs()
    worst = (err / bound).max().item()
    print(f"{label}: worst = {worst:.3f}")
    assert bool((err <= bound).all()), (label, worst)


def _id(case):
    return "-".join(str(x) for x in case[0]) + "-" + case[1]


@pytest.mark.parametrize("shape,name", VIT_CASES, ids=[_id(c) for c in VIT_CASES])
def test_vit_attention_within_the_fp64_bound(shape, name):
    B, N, H, D = shape
    q, k, v, scale, A, bound = _case(name, B, H, N, D, False)
    out = _heads(_vit(_pack(q, k, v).cuda(), H, scale), H)
    _within_bound(f"vit {shape} {name}", out, A, bound)
    if name == "equal_rows":
        assert torch.equal(out.cpu(), v)


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("L,causal,seq_first", CLIP_LAYOUTS)
def test_mha_attention_within_the_fp64_bound(L, causal, seq_first, name):
    q, k, v, scale, A, bound = _case(name, CLIP_B, CLIP_H, L, CLIP_D, causal)
    qkv = _pack(q, k, v).cuda()
    got = _mha(qkv, CLIP_H, scale, causal, seq_first)
    out = _heads(got, CLIP_H)
    _within_bound(f"mha L={L} causal={causal} seq_first={seq_first} {name}", out, A, bound)
    if name == "equal_rows":
        assert torch.equal(out.cpu(), v)
    if not causal:
        both = _mha(qkv, CLIP_H, scale, False, seq_first, colsq=True)
        assert torch.equal(both, got)


@pytest.mark.parametrize("B,N,H,D", VIT_WALKS)
def test_vit_equal_rows_on_the_second_units(B, N, H, D):
    """`equal_rows` on the shapes whose workgroups walk on to a second unit (the other ViT shapes
    and every CLIP shape assert it next to their bound): the output is V's row, bit for bit."""
    q, k, v = ref.build("equal_rows", B, H, N, D)
    out = _heads(_vit(_pack(q, k, v).cuda(), H, D ** -0.5), H).cpu()
    assert torch.equal(out, v)


def _poison(t):
    """NaN, +Inf and -Inf in turn."""
    flat = t.view(-1)
    flat[0::3] = float("nan")
    flat[1::3] = float("inf")
    flat[2::3] = float("-inf")


def test_vit_sample_of_nan_and_inf_stays_in_its_own_output():
    """(33, 33, 8, 64): 264 items on 256 workgroups; items 0 .. 7 (sample 0) are each the first
    unit of a workgroup that walks on to an item of sample 32 (K through registers into the idle
    buffer, V over the image sample 0 just left).  With sample 0 all NaN / Inf, every other
    sample's output equals, bit for bit, the run where sample 0 is zeros."""
    B, N, H, D = 33, 33, 8, 64
    qkv = _pack(*ref.gauss(1.7, B, H, N, D)).cuda()
    clean, dirty = qkv.clone(), qkv.clone()
    clean[0] = 0
    _poison(dirty[0])
    a = _vit(clean, H, D ** -0.5)
    b = _vit(dirty, H, D ** -0.5)
    assert not torch.isnan(a).any()
    assert torch.equal(a[1:], b[1:])


def test_mha_sample_of_nan_and_inf_stays_in_its_own_output():
    """(20, 129, 3, 64), sequence-first: sample 1's rows lie between the others' in memory.  With
    sample 1 all NaN / Inf, every other sample's output equals, bit for bit, the run where it is
    zeros, causal or not, and so does the colsq kernel's output."""
    B, L, H = 20, 129, 3
    qkv = _pack(*ref.gauss(1.7, B, H, L, CLIP_D)).cuda()
    clean, dirty = qkv.clone(), qkv.clone()
    clean[1] = 0
    _poison(dirty[1])
    keep = [b for b in range(B) if b != 1]
    for causal in (False, True):
        a = _mha(clean, H, CLIP_D ** -0.5, causal, True)
        b = _mha(dirty, H, CLIP_D ** -0.5, causal, True)
        assert not torch.isnan(a).any()
        assert torch.equal(a[keep], b[keep]), causal
    a = _mha(clean, H, CLIP_D ** -0.5, False, True, colsq=True)
    b = _mha(dirty, H, CLIP_D ** -0.5, False, True, colsq=True)
    assert torch.equal(a[keep], b[keep])


@pytest.mark.parametrize("B,N,H,D", [(1, 1, 1, 8), (1, 221, 2, 96), (1, 261, 2, 88), (3, 257, 16, 88),
                                      (33, 33, 8, 64), (17, 65, 16, 88)])
def test_vit_entry_stays_inside_its_buffers(B, N, H, D):
    """`ecoflap_vit_attention` itself: qkv is the first B images of a (B + 1)-image allocation whose
    last image is NaN, out the front of a buffer filled with 7.0.  The result equals
    `fused.vit_attention`'s on a copy of the B images and no half behind it is touched."""
    from ecoflap_amd import hip
    from ecoflap_amd.shapes import fused
    lib = fused._get()
    qkv = _pack(*ref.gauss(1.7, B, H, N, D)).cuda()
    want = _vit(qkv, H, D ** -0.5)
    wide = torch.full((B + 1, N, 3 * H * D), float("nan"), dtype=torch.float16, device="cuda")
    wide[:B] = qkv
    n_out = B * N * H * D
    out = torch.full((2 * n_out + 64,), 7.0, dtype=torch.float16, device="cuda")
    rc = lib.ecoflap_vit_attention(wide.data_ptr(), out.data_ptr(), B, N, H, D, D ** -0.5,
                                   hip.DTYPE_CODE[torch.float16],
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    assert torch.equal(out[:n_out].view(B, N, H * D), want)
    assert bool((out[n_out:] == 7.0).all())
