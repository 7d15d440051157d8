"""GPU: `ecoflap_mha_attention` (csrc/mha_attention.hip, `fused.mha_attention`), the attention of
the OpenAI-CLIP towers' shape family (head width 64, <= 224 tokens, optional causal mask, sequence-
or batch-first rows read in place) against fp32 `softmax(q k^T * scale + mask) v` on the same fp16
inputs, with the bounds of `test_gpu_parity.py::test_vit_attention_kernel_vs_fp32_reference`."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 64
SHAPES = [(77, 8), (197, 12), (50, 12), (1, 1), (33, 2), (224, 4)]      # (tokens, heads)
BATCHES = [1, 5, 16, 256]


def _reference(qkv_bf, heads, scale, causal):
    """fp32 attention of a batch-first [B, L, 3 * heads * 64] fp16 tensor -> [B, L, heads * 64] fp32
    (in slices of the batch: the fp32 score tensor of 256 x 12 x 197 x 197 is half a gigabyte)."""
    B, L, _ = qkv_bf.shape
    out = torch.empty(B, L, heads * D, dtype=torch.float32, device=qkv_bf.device)
    mask = None
    if causal:
        mask = torch.full((L, L), float("-inf"), device=qkv_bf.device).triu_(1)
    for b0 in range(0, B, 32):
        q, k, v = qkv_bf[b0:b0 + 32].float().reshape(-1, L, 3, heads, D).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-1, -2)) * scale
        if mask is not None:
            s = s + mask
        out[b0:b0 + 32] = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(-1, L, heads * D)
    return out


def _run(qkv_bf, heads, scale, causal, seq_first):
    """The kernel on the batch-first data in the asked row order -> batch-first result."""
    from ecoflap_amd.shapes import fused
    with torch.no_grad():
        if seq_first:
            got = fused.mha_attention(qkv_bf.transpose(0, 1).contiguous(), heads, scale, causal=causal,
                                      seq_first=True)
            assert got is not None
            return got.transpose(0, 1)
        got = fused.mha_attention(qkv_bf, heads, scale, causal=causal, seq_first=False)
        assert got is not None
        return got


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("seq_first", [False, True])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L,H", SHAPES)
def test_kernel_vs_fp32_reference(L, H, causal, seq_first, B):
    g = torch.Generator(device="cuda").manual_seed(1000 * B + 10 * L + H + int(causal))
    qkv = (torch.randn(B, L, 3 * H * D, device="cuda", generator=g) * 1.7).half()
    scale = D ** -0.5
    got = _run(qkv, H, scale, causal, seq_first)
    assert got.shape == (B, L, H * D) and got.dtype == torch.float16
    want = _reference(qkv, H, scale, causal)
    err = (got.float() - want).abs().max().item()
    print(f"gaussian: max|err| {err:.3e}, max|want| {want.abs().max().item():.3e}")
    assert err <= 4e-3 * max(1.0, want.abs().max().item()), err
    # sharper test of the operand layouts: integer data, one-hot attention (huge scale)
    qi = torch.randint(-2, 3, (B, L, 3 * H * D), device="cuda", generator=g).half()
    got_i = _run(qi, H, 64.0, causal, seq_first)
    want_i = _reference(qi, H, 64.0, causal)
    err_i = (got_i.float() - want_i).abs().max().item()
    print(f"integer: max|err| {err_i:.3e}, max|want| {want_i.abs().max().item():.3e}")
    assert err_i <= 2e-3 * max(1.0, want_i.abs().max().item()), err_i
    if causal:
        # query 0 sees key 0 alone: its probability is exp2(0) = 1, the row sum 1, its inverse 1
        # (all exact), so the output row is v[0] itself
        v0 = qkv[:, 0].reshape(B, 3, H * D)[:, 2]
        assert torch.equal(got[:, 0], v0)
    # batch invariance: sample 0 alone == sample 0 inside the batch, bit for bit
    alone = _run(qkv[:1].contiguous(), H, scale, causal, seq_first)
    assert torch.equal(alone[0], got[0])


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L,H,B", [(77, 8, 16), (197, 12, 5), (33, 2, 3), (1, 1, 1), (224, 4, 2)])
def test_seq_first_equals_batch_first_bit_for_bit(L, H, B, causal):
    """One arithmetic whatever the row order: contiguous copies in either order and a permuted
    view of either (read in place through its strides) all give the same bits."""
    from ecoflap_amd.shapes import fused
    g = torch.Generator(device="cuda").manual_seed(L + H + B)
    bf = (torch.randn(B, L, 3 * H * D, device="cuda", generator=g) * 1.7).half()
    sf = bf.transpose(0, 1).contiguous()
    with torch.no_grad():
        out_bf = fused.mha_attention(bf, H, D ** -0.5, causal=causal, seq_first=False)
        out_sf = fused.mha_attention(sf, H, D ** -0.5, causal=causal, seq_first=True)
        view_sf = fused.mha_attention(bf.transpose(0, 1), H, D ** -0.5, causal=causal, seq_first=True)
        view_bf = fused.mha_attention(sf.transpose(0, 1), H, D ** -0.5, causal=causal, seq_first=False)
    assert out_sf.shape == (L, B, H * D) and out_sf.is_contiguous() and out_bf.is_contiguous()
    assert torch.equal(out_sf.transpose(0, 1), out_bf)
    assert torch.equal(view_sf, out_sf) and torch.equal(view_bf, out_bf)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L,H,B", [(77, 3, 3), (90, 1, 5), (33, 1, 3), (50, 3, 1), (20, 1, 7), (1, 3, 3)])
def test_last_workgroup_with_fewer_heads_than_it_holds(L, H, B, causal):
    """A workgroup holds 2 (65-96 tokens, 33-64 tokens) or 4 (<= 32 tokens) heads; here B * H is
    not a multiple of that, so the last workgroup has idle waves beside working ones."""
    g = torch.Generator(device="cuda").manual_seed(L * H + B)
    qkv = (torch.randn(B, L, 3 * H * D, device="cuda", generator=g) * 1.7).half()
    got = _run(qkv, H, D ** -0.5, causal, True)
    want = _reference(qkv, H, D ** -0.5, causal)
    assert (got.float() - want).abs().max().item() <= 4e-3 * max(1.0, want.abs().max().item())


def test_causal_prefix_is_the_prefix_of_the_causal_result():
    """Keys above the diagonal do not enter a query's result: the causal attention of the first n
    tokens alone equals, bit for bit, the first n rows of the causal attention of the whole
    sequence (n on both sides of the 32-token tile edges), and nothing is NaN."""
    from ecoflap_amd.shapes import fused
    L, H, B = 77, 8, 4
    g = torch.Generator(device="cuda").manual_seed(5)
    a = (torch.randn(L, B, 3 * H * D, device="cuda", generator=g) * 1.7).half()
    with torch.no_grad():
        full = fused.mha_attention(a, H, D ** -0.5, causal=True)
        assert not torch.isnan(full).any()
        for n in (1, 31, 32, 33, 64, 76):
            part = fused.mha_attention(a[:n].contiguous(), H, D ** -0.5, causal=True)
            assert torch.equal(part, full[:n]), n


def test_refused_inputs_return_none():
    from ecoflap_amd.shapes import fused
    ok = torch.randn(8, 2, 3 * 2 * D, device="cuda").half()
    with torch.no_grad():
        assert fused.mha_attention(ok, 2, D ** -0.5) is not None
        assert fused.mha_attention(torch.randn(8, 2, 3 * 2 * 32, device="cuda").half(), 2, 32 ** -0.5) is None
        assert fused.mha_attention(torch.randn(8, 2, 3 * 2 * 88, device="cuda").half(), 2, 88 ** -0.5) is None
        assert fused.mha_attention(torch.randn(225, 1, 3 * D, device="cuda").half(), 1, D ** -0.5) is None
        assert fused.mha_attention(ok.bfloat16(), 2, D ** -0.5) is None
        assert fused.mha_attention(ok.float(), 2, D ** -0.5) is None
        assert fused.mha_attention(ok.cpu(), 2, D ** -0.5) is None
        assert fused.mha_attention(ok, 2, 0.0) is None
        assert fused.mha_attention(ok[:, :, 1:], 2, D ** -0.5) is None          # width not 3 * heads * 64
    assert fused.mha_attention(ok, 2, D ** -0.5) is None                            # autograd on


def test_entry_point_argument_errors():
    """`ecoflap_mha_attention` itself: every argument error returns its code before a launch (the
    output keeps its fill)."""
    from ecoflap_amd import hip
    lib = hip.load_library()
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.ecoflap_mha_attention.argtypes = [vp, vp, i64, i64, i64, i64, i64, i64, i64, i64,
                                          ctypes.c_int, ctypes.c_float, ctypes.c_int, vp]
    L, B, H = 16, 2, 2
    qkv = torch.randn(L * B * 3 * H * D + 8, device="cuda").half()
    out = torch.full((L * B * H * D + 8,), 7.0, device="cuda").half()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    row, orow = 3 * H * D, H * D

    def call(q=None, o=None, batch=B, tokens=L, heads=H, hd=D, qts=B * row, qbs=row, ots=B * orow,
             obs=orow, scale=0.125, dtype=1):
        return lib.ecoflap_mha_attention(qkv.data_ptr() if q is None else q, out.data_ptr() if o is None else o,
                                         batch, tokens, heads, hd, qts, qbs, ots, obs, 0, scale, dtype, st)

    assert call(dtype=2) == -1 and call(dtype=0) == -1                      # EDTYPE
    assert call(hd=32) == -3 and call(tokens=225) == -3 and call(tokens=0) == -3      # ESIZE
    assert call(batch=0) == -3 and call(scale=0.0) == -3 and call(qts=row - 8) == -3
    assert call(q=0) == -2 and call(o=0) == -2                              # ENULL
    assert call(q=qkv.data_ptr() + 2) == -5 and call(o=out.data_ptr() + 8) == -5      # EALIGN
    assert call(qts=B * row + 4) == -5 and call(obs=orow + 2) == -5
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out[:L * B * H * D] == 7.0).all()) and bool((out[L * B * H * D:] == 7.0).all())
