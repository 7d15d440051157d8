"""GPU: `ecoflap_mha_attention_colsq` (csrc/mha_attention.hip, `fused.mha_attention_colsq`): the
non-causal attention of the CLIP towers with the Wanda column statistic of its output as an
epilogue — same output bits as `ecoflap_mha_attention(causal = 0)`, the statistic bitwise
repeatable and independent of whether the output is stored, within 1e-5 (the tolerance
for re-ordered float reductions) of the fp64 sum of squares of that fp16 output, and no further
from an fp64 evaluation of the reference's `hacky_attn` chain than that chain run in fp16."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

TOWERS = {"visual": (197, 12), "text": (77, 8)}


def _qkv(L, B, H, seq_first, seed=0, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = (L, B, 3 * H * 64) if seq_first else (B, L, 3 * H * 64)
    return (torch.randn(shape, device="cuda", generator=g) * scale).half()


@pytest.mark.parametrize("seq_first", [True, False])
@pytest.mark.parametrize("batch", [1, 4, 16])
@pytest.mark.parametrize("tower", list(TOWERS))
def test_output_bits_statistic_and_repeatability(tower, batch, seq_first):
    from ecoflap_amd.shapes import fused
    L, H = TOWERS[tower]
    qkv = _qkv(L, batch, H, seq_first, seed=batch)
    with torch.no_grad():
        want = fused.mha_attention(qkv, H, 64 ** -0.5, causal=False, seq_first=seq_first)
        y, sq = fused.mha_attention_colsq(qkv, H, 64 ** -0.5, out=True, seq_first=seq_first)
        none, sq_only = fused.mha_attention_colsq(qkv, H, 64 ** -0.5, out=False, seq_first=seq_first)
        y2, sq2 = fused.mha_attention_colsq(qkv, H, 64 ** -0.5, out=True, seq_first=seq_first)
    assert none is None and sq.shape == (H * 64,) and sq.dtype == torch.float32
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))
    assert torch.equal(sq.view(torch.int32), sq_only.view(torch.int32))
    assert torch.equal(sq.view(torch.int32), sq2.view(torch.int32)) and torch.equal(y, y2)
    exact = (want.reshape(-1, H * 64).double() ** 2).sum(0)
    rel = ((sq.double() - exact).abs() / exact).max().item()
    print(f"{tower} batch {batch} seq_first {seq_first}: max rel |sq - fp64| {rel:.2e}")
    assert rel <= 1e-5, rel


def test_token_tail_and_strided_views():
    """Query rows >= tokens contribute nothing (tokens not a multiple of 32), and a permuted view
    is read in place."""
    from ecoflap_amd.shapes import fused
    for L in (1, 31, 33, 100, 224):
        qkv = _qkv(L, 3, 2, True, seed=L)
        with torch.no_grad():
            y, sq = fused.mha_attention_colsq(qkv, 2, 0.125, out=True)
            yv, sqv = fused.mha_attention_colsq(qkv.transpose(0, 1), 2, 0.125, out=True, seq_first=False)
        exact = (y.reshape(-1, 128).double() ** 2).sum(0)
        assert ((sq.double() - exact).abs() / exact).max().item() <= 1e-5, L
        assert torch.equal(sqv, sq) and torch.equal(yv.transpose(0, 1), y)


def test_refusals_match_mha_attention():
    from ecoflap_amd.shapes import fused
    with torch.no_grad():
        ok = torch.randn(8, 2, 3 * 2 * 64, device="cuda").half()
        assert fused.mha_attention_colsq(ok, 2, 0.125) is not None
        assert fused.mha_attention_colsq(torch.randn(8, 2, 3 * 2 * 32, device="cuda").half(), 2, 32 ** -0.5) is None
        assert fused.mha_attention_colsq(torch.randn(225, 1, 192, device="cuda").half(), 1, 0.125) is None
        assert fused.mha_attention_colsq(ok.float(), 2, 0.125) is None
        assert fused.mha_attention_colsq(ok.cpu(), 2, 0.125) is None
        assert fused.mha_attention_colsq(ok, 2, 0.0) is None
    assert fused.mha_attention_colsq(ok, 2, 0.125) is None                  # autograd on


def test_runs_inside_a_captured_graph():
    """Launches only: captured once, replayed on new inputs, the statistic is the eager one."""
    from ecoflap_amd.shapes import fused
    static = _qkv(77, 4, 8, True, seed=1)
    with torch.no_grad():
        fused.mha_attention_colsq(static, 8, 0.125, out=False)             # warm-up
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _, sq = fused.mha_attention_colsq(static, 8, 0.125, out=False)
        for seed in (2, 3):
            fresh = _qkv(77, 4, 8, True, seed=seed)
            static.copy_(fresh)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(sq, fused.mha_attention_colsq(fresh, 8, 0.125, out=False)[1])


def test_c_entry_argument_errors():
    """Every argument error returns its code before a launch (nothing touches the GPU: the
    pointers handed in are never dereferenced)."""
    from ecoflap_amd import hip
    lib = hip.load_library()
    vp, i64, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t
    lib.ecoflap_mha_attention_colsq_workspace_bytes.restype = sz
    lib.ecoflap_mha_attention_colsq_workspace_bytes.argtypes = [i64, i64]
    lib.ecoflap_mha_attention_colsq.argtypes = [vp, vp, vp, vp, sz, i64, i64, i64, i64, i64, i64, i64, i64,
                                                ctypes.c_float, ctypes.c_int, vp]
    assert lib.ecoflap_mha_attention_colsq_workspace_bytes(16, 12) == 16 * 12 * 64 * 4
    assert lib.ecoflap_mha_attention_colsq_workspace_bytes(0, 12) == 0
    B, L, H = 2, 8, 2
    base = dict(qkv=0x1000, out=0x2000, sq=0x3000, ws=0x4000, ws_bytes=B * H * 256, batch=B, tokens=L,
                heads=H, head_dim=64, qts=B * 3 * H * 64, qbs=3 * H * 64, ots=B * H * 64, obs=H * 64,
                scale=0.125, dtype=1)

    def call(**kw):
        a = dict(base, **kw)
        return lib.ecoflap_mha_attention_colsq(a["qkv"], a["out"], a["sq"], a["ws"], a["ws_bytes"], a["batch"],
                                               a["tokens"], a["heads"], a["head_dim"], a["qts"], a["qbs"],
                                               a["ots"], a["obs"], a["scale"], a["dtype"], None)

    EDTYPE, ENULL, ESIZE, EALIGN = -1, -2, -3, -5
    assert call(dtype=0) == EDTYPE and call(dtype=2) == EDTYPE
    for bad in (dict(batch=0), dict(tokens=0), dict(tokens=225), dict(heads=0), dict(head_dim=88),
                dict(scale=0.0), dict(scale=float("inf")), dict(qts=3 * H * 64 - 8), dict(qbs=-8),
                dict(ots=H * 64 - 8), dict(ws_bytes=B * H * 256 - 1)):
        assert call(**bad) == ESIZE, bad
    for bad in (dict(qkv=None), dict(sq=None), dict(ws=None)):
        assert call(**bad) == ENULL, bad
    for bad in (dict(qkv=0x1008), dict(out=0x2008), dict(sq=0x3004), dict(ws=0x4008), dict(qts=B * 3 * H * 64 + 4),
                dict(obs=H * 64 + 4)):
        assert call(**bad) == EALIGN, bad
    # a null `out` is an argument, not an error: its strides are then not looked at (real buffers here)
    qkv = torch.randn(L, B, 3 * H * 64, device="cuda").half()
    sq = torch.empty(H * 64, device="cuda")
    ws = torch.empty(B * H * 256, dtype=torch.uint8, device="cuda")
    assert call(qkv=qkv.data_ptr(), out=None, sq=sq.data_ptr(), ws=ws.data_ptr(), ots=0, obs=-4) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(sq).all() and float(sq.min()) > 0


@pytest.mark.parametrize("tower", list(TOWERS))
def test_statistic_against_the_reference_chain(tower):
    """The kernel's statistic and the reference's literal `hacky_attn` chain in fp16 torch
    (wanda_pruner.py:76-101: `q * scale`, `q @ k^T`, softmax, `@ v`, all rounded to fp16; then
    WrappedGPT's fp32 `norm ** 2`), each against an fp64 evaluation of the chain on the same qkv.
    The kernel keeps fp32 scores where the chain rounds them, so it may be no further off than
    twice the chain's own error plus one fp16 ulp of the statistic's scale (the rule of
    test_clip_shape_gpu.py)."""
    from ecoflap_amd.shapes import fused
    L, H = TOWERS[tower]
    B = 16
    qkv = _qkv(L, B, H, False, seed=7)          # [N, L, 3D]: the layout the side copy's qkv Linear leaves

    def chain(t):
        q, k, v = t.reshape(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
        q = q * (64 ** -0.5)
        attn = (q @ k.transpose(-2, -1)).softmax(dim=-1)
        return (attn @ v).transpose(1, 2).reshape(B * L, H * 64)

    with torch.no_grad():
        want = (chain(qkv.double()) ** 2).sum(0)
        half = torch.norm(chain(qkv).t().float(), p=2, dim=1) ** 2
        _, sq = fused.mha_attention_colsq(qkv, H, 64 ** -0.5, out=False, seq_first=False)
    top = want.max().item()
    err, err_chain = (sq.double() - want).abs().max().item(), (half.double() - want).abs().max().item()
    rel, rel_chain = ((sq.double() - want).abs() / want).max().item(), ((half.double() - want).abs() / want).max().item()
    print(f"{tower}: kernel max|err| {err:.3e} (rel {rel:.2e}), fp16 chain {err_chain:.3e} (rel {rel_chain:.2e}), "
          f"max statistic {top:.3e}")
    assert err <= 2 * err_chain + 2.0 ** -10 * max(1.0, top), (err, err_chain)
