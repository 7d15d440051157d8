"""GPU: `ecoflap_causal_attention` (`fused.causal_attention`, csrc/causal_attention.hip on
csrc/attention_stream.h), the streaming causal rotary attention of the LLaMA path, against the fp64
attention of the operands its documented arithmetic forms, element by element within the a-priori
bound of `attention_reference.exact_and_bound_stream` (derived from the steps the kernel documents;
nothing in it is measured on a kernel, and tests/test_causal_attention_bound.py shows on the CPU
that flushed subnormal probabilities and a padded key leaking into the last query tile's row sums
both leave it).  The bound never includes the rotation: with a table, the exact result is that of
`rotate_documented(q)`, `rotate_documented(k)`, the kernel's rotation op for op.

Shapes: one key block and one key more (65), the 256-query workgroup boundary from both sides (255,
256; 257, where the second workgroup has one live query and seven idle waves that still stage K
and V), tails that are no multiple of the 32-query tile or the 64-key block (300, 513), every edge
of the first tiles, and the kernel's limit, 4096.  Inputs: the builders of
tests/attention_reference.py.  Every case prints worst = max |out - exact| / bound.

Next to the bound: the rotation is pinned bit for bit by tables on which it is exact (which half
pairs with which, the sign, and which table row a query or key of a tail tile reads); NaN and Inf
stay inside their own (sample, head); the C entry writes nothing outside its output window; a batch
stride of 0 is honoured.

Measured maxima of `worst` on an MI355X, 128 cases, none above 1:
    per table     none 0.762, rotary 0.636, identity 0.691, swap 0.691, parity 0.699
    per input     gauss 0.3 0.666, gauss 1.7 0.564, gauss 8.0 0.089, equal_keys 0.671, equal_rows 0
                  (V bit for bit, under all three exact tables too), subnormal_p 0.725, last_key 0.533,
                  huge_v 0.326, subnormal_p_late 0.762 ((2, 65, 2), no table)
    at the limit  4096 tokens: gauss 1.7 0.489, subnormal_p 0.664; 2048: 0.475 and 0.517
The CPU restatement of the kernel's arithmetic reaches 0.80 on the cases of
tests/test_causal_attention_bound.py, where flushed subnormal probabilities sit at 42 - 167 times
the bound on the two `subnormal_p` builders: fp16-subnormal probabilities survive the packed convert
and the second product of the streaming kernel as well.
"""
import ctypes
import functools

import pytest
import torch

import attention_reference as ref

pytestmark = pytest.mark.gpu

D = 128
SCALE = D ** -0.5
ALL = list(ref.STREAM_BUILDERS)
MAIN = [(2, 65, 2), (1, 257, 2), (2, 300, 3), (1, 513, 2)]                 # (B, T, H)
SMALL = [(1, T, 2) for T in (1, 31, 32, 33, 64, 255, 256)]
LONG = [(1, 2048, 1), (1, 4096, 1)]
PLAIN_CASES = ([(s, n) for s in MAIN for n in ALL]
               + [(s, n) for s in SMALL for n in ("gauss1.7", "equal_keys")]
               + [(s, n) for s in LONG for n in ("gauss1.7", "subnormal_p")])
ROPE_CASES = [(s, n) for s in MAIN for n in ("gauss0.3", "gauss1.7", "gauss8.0", "last_key", "huge_v")]
TABLE_CASES = [(s, n, t) for t in ref.EXACT_TABLES for s in ((1, 257, 2), (2, 300, 3)) for n in ALL]


def _rows(x):
    """[B, H, T, 128] -> the projections' layout [B, T, H * 128]."""
    B, H, T, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, T, H * D).contiguous()


def _heads(out, H):
    """merged heads [B, T, H * 128] -> [B, H, T, 128]."""
    B, T, _ = out.shape
    return out.view(B, T, H, D).permute(0, 2, 1, 3)


def _table(kind, T):
    if kind is None:
        return None
    return ref.rope_table(T) if kind == "real" else ref.EXACT_TABLES[kind](T)


@functools.lru_cache(maxsize=None)
def _case(name, B, T, H, kind):
    """Inputs (fp16 [B, H, T, 128]), the table, and the fp64 result with its bound of the operands
    as the kernel forms them, computed once on the CPU."""
    q, k, v = ref.build_stream(name, B, H, T)
    table = _table(kind, T)
    qr, kr = (q, k) if table is None else (ref.rotate_documented(q, *table), ref.rotate_documented(k, *table))
    A, bound = ref.exact_and_bound_stream(qr, kr, v, SCALE)
    return q, k, v, table, qr, kr, A, bound


def _kernel(q, k, v, H, table):
    """`fused.causal_attention` on [B, T, H * 128] device tensors (any strides it accepts)."""
    from ecoflap_amd.shapes import fused
    rope = None if table is None else tuple(t.cuda() for t in table)
    with torch.no_grad():
        out = fused.causal_attention(q, k, v, H, SCALE, rope=rope)
    assert out is not None and out.dtype == torch.float16 and out.shape == q.shape
    return out


def _run(q, k, v, table):
    """fp16 [B, H, T, 128] on the CPU -> the kernel's output, [B, H, T, 128] on the CPU."""
    H = q.shape[1]
    return _heads(_kernel(_rows(q).cuda(), _rows(k).cuda(), _rows(v).cuda(), H, table), H).cpu()


def _within_bound(label, out, A, bound):
    assert not torch.isnan(out).any(), label
    err = (out.double() - A).abs()
    worst = (err / bound).max().item()
    print(f"{label}: worst = {worst:.3f}")
    assert bool((err <= bound).all()), (label, worst)


def _id(case):
    return "-".join(str(x) for x in case[0]) + "-" + "-".join(case[1:])


@pytest.mark.parametrize("shape,name", PLAIN_CASES, ids=[_id(c) for c in PLAIN_CASES])
def test_without_rotation_within_the_fp64_bound(shape, name):
    B, T, H = shape
    q, k, v, _, _, _, A, bound = _case(name, B, T, H, None)
    out = _run(q, k, v, None)
    _within_bound(f"plain {shape} {name}", out, A, bound)
    if name == "equal_rows":
        assert torch.equal(out, v)


@pytest.mark.parametrize("shape,name", ROPE_CASES, ids=[_id(c) for c in ROPE_CASES])
def test_with_the_rotary_table_within_the_fp64_bound(shape, name):
    B, T, H = shape
    q, k, v, table, _, _, A, bound = _case(name, B, T, H, "real")
    _within_bound(f"rope {shape} {name}", _run(q, k, v, table), A, bound)


@pytest.mark.parametrize("shape,name,kind", TABLE_CASES, ids=[_id(c) for c in TABLE_CASES])
def test_with_an_exact_table_within_the_fp64_bound(shape, name, kind):
    """The ROPE instantiation on tables whose rotation rounds nothing: the exact result is that of
    the permuted inputs.  `equal_rows` returns V bit for bit.  Under identity and swap the rotated
    keys of a head are still one row and p = 1 exactly, as without a table.  Under `parity_table`
    the keys at even and at odd positions are two rows: the class with the larger score has p = 1
    exactly from the first block on (both sit in it), the other p = x < 1 with an fp16 rounding
    error of at most 2^-11 x in O and none in l, so O / l = v * (1 + e) with |e| <= 2^-11 *
    n' x / (n + n' x) for n keys at p = 1 and n' <= n + 1 at x: below 2^-12, the least relative
    half ulp of an fp16, unless x > n / (n + 1), and only past the half ulp does the output leave v."""
    B, T, H = shape
    q, k, v, table, _, _, A, bound = _case(name, B, T, H, kind)
    out = _run(q, k, v, table)
    _within_bound(f"{kind} {shape} {name}", out, A, bound)
    if name == "equal_rows":
        assert torch.equal(out, v)


@pytest.mark.parametrize("kind", ["swap", "parity"])
@pytest.mark.parametrize("B,T,H", [(1, 257, 2), (2, 300, 3)])
def test_the_rotation_is_the_permutation_bit_for_bit(B, T, H, kind):
    """kernel(q, k, v, table) == kernel(permuted q, permuted k, v, no table), the permutation done on
    the host: lo' = -hi, hi' = lo at every position (swap) or at the odd positions only (parity).  A
    wrong pairing, a wrong sign, or a query or key that reads another position's table row (the
    tail rows clamp their table and row addresses) changes the operands, not a rounding."""
    q, k, v, table, qr, kr, _, _ = _case("gauss1.7", B, T, H, kind)
    assert torch.equal(qr, ref.swap_halves(q, odd_only=kind == "parity"))
    assert torch.equal(kr, ref.swap_halves(k, odd_only=kind == "parity"))
    assert not torch.equal(qr, q)
    through_table = _run(q, k, v, table)
    on_the_host = _run(qr, kr, v, None)
    assert torch.equal(through_table, on_the_host)


def _poison(t):
    """NaN, +Inf and -Inf in turn."""
    t[..., 0::3] = float("nan")
    t[..., 1::3] = float("inf")
    t[..., 2::3] = float("-inf")


@pytest.mark.parametrize("kind", [None, "real"])
def test_a_head_of_nan_and_inf_stays_in_its_own_output(kind):
    """(3, 300, 2): with (sample 1, head 1) of q, k and v all NaN / Inf, every other (sample, head)
    of the output equals, bit for bit, the run where that slice is finite."""
    B, T, H = 3, 300, 2
    q, k, v = (_rows(t).cuda() for t in ref.gauss(1.7, B, H, T, D, causal=True))
    table = _table(kind, T)
    clean = _kernel(q, k, v, H, table)
    assert not torch.isnan(clean).any()
    dq, dk, dv = q.clone(), k.clone(), v.clone()
    for t in (dq, dk, dv):
        _poison(t[1, :, D:2 * D])
    dirty = _kernel(dq, dk, dv, H, table)
    assert torch.equal(dirty[0], clean[0]) and torch.equal(dirty[2], clean[2])
    assert torch.equal(dirty[1, :, :D], clean[1, :, :D])


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("B,T", [(1, 1), (2, 257), (2, 300)])
def test_the_entry_stays_inside_its_output_window(B, T, rope):
    """`ecoflap_causal_attention` itself: out is a window in the middle of a larger allocation filled
    with one bit pattern, its token stride 64 halves wider than a row and its batch stride 128
    halves wider than T tokens.  The window holds `fused.causal_attention`'s result and every half
    outside it keeps its bits."""
    from ecoflap_amd import hip
    from ecoflap_amd.shapes import fused
    H = 2
    C = H * D
    q, k, v = (_rows(t).cuda() for t in ref.gauss(1.7, B, H, T, D, causal=True))
    table = ref.rope_table(T) if rope else None
    want = _kernel(q, k, v, H, table)
    fused._get()
    lib = hip.load_library()
    pad, ts = 512, C + 64
    bs = T * ts + 128
    canary = 0x5A5A
    buf = torch.full((pad + B * bs + pad,), canary, dtype=torch.int16, device="cuda")
    cos, sin = (None, None) if table is None else (t.cuda() for t in table)
    rc = lib.ecoflap_causal_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), buf.data_ptr() + 2 * pad,
                                      None if cos is None else cos.data_ptr(),
                                      None if sin is None else sin.data_ptr(), B, T, H, D, q.stride(1),
                                      q.stride(0), ts, bs, SCALE, hip.DTYPE_CODE[torch.float16],
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    window = torch.as_strided(buf, (B, T, C), (bs, ts, 1), pad)
    assert torch.equal(window, want.view(torch.int16))
    outside = torch.ones_like(buf, dtype=torch.bool)
    torch.as_strided(outside, (B, T, C), (bs, ts, 1), pad).fill_(False)
    assert int(outside.sum()) == buf.numel() - B * T * C
    assert bool((buf[outside] == canary).all())


@pytest.mark.parametrize("rope", [False, True])
def test_a_batch_stride_of_zero(rope):
    """q, k and v `expand`ed from one sample to three (batch stride 0, which the entry documents as
    allowed): each of the three outputs equals the one-sample run bit for bit."""
    T, H = 300, 2
    q, k, v = (_rows(t).cuda() for t in ref.gauss(1.7, 1, H, T, D, causal=True))
    table = ref.rope_table(T) if rope else None
    one = _kernel(q, k, v, H, table)
    q3, k3, v3 = (t.expand(3, T, H * D) for t in (q, k, v))
    assert q3.stride(0) == 0
    three = _kernel(q3, k3, v3, H, table)
    for b in range(3):
        assert torch.equal(three[b], one[0]), b
