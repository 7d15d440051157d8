"""GPU: `ecoflap_causal_attention_gqa` (csrc/causal_attention.hip, `fused.causal_attention(...,
kv_heads=)`), grouped-query causal rotary attention.  Query head h reads KV head h // G, G = heads //
kv_heads; a workgroup serves P query heads of one KV group times 8 / P query tiles of 32.

(a) For P = 0 and every valid explicit P the output equals, bit for bit, `ecoflap_causal_attention`
    on K / V expanded to `heads` heads with `repeat_interleave`: P changes the schedule only.
(b) q, k, v read as slices of one [B, T, (heads + 2 kv_heads) * 128] buffer whose batch stride
    exceeds T rows, `out` written into a wider buffer: same bits, guard bands untouched.
(c) Sample 1 of a batch of 2 equals the same sample run alone, bit for bit.
(d) Within `attention_reference.exact_and_bound_stream` (the project's derived bound; nothing fitted)
    of the fp64 result on the expanded, `rotate_documented`-rotated operands, on every builder of
    `STREAM_BUILDERS`.

Tokens 33, 65, 129, 257 are one query past the workgroup span at P = 8, 4, 2, 1; 300 is ragged in
every unit; (16, 1) puts two workgroups on one KV group; (3, 1) and (6, 1) reach P = 1 and P = 2
with G not a power of two."""
import ctypes
import functools

import pytest
import torch

import attention_reference as ref

pytestmark = pytest.mark.gpu

D = 128
SCALE = D ** -0.5
B = 2
HEADS = [(2, 1), (4, 2), (8, 1), (16, 1), (3, 1), (6, 1)]
TOKENS = [1, 33, 65, 129, 257, 300]


def _valid_p(H, KVH):
    return [p for p in (1, 2, 4, 8) if (H // KVH) % p == 0]


@functools.lru_cache(maxsize=None)
def _inputs(H, KVH, T):
    g = torch.Generator().manual_seed(104729 * T + 131 * H + KVH)
    q = torch.randn(B, T, H * D, generator=g).half()
    k, v = (torch.randn(B, T, KVH * D, generator=g).half() for _ in range(2))
    return q, k, v


def _expand(t, H, KVH):
    """[B, T, KVH * 128] -> [B, T, H * 128]: KV head j repeated for the query heads j * G .. j * G + G - 1."""
    Bn, T, _ = t.shape
    return t.view(Bn, T, KVH, D).repeat_interleave(H // KVH, dim=2).reshape(Bn, T, H * D).contiguous()


def _rope(T, rope):
    return tuple(t.cuda() for t in ref.rope_table(T)) if rope else None


def _gqa(q, k, v, H, KVH, rope, P=0):
    from ecoflap_amd.shapes import fused
    with torch.no_grad():
        out = fused.causal_attention(q, k, v, H, SCALE, rope=rope, kv_heads=KVH, heads_per_workgroup=P)
    assert out is not None and out.dtype == torch.float16 and out.shape == q.shape
    return out


@functools.lru_cache(maxsize=None)
def _oracle(H, KVH, T, rope):
    """`ecoflap_causal_attention` on K / V expanded in memory, once per case."""
    from ecoflap_amd.shapes import fused
    q, k, v = (t.cuda() for t in _inputs(H, KVH, T))
    with torch.no_grad():
        out = fused.causal_attention(q, _expand(k, H, KVH), _expand(v, H, KVH), H, SCALE, rope=_rope(T, rope))
    assert out is not None
    return out


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("H,KVH", HEADS)
def test_every_heads_per_workgroup_gives_the_bits_of_the_plain_entry_on_expanded_kv(H, KVH, T, rope):
    q, k, v = (t.cuda() for t in _inputs(H, KVH, T))
    want = _oracle(H, KVH, T, rope)
    assert not torch.isnan(want).any()
    for P in [0] + _valid_p(H, KVH):
        got = _gqa(q, k, v, H, KVH, _rope(T, rope), P)
        assert torch.equal(got, want), P


def test_an_invalid_heads_per_workgroup_is_refused():
    q, k, v = (t.cuda() for t in _inputs(6, 1, 33))
    from ecoflap_amd.shapes import fused
    with torch.no_grad():
        for P in (3, 4, 8):
            assert fused.causal_attention(q, k, v, 6, SCALE, kv_heads=1, heads_per_workgroup=P) is None


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("H,KVH", HEADS)
def test_slices_of_one_buffer_and_a_guarded_output(H, KVH, T, rope):
    from ecoflap_amd import hip
    from ecoflap_amd.shapes import fused
    q, k, v = _inputs(H, KVH, T)
    C, Ck = H * D, KVH * D
    buf = torch.full((B, T + 3, C + 2 * Ck), float("nan"), dtype=torch.float16)    # batch stride > T rows
    buf[:, :T, :C], buf[:, :T, C:C + Ck], buf[:, :T, C + Ck:] = q, k, v
    buf = buf.cuda()
    qs, ks, vs = buf[:, :T, :C], buf[:, :T, C:C + Ck], buf[:, :T, C + Ck:]
    assert qs.stride(0) > T * qs.stride(1)
    want = _oracle(H, KVH, T, rope)
    table = _rope(T, rope)
    assert torch.equal(_gqa(qs, ks, vs, H, KVH, table), want)
    # out in the middle of a wider buffer, with rows before and after and columns left and right of it
    fused._get()
    lib = hip.load_library()
    wide = torch.full((B, T + 2, C + 128), 7.0, dtype=torch.float16, device="cuda")
    out = wide[:, 1:T + 1, 64:64 + C]
    for P in [0] + _valid_p(H, KVH):
        wide.fill_(7.0)
        rc = lib.ecoflap_causal_attention_gqa(
            qs.data_ptr(), ks.data_ptr(), vs.data_ptr(), out.data_ptr(),
            None if table is None else table[0].data_ptr(), None if table is None else table[1].data_ptr(),
            B, T, H, KVH, D, qs.stride(1), qs.stride(0), ks.stride(1), ks.stride(0), out.stride(1), out.stride(0),
            SCALE, P, 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(out, want), P
        assert bool((wide[:, 0] == 7.0).all()) and bool((wide[:, T + 1] == 7.0).all()), P
        assert bool((wide[:, :, :64] == 7.0).all()) and bool((wide[:, :, 64 + C:] == 7.0).all()), P


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("H,KVH", HEADS)
def test_batch_invariant_bit_for_bit(H, KVH, T):
    q, k, v = (t.cuda() for t in _inputs(H, KVH, T))
    table = _rope(T, True)
    for P in [0] + _valid_p(H, KVH):
        whole = _gqa(q, k, v, H, KVH, table, P)
        alone = _gqa(q[1:2].contiguous(), k[1:2].contiguous(), v[1:2].contiguous(), H, KVH, table, P)
        assert torch.equal(alone[0], whole[1]), P


@functools.lru_cache(maxsize=None)
def _bound_case(name, H, KVH, T):
    """Built at `heads` heads; K / V of a KV head are those of its group's first query head, so the
    forcing relation between q and k (`last_key`) holds for that head, the table-free ones
    (`subnormal_p_late`, `huge_v`, ...) for all.  The reference sees the expanded, rotated operands."""
    G = H // KVH
    q, k, v = ref.build_stream(name, B, H, T)                  # [B, H, T, 128]
    k, v = k[:, ::G].contiguous(), v[:, ::G].contiguous()       # [B, KVH, T, 128]
    cos, sin = ref.rope_table(T)
    A, bound = ref.exact_and_bound_stream(ref.rotate_documented(q, cos, sin),
                                          ref.rotate_documented(k.repeat_interleave(G, dim=1), cos, sin),
                                          v.repeat_interleave(G, dim=1), SCALE)
    flat = lambda t: t.transpose(1, 2).reshape(B, T, -1).contiguous()      # noqa: E731
    return flat(q), flat(k), flat(v), flat(A), flat(bound)


@pytest.mark.parametrize("name", list(ref.STREAM_BUILDERS))
@pytest.mark.parametrize("T", [65, 257, 300])
@pytest.mark.parametrize("H,KVH", [(8, 1), (6, 1)])
def test_within_the_derived_bound_of_the_fp64_result(H, KVH, T, name):
    q, k, v, A, bound = _bound_case(name, H, KVH, T)
    out = _gqa(q.cuda(), k.cuda(), v.cuda(), H, KVH, _rope(T, True)).cpu()
    assert not torch.isnan(out).any()
    worst = ((out.double() - A).abs() / bound).max().item()
    print(f"{name} H={H} KVH={KVH} T={T}: worst |out - A| / bound {worst:.3f}")
    assert worst <= 1.0


def test_refused_inputs_return_none():
    from ecoflap_amd.shapes import fused
    q = torch.randn(2, 8, 4 * D, device="cuda").half()
    k, v = (torch.randn(2, 8, 2 * D, device="cuda").half() for _ in range(2))
    with torch.no_grad():
        assert fused.causal_attention(q, k, v, 4, SCALE, kv_heads=2) is not None
        assert fused.causal_attention(q, k, v, 4, SCALE) is None                        # k / v narrower than q
        assert fused.causal_attention(q, k, v, 4, SCALE, kv_heads=4) is None
        assert fused.causal_attention(q, k, v, 4, SCALE, kv_heads=1) is None            # k / v are 2 heads wide
        assert fused.causal_attention(q, k, v, 4, SCALE, kv_heads=3) is None
        assert fused.causal_attention(q, k, v[:, :4], 4, SCALE, kv_heads=2) is None
        assert fused.causal_attention(q, k, torch.zeros(2, 8, 4 * D, device="cuda").half()[..., ::2], 4, SCALE,
                                      kv_heads=2) is None                               # v's strides differ from k's
        assert fused.causal_attention(q, k.bfloat16(), v.bfloat16(), 4, SCALE, kv_heads=2) is None
        assert fused.causal_attention(q.cpu(), k.cpu(), v.cpu(), 4, SCALE, kv_heads=2) is None
        # kv_heads == heads is the plain call
        assert torch.equal(fused.causal_attention(q, q, q, 4, SCALE, kv_heads=4), fused.causal_attention(q, q, q, 4, SCALE))
    assert fused.causal_attention(q, k, v, 4, SCALE, kv_heads=2) is None                # autograd on
