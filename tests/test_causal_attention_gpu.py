"""GPU: `ecoflap_causal_attention` (csrc/causal_attention.hip, `fused.causal_attention`), the causal
rotary attention of a LLaMA block, against three quantities the test computes on the CPU from the
same fp16 inputs and the same fp32 table:

    A        the fp64 result
    e_chain  max|chain - A|, chain = transformers' eager op chain in fp16 (table cast to fp16):
             q * cos + rotate_half(q) * sin, matmul * scale + mask, softmax(dtype=float32).to(fp16), matmul
    e_kernel max|out - A|

and demands e_kernel <= e_chain: the kernel may not be further from exact than the op chain it
replaces.  The bound comes from the reference arithmetic, not from the code under test; on random
data it is 1.5e-3 .. 3.0e-3 at output scale ~ 3, and a wrong mask, rotation or rescale moves
outputs by O(1).  The kernel rescales on every key block (no deferred-rescale threshold); the
forcing cases plant one key whose score towers over its row, once in a late key block (the running
maximum jumps there) and once in the first (every later block is rescaled against it)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
THETA = 10000.0


def _table(T):
    inv_freq = 1.0 / (THETA ** (torch.arange(0, D, 2, dtype=torch.float) / D))
    freqs = torch.arange(T, dtype=torch.float)[:, None] * inv_freq[None, :]
    return freqs.cos(), freqs.sin()                     # [T, 64] fp32


def _rotate_half(x):
    return torch.cat((-x[..., D // 2:], x[..., : D // 2]), dim=-1)


def _rot(x, cos, sin):
    """x: [..., T, 128]; cos / sin: [T, 64] in x's dtype."""
    c, s = torch.cat((cos, cos), -1), torch.cat((sin, sin), -1)
    return (x * c) + (_rotate_half(x) * s)


def _heads(t, H):
    B, T, _ = t.shape
    return t.view(B, T, H, D).transpose(1, 2)           # [B, H, T, 128]


def _exact(q, k, v, H, scale, cos, sin):
    q, k, v = (_heads(t, H).double() for t in (q, k, v))
    if cos is not None:
        q, k = _rot(q, cos.double(), sin.double()), _rot(k, cos.double(), sin.double())
    T = q.shape[2]
    s = (q @ k.transpose(2, 3)) * scale
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu_(1), float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(q.shape[0], T, H * D)


def _chain(q, k, v, H, scale, cos, sin):
    q, k, v = (_heads(t, H) for t in (q, k, v))
    if cos is not None:
        q, k = _rot(q, cos.half(), sin.half()), _rot(k, cos.half(), sin.half())
    T = q.shape[2]
    w = torch.matmul(q, k.transpose(2, 3)) * scale
    w = w + torch.full((T, T), torch.finfo(torch.float16).min, dtype=torch.float16).triu_(1)
    w = torch.nn.functional.softmax(w, dim=-1, dtype=torch.float32).to(torch.float16)
    return torch.matmul(w, v).transpose(1, 2).contiguous().reshape(q.shape[0], T, H * D)


@functools.lru_cache(maxsize=None)
def _case(T, B, H, rope, spike):
    """Inputs and the two CPU references of one case, computed once.  spike: None, or the key j
    that is overwritten (in every head) with the inverse rotation of 0.6 * rot(q_i), i = T - 3."""
    g = torch.Generator().manual_seed(7919 * T + 31 * B + H + (17 if rope else 0))
    q, k, v = (torch.randn(B, T, H * D, generator=g).half() for _ in range(3))
    cos, sin = _table(T) if rope else (None, None)
    if spike is not None:
        i, j = T - 3, spike
        qi = q[:, i].view(B, H, D).float()
        c = torch.cat((cos, cos), -1)
        s = torch.cat((sin, sin), -1)
        kr = 0.6 * (qi * c[i] + _rotate_half(qi) * s[i])
        k = k.clone()
        k[:, j] = (kr * c[j] - _rotate_half(kr) * s[j]).reshape(B, H * D).half()
    scale = D ** -0.5
    exact = _exact(q, k, v, H, scale, cos, sin)
    e_chain = (_chain(q, k, v, H, scale, cos, sin).double() - exact).abs().max().item()
    return q, k, v, cos, sin, scale, exact, e_chain


def _kernel(q, k, v, H, scale, cos, sin):
    from ecoflap_amd.shapes import fused
    rope = None if cos is None else (cos.cuda(), sin.cuda())
    with torch.no_grad():
        out = fused.causal_attention(q.cuda(), k.cuda(), v.cuda(), H, scale, rope=rope)
    assert out is not None and out.dtype == torch.float16 and out.shape == q.shape
    return out


def _check(T, B, H, rope, spike=None):
    q, k, v, cos, sin, scale, exact, e_chain = _case(T, B, H, rope, spike)
    out = _kernel(q, k, v, H, scale, cos, sin).cpu()
    assert not torch.isnan(out).any()
    e_kernel = (out.double() - exact).abs().max().item()
    print(f"T={T} B={B} H={H} rope={rope} spike={spike}: e_kernel {e_kernel:.3e} e_chain {e_chain:.3e} "
          f"ratio {e_kernel / e_chain if e_chain else 0.0:.3f} max|A| {exact.abs().max().item():.2f}")
    if T == 1:      # the probability is 1: the output is v's row, and so is the chain's
        assert e_chain == 0.0
        assert torch.equal(out, v)
    assert e_kernel <= e_chain
    return out


SHAPES = [(T, 2, 2) for T in (1, 31, 32, 33, 64, 65, 129, 300, 513)] + [(2048, 1, 2), (129, 1, 3)]


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("T,B,H", SHAPES)
def test_not_further_from_exact_than_the_fp16_chain(T, B, H, rope):
    _check(T, B, H, rope)


@pytest.mark.parametrize("where", ["late", "first"])
@pytest.mark.parametrize("T", [129, 300, 513, 2048])
def test_a_key_that_forces_the_rescale(T, where):
    """Query T - 3 meets a key with score ~ 6.6 against ~ 2.5 for the next largest: at j = T - 70
    the running maximum jumps in a late key block and O and l of everything before are rescaled;
    at j = 2 the maximum is set in the first block and every later block is scaled against it."""
    j = T - 70 if where == "late" else 2
    q, k, v, cos, sin, scale, exact, _ = _case(T, 1, 2, True, j)
    # the planted score really towers over the row (else this test forces nothing)
    qr = _rot(_heads(q, 2).double(), cos.double(), sin.double())[0, :, T - 3]
    kr = _rot(_heads(k, 2).double(), cos.double(), sin.double())[0, :, : T - 2]
    s = torch.einsum("hd,hkd->hk", qr, kr) * scale
    top = s[:, j].clone()
    s[:, j] = float("-inf")
    assert bool((top > s.max(dim=1).values + 2.0).all())
    _check(T, 1, 2, True, spike=j)


def test_batch_invariant_and_repeatable_bit_for_bit():
    T, B, H = 65, 3, 2
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(B, T, H * D, generator=g).half() for _ in range(3))
    cos, sin = _table(T)
    whole = _kernel(q, k, v, H, D ** -0.5, cos, sin)
    again = _kernel(q, k, v, H, D ** -0.5, cos, sin)
    assert torch.equal(whole, again)
    for b in range(B):
        alone = _kernel(q[b:b + 1].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous(), H,
                        D ** -0.5, cos, sin)
        assert torch.equal(alone[0], whole[b]), b


def test_slices_of_one_buffer_and_a_strided_output():
    """q, k and v as three slices of one [B, T, 3 * H * 128] buffer give the bits of three separate
    tensors; an `out` whose token stride is longer than a row keeps its gap bytes."""
    import ctypes
    from ecoflap_amd import hip
    from ecoflap_amd.shapes import fused
    T, B, H = 65, 2, 2
    C = H * D
    g = torch.Generator().manual_seed(6)
    qkv = torch.randn(B, T, 3 * C, generator=g).half().cuda()
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    cos, sin = (t.cuda() for t in _table(T))
    with torch.no_grad():
        sliced = fused.causal_attention(q, k, v, H, D ** -0.5, rope=(cos, sin))
        apart = fused.causal_attention(q.contiguous(), k.contiguous(), v.contiguous(), H, D ** -0.5,
                                       rope=(cos, sin))
    assert sliced is not None and apart is not None and torch.equal(sliced, apart)
    fused._get()
    lib = hip.load_library()
    wide = torch.full((B, T, C + 64), 7.0, dtype=torch.float16, device="cuda")
    rc = lib.ecoflap_causal_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), wide.data_ptr(),
                                      cos.data_ptr(), sin.data_ptr(), B, T, H, D, q.stride(1), q.stride(0),
                                      wide.stride(1), wide.stride(0), D ** -0.5, 1,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(wide[..., :C], sliced)
    assert bool((wide[..., C:] == 7.0).all())


def test_refused_inputs_return_none():
    from ecoflap_amd.shapes import fused
    ok = [torch.randn(2, 8, 2 * D, device="cuda").half() for _ in range(3)]
    cos, sin = (t.cuda() for t in _table(8))
    with torch.no_grad():
        assert fused.causal_attention(*ok, 2, D ** -0.5, rope=(cos, sin)) is not None
        assert fused.causal_attention(*ok, 4, 64 ** -0.5) is None                       # head width 64
        assert fused.causal_attention(*[t.bfloat16() for t in ok], 2, D ** -0.5) is None
        assert fused.causal_attention(*[t.cpu() for t in ok], 2, D ** -0.5) is None
        assert fused.causal_attention(*ok, 2, 0.0) is None
        assert fused.causal_attention(ok[0], ok[1], ok[2][:, :4], 2, D ** -0.5) is None  # shapes differ
        assert fused.causal_attention(*ok, 2, D ** -0.5, rope=(cos[:4], sin[:4])) is None
        long = [torch.zeros(1, 4097, D, device="cuda").half() for _ in range(3)]
        assert fused.causal_attention(*long, 1, D ** -0.5) is None
    assert fused.causal_attention(*ok, 2, D ** -0.5) is None                            # autograd on
