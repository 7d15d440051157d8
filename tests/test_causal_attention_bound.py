"""CPU: the a-priori error bound `attention_reference.exact_and_bound_stream` of the streaming causal
kernel (csrc/attention_stream.h, csrc/causal_attention.hip) separates the arithmetic the kernel
documents from two faults that the criterion of tests/test_causal_attention_gpu.py (one number per
tensor, Gaussian data of amplitude 1) lets through, before any GPU runs: `emulate_stream` stays
within the bound on every input builder; with fp16-subnormal probabilities flushed to zero it leaves
it on `subnormal_p`, `subnormal_p_late` and `gauss(1.7)`; with one padded key leaking into the row
sum of the last 32-query tile it leaves it on `equal_keys`.  The rotation as the kernel documents
it, `rotate_documented`, is held to the fp64 rotation, and the three exact tables to their
permutations.

max |emulated - exact| / bound at 128 wide, B = H = 2, T in {65, 257, 300, 513}:
    documented arithmetic   0.80 at most (`subnormal_p`, 513 tokens); `subnormal_p_late` 0.76
    flush                   166 - 167 on `subnormal_p`, 42 - 166 on `subnormal_p_late`,
                            8.7 - 15.5 on gauss(1.7)
    leak                    1.67 / 12.5 / 2.80 on `equal_keys` at 257 / 300 / 513 tokens"""
import functools

import pytest
import torch

import attention_reference as ref

D = 128
B, H = 2, 2
TOKENS = [65, 257, 300, 513]
SCALE = D ** -0.5


@functools.lru_cache(maxsize=None)
def _case(name, T):
    q, k, v = ref.build_stream(name, B, H, T)
    A, bound = ref.exact_and_bound_stream(q, k, v, SCALE)
    return q, k, v, A, bound


def _worst(name, T, fault):
    q, k, v, A, bound = _case(name, T)
    out = ref.emulate_stream(q, k, v, SCALE, fault=fault)
    assert out.dtype == torch.float16 and not torch.isnan(out).any()
    worst = ((out.double() - A).abs() / bound).max().item()
    print(f"{name} T={T} fault={fault}: worst {worst:.3f}")
    return worst


@pytest.mark.parametrize("name", list(ref.STREAM_BUILDERS))
@pytest.mark.parametrize("T", TOKENS)
def test_documented_arithmetic_is_within_the_bound(T, name):
    assert _worst(name, T, None) <= 1.0
    if name == "equal_rows":
        q, k, v, _, _ = _case(name, T)
        assert torch.equal(ref.emulate_stream(q, k, v, SCALE), v)


@pytest.mark.parametrize("name", ["subnormal_p", "subnormal_p_late", "gauss1.7"])
@pytest.mark.parametrize("T", TOKENS)
def test_flushed_subnormal_probabilities_exceed_the_bound(T, name):
    assert _worst(name, T, "flush") > 1.0


@pytest.mark.parametrize("T", [257, 300, 513])
def test_a_key_leaked_into_the_last_query_tile_exceeds_the_bound(T):
    assert _worst("equal_keys", T, "leak") > 1.0


def test_the_stream_bound_is_the_two_pass_bound_with_per_row_counts():
    """Same exact result; and the streaming bound differs from the two-pass one only in its
    u32 counts (per row and per block instead of the global N), so at 513 tokens the two lie
    within 513 * u32 / u16 of each other: no term of the order of u16 was added or lost."""
    q, k, v, A, bound = _case("gauss1.7", 513)
    A2, bound2 = ref.exact_and_bound(q, k, v, SCALE, True)
    assert torch.equal(A, A2)
    assert ((bound / bound2 - 1).abs().max().item()) < 2 * 513 * ref.U32 / ref.U16


@pytest.mark.parametrize("T", TOKENS)
def test_subnormal_p_late_rescales_and_then_goes_subnormal(T):
    """The builder's own precondition, from the fp64 scores of the last query's row.  From 71 tokens
    on: what lies before the towering key was accumulated at normal probabilities (the smallest
    above 1/2 of its own maximum) and is rescaled by alpha < 2^-14; more than 90 % of the keys
    after it have probabilities in (0, 2^-14); V of the towering key is zero and the output is not.
    At 65 tokens the key sits at 0 and the builder is `subnormal_p`'s layout."""
    q, k, v, A, _ = _case("subnormal_p_late", T)
    j = ref.late_key(T)
    alpha, before, after = ref.late_key_profile(q, k, SCALE)
    print(f"T={T} key {j}: alpha {alpha.max().item():.3e} before {before.min().item():.3f} "
          f"after {after.min().item():.4f}")
    assert bool((after > 0.9).all())
    if T >= 71:
        assert j == T - 70 and j // 64 < (T - 1) // 64        # a later block follows the key's own
        assert bool((alpha < ref.P_SUBNORMAL).all()) and bool((alpha > 0).all())
        assert bool((before > 0.5).all())
    else:
        assert j == 0 and bool((ref.subnormal_fraction(q, k, SCALE, True) > 0.9).all())
    assert bool((v[:, :, j] == 0).all()) and A[:, :, -1].abs().min().item() > 0


# ---- the rotation -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["gauss0.3", "gauss1.7", "gauss8.0"])
@pytest.mark.parametrize("T", TOKENS)
def test_rotate_documented_against_the_fp64_rotation(T, name):
    """Each element within u16 * |x'| + 2 * u32 * (|lo c| + |hi s|) of the fp64 rotation of the same
    fp16 input by the same fp32 table: two products and a sum rounded to fp32 (the sum is at most
    |lo c| + |hi s|), one rounding to fp16.  The fp16 term is relative, so it describes results in the
    normal range, |x'| >= 2^-14; the few results below it (printed) are held to half the subnormal
    spacing, 2^-25, in its place."""
    x = ref.build_stream(name, B, H, T)[0]
    cos, sin = ref.rope_table(T)
    got = ref.rotate_documented(x, cos, sin).double()
    lo, hi, c, s = x[..., :64].double(), x[..., 64:].double(), cos.double(), sin.double()
    want = torch.cat((lo * c - hi * s, hi * c + lo * s), dim=-1)
    mag = torch.cat(((lo * c).abs() + (hi * s).abs(), (hi * c).abs() + (lo * s).abs()), dim=-1)
    allowed = ref.U16 * want.abs() + 2 * ref.U32 * mag
    normal = want.abs() >= ref.P_SUBNORMAL
    print(f"{name} T={T}: worst {((got - want).abs() / allowed)[normal].max().item():.3f}, "
          f"{int((~normal).sum())} of {normal.numel()} results below 2^-14")
    assert bool(((got - want).abs() <= allowed)[normal].all())
    # below the normal range the fp16 spacing is 2^-24: half of it, and the same fp32 terms
    assert bool(((got - want).abs() <= 2.0 ** -25 + 2 * ref.U32 * mag)[~normal].all())


@pytest.mark.parametrize("T", TOKENS)
def test_the_exact_tables_permute_bit_for_bit(T):
    x = ref.build_stream("gauss1.7", B, H, T)[0]
    assert torch.equal(ref.rotate_documented(x, *ref.identity_table(T)), x)
    assert torch.equal(ref.rotate_documented(x, *ref.swap_table(T)), ref.swap_halves(x))
    par = ref.rotate_documented(x, *ref.parity_table(T))
    assert torch.equal(par, ref.swap_halves(x, odd_only=True))
    assert torch.equal(par[..., 0::2, :], x[..., 0::2, :])
    assert torch.equal(par[..., 1::2, :64], -x[..., 1::2, 64:]) and torch.equal(par[..., 1::2, 64:], x[..., 1::2, :64])


def test_rope_table_is_the_rotary_embedding():
    cos, sin = ref.rope_table(300)
    assert cos.dtype == torch.float32 and cos.shape == sin.shape == (300, 64)
    pos = torch.arange(300, dtype=torch.float64)[:, None]
    freq = 10000.0 ** (-torch.arange(0, 128, 2, dtype=torch.float64) / 128)
    # fp32 angles up to 299 carry an error of up to 299 * 2^-24 * a few
    assert (cos.double() - (pos * freq).cos()).abs().max().item() < 1e-4
    assert (sin.double() - (pos * freq).sin()).abs().max().item() < 1e-4
