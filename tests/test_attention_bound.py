"""CPU: the a-priori error bound of tests/attention_reference.py separates the arithmetic that
csrc/attention_tile.h documents from two faults the older tolerance (4e-3 of the output scale) lets
through, before any GPU runs: `emulate_tile` stays within the bound on every input builder, with
fp16-subnormal probabilities flushed to zero it leaves it on `subnormal_p` and `gauss(1.7)`, and
with one padded key leaking into the row sum it leaves it on `equal_keys`.

max |emulated - exact| / bound over these cases: 0.78 for the documented arithmetic (`subnormal_p`,
causal); flush 4.0 - 12 on gauss(1.7), 168 on `subnormal_p`; leak 28 - 770 on `equal_keys`."""
import functools

import pytest
import torch

import attention_reference as ref

CASES = [(257, 88, False), (77, 64, True), (33, 64, False)]       # (N, D, causal)
B, H = 2, 2


@functools.lru_cache(maxsize=None)
def _case(name, N, D, causal):
    q, k, v = ref.build(name, B, H, N, D, causal=causal)
    scale = D ** -0.5
    A, bound = ref.exact_and_bound(q, k, v, scale, causal)
    return q, k, v, scale, A, bound


def _worst(name, N, D, causal, fault):
    q, k, v, scale, A, bound = _case(name, N, D, causal)
    out = ref.emulate_tile(q, k, v, scale, causal, fault=fault)
    assert out.dtype == torch.float16 and not torch.isnan(out).any()
    worst = ((out.double() - A).abs() / bound).max().item()
    print(f"{name} N={N} D={D} causal={causal} fault={fault}: worst {worst:.3f}")
    return worst


@pytest.mark.parametrize("name", list(ref.BUILDERS))
@pytest.mark.parametrize("N,D,causal", CASES)
def test_documented_arithmetic_is_within_the_bound(N, D, causal, name):
    assert _worst(name, N, D, causal, None) <= 1.0
    if name == "equal_rows":
        q, k, v, scale, _, _ = _case(name, N, D, causal)
        assert torch.equal(ref.emulate_tile(q, k, v, scale, causal), v)


@pytest.mark.parametrize("name", ["subnormal_p", "gauss1.7"])
@pytest.mark.parametrize("N,D,causal", CASES)
def test_flushed_subnormal_probabilities_exceed_the_bound(N, D, causal, name):
    assert _worst(name, N, D, causal, "flush") > 1.0


@pytest.mark.parametrize("N,D,causal", CASES)
def test_a_leaked_padded_key_exceeds_the_bound(N, D, causal):
    assert _worst("equal_keys", N, D, causal, "leak") > 1.0


@pytest.mark.parametrize("N,D,causal", CASES)
def test_subnormal_p_puts_the_row_into_the_subnormal_range(N, D, causal):
    """The builder's own precondition, from the fp64 scores: more than 90 % of the probabilities of
    a row that sees every key lie in (0, 2^-14), and they carry the whole output (V of the one
    large key is zero)."""
    q, k, v, scale, A, _ = _case("subnormal_p", N, D, causal)
    frac = ref.subnormal_fraction(q, k, scale, causal)
    print(f"N={N} D={D} causal={causal}: subnormal fraction {frac.min().item():.4f}")
    assert bool((frac > 0.9).all())
    assert bool((v[:, :, 0] == 0).all()) and A[:, :, -1].abs().min().item() > 0


def test_equal_keys_probabilities_are_one_over_visible():
    q, k, v, scale, A, _ = _case("equal_keys", 77, 64, True)
    n = torch.arange(1, 78, dtype=torch.float64)[:, None]
    mean = v.double().cumsum(dim=2) / n
    assert (A - mean).abs().max().item() < 1e-12
