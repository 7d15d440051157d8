"""The numpy reference of the global-threshold pruning kernels (global_prune_reference.py)
against the torch oracle, on the CPU, on every edge case the GPU test uses: masks, weight bit
patterns, accumulators and zero counts.  This pins the reference before it judges a kernel."""
import numpy as np
import pytest
import torch

import global_prune_reference as R
from helpers import NP2T, from_bits, to_bits

GROUPS = ("consecutive", "runs", "degenerate", "fullrange", "signed", "mixed", "overflow", "protect")


def group_cases(group):
    cases = [c for name, c in R.prune_cases().items() if name.startswith(group + "-")]
    assert cases, group
    return cases


def to_torch(bits, dt):
    return from_bits(bits.view(np.int32 if dt == "f32" else np.int16).copy(), NP2T[dt])


def bits_of(t, dt):
    return to_bits(t).view(R.UINT[dt]).copy()          # to_bits shares a CPU tensor's memory


@pytest.fixture(scope="module")
def orc(oracle):
    from oracle_backend import OracleKernels
    return OracleKernels()


def run_oracle(orc, case):
    c = case.clone()
    w = [to_torch(l.w, l.dt) for l in c.layers]
    acc = [None if l.acc is None else torch.from_numpy(l.acc) for l in c.layers]
    mask = [torch.from_numpy(l.mask) for l in c.layers]
    for step in c.grad_steps or []:
        orc.grad_accum_multi(acc, [to_torch(g, l.dt) for l, g in zip(c.layers, step)])
    accs = [None if a is None else a.numpy().copy() for a in acc]
    rounds = []
    for k, prot in c.rounds:
        orc.global_threshold_prune(w, None if c.mode == 3 else acc, mask, c.mode, c.n_batches, k, prot)
        rounds.append({"w": [bits_of(t, l.dt) for t, l in zip(w, c.layers)],
                       "mask": [m.numpy().copy() for m in mask]})
    return accs, rounds


def check_reference_itself(case, rounds):
    """What a case fixes by construction, and the count that needs no sort."""
    for (k, _), want, r in zip(case.rounds, case.pruned, rounds):
        zeros = sum(int((m == 0).sum()) for m in r["mask"])
        assert zeros >= k and zeros == r["removed"], (case.name, k, zeros, r["removed"])
        assert want is None or zeros == want, (case.name, k, zeros, want)
        assert all(set(np.unique(m)) <= {0, 1} for m in r["mask"])


@pytest.mark.parametrize("group", GROUPS)
def test_reference_equals_oracle(orc, group):
    bad = []
    for case in group_cases(group):
        accs, rounds = R.run_case(case)
        check_reference_itself(case, rounds)
        o_accs, o_rounds = run_oracle(orc, case)
        for a, b in zip(accs, o_accs):
            if a is not None and not np.array_equal(a, b, equal_nan=True):
                bad.append((case.name, "acc"))
        for i, (r, o) in enumerate(zip(rounds, o_rounds)):
            for what in ("mask", "w"):
                if not all(np.array_equal(x, y) for x, y in zip(r[what], o[what])):
                    bad.append((case.name, i, what))
    assert not bad, bad


def test_alignment_cases_equal_oracle(orc):
    for case in R.alignment_cases():
        _, rounds = R.run_case(case)
        check_reference_itself(case, rounds)
        _, o_rounds = run_oracle(orc, case)
        for r, o in zip(rounds, o_rounds):
            assert np.array_equal(r["mask"][0], o["mask"][0]) and np.array_equal(r["w"][0], o["w"][0]), case.name


def test_nan_scores_rank_last(orc):
    """The overflow cases really hold what they are for: NaN scores that sort above +inf."""
    case = R.prune_cases()["overflow-nan0"]
    _, rounds = R.run_case(case)
    allv = np.sort(np.concatenate(rounds[0]["scores"]))
    assert np.isnan(allv[-3:]).all() and np.isinf(allv[-7:-3]).all() and np.isfinite(allv[:-7]).all()
    assert np.isnan(rounds[0]["thr"]) and rounds[0]["removed"] == case.total
    _, below = R.run_case(R.prune_cases()["overflow-below"])
    assert below[0]["removed"] == case.total // 2 + 3          # a NaN score is never kept


def test_grad_accum_reference_equals_oracle(orc):
    rows = R.grad_accum_rows()
    assert {dt for dt, *_ in rows} == set(R.DTS) and max(a.size for _, a, *_ in rows) == R.ACCUM_WRAP
    accs = [torch.from_numpy(a.copy()) for _, a, _, _, _ in rows]
    orc.grad_accum_multi(accs, [to_torch(g, dt) for dt, _, g, _, _ in rows])
    for (dt, a, g, _, _), got in zip(rows, accs):
        want = R.grad_accum(a, g, dt)
        assert want.dtype == np.float32
        assert np.array_equal(want.view(np.uint32), got.numpy().view(np.uint32)), (dt, a.size)
    dt, a, g, _, _ = rows[2]                 # the planted head: -0 onto +0, inf, the two roundings
    head = R.grad_accum(a, g, dt)[:7]
    assert head.view(np.uint32)[0] == 0 and np.isinf(head[3]) and np.isinf(head[4])
    assert head[5] == np.float32(16777216.0) and head[6] == np.float32(1.0)


def test_zero_count_reference_equals_oracle(orc):
    rows = R.count_zero_rows()
    want = [R.count_zeros(bits, dt) for dt, bits, _ in rows]
    assert orc.count_zeros_multi([to_torch(bits, dt) for dt, bits, _ in rows]) == want
    for (dt, bits, _), n in zip(rows, want):
        sign = R.SIGN[dt]
        assert n == int(((bits == 0) | (bits == sign)).sum()), (dt, bits.size)    # the two zeros only
    assert want[:4] == [2, 1, 0, 9]
