"""The global-threshold pruning kernels (csrc/global_prune.hip) at their selection edges, bit for
bit against the numpy reference of tests/global_prune_reference.py (pinned against the torch
oracle by tests/test_global_prune_reference.py): masks, weight bit patterns, accumulators and
zero counts.  Every array lives inside a larger buffer between sentinel elements, which no call
may change.  Run on an MI355X with `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import global_prune_reference as R
from helpers import NP2T
from test_global_prune_reference import GROUPS, group_cases

pytestmark = pytest.mark.gpu

PAD = 16                                  # elements: keeps a 16-byte alignment for every dtype
W_SENTINEL = {"f32": 0x4b3c614e, "f16": 0x5a5a, "bf16": 0x5a5a}
ACC_SENTINEL = 0x4b3c614e
MASK_SENTINEL = 0xa5
DEVICE = "cuda"


@pytest.fixture(scope="module")
def kern():
    from ecoflap_amd import hip
    assert torch.cuda.is_available()
    return hip.HipKernels()


class Buf:
    """`data` at element `PAD + off` of a device buffer filled with a sentinel; .t is the view
    the kernels get."""

    def __init__(self, data, sentinel, off=0, torch_dtype=None):
        self.n, self.at = data.size, PAD + off
        host = np.full(self.at + self.n + PAD, sentinel, dtype=data.dtype)
        host[self.at:self.at + self.n] = data
        self.sentinel = host.copy()
        signed = {1: np.uint8, 2: np.int16, 4: np.int32}[data.dtype.itemsize]
        self.np_dtype = data.dtype
        self.buf = torch.from_numpy(host.view(signed)).to(DEVICE)
        self.t = self.buf[self.at:self.at + self.n]
        if torch_dtype is not None:
            self.t = self.t.view(torch_dtype)
        assert self.t.is_contiguous() and self.t.data_ptr() % data.dtype.itemsize == 0
        assert (self.t.data_ptr() % 16 == 0) == (off * data.dtype.itemsize % 16 == 0)

    def read(self):
        """(the data, whether everything around it still holds the sentinel)"""
        host = self.buf.cpu().numpy().view(self.np_dtype).copy()
        got = host[self.at:self.at + self.n].copy()
        host[self.at:self.at + self.n] = self.sentinel[self.at:self.at + self.n]
        return got, bool(np.array_equal(host, self.sentinel))


def f32_buf(acc, off=0):
    return Buf(acc.view(np.uint32), ACC_SENTINEL, off, torch.float32)


def w_buf(bits, dt, off=0):
    return Buf(bits, W_SENTINEL[dt], off, NP2T[dt])


def run_hip(kern, case, offsets=(0, 0, 0)):
    """The whole case through HipKernels.  Returns (accumulator bits, per round {"w", "mask"},
    sentinels intact)."""
    layers = case.layers
    w = [w_buf(l.w, l.dt, offsets[0]) for l in layers]
    acc = [None if l.acc is None else f32_buf(l.acc, offsets[1]) for l in layers]
    mask = [Buf(l.mask, MASK_SENTINEL, offsets[2]) for l in layers]
    intact = True
    for step in case.grad_steps or []:
        g = [w_buf(bits, l.dt) for l, bits in zip(layers, step)]
        kern.grad_accum_multi([a.t for a in acc], [x.t for x in g])
        for x, bits in zip(g, step):
            after, ok = x.read()
            intact &= ok and bool(np.array_equal(after, bits))
    accs = [None if a is None else a.read()[0] for a in acc]
    rounds = []
    for k, prot in case.rounds:
        kern.global_threshold_prune([x.t for x in w], None if case.mode == 3 else [a.t for a in acc],
                                    [m.t for m in mask], case.mode, case.n_batches, k, prot)
        rounds.append({"w": [x.read()[0] for x in w], "mask": [m.read()[0] for m in mask]})
    for b in w + mask + [a for a in acc if a is not None]:
        intact &= b.read()[1]
    for a, before in zip(acc, accs):          # a prune call reads the accumulators only
        intact &= a is None or bool(np.array_equal(a.read()[0], before))
    return accs, rounds, intact


def compare(case, got, want, bad, tag=""):
    """got / want: (accumulators, rounds).  Appends what differs to `bad`."""
    for li, (a, b) in enumerate(zip(got[0], want[0])):
        if b is not None and not np.array_equal(a, b.view(np.uint32)):
            bad.append((case.name, tag, "acc", li))
    for i, ((k, _), fixed, r, ref) in enumerate(zip(case.rounds, case.pruned, got[1], want[1])):
        for what in ("mask", "w"):
            for li, (x, y) in enumerate(zip(r[what], ref[what])):
                if not np.array_equal(x, y):
                    bad.append((case.name, tag, f"round {i}", what, f"layer {li}", int((x != y).sum())))
        # independent of the reference's masks: the zeros a threshold at rank k must leave
        zeros = sum(int((m == 0).sum()) for m in r["mask"])
        if zeros < k or zeros != ref["removed"] or (fixed is not None and zeros != fixed):
            bad.append((case.name, tag, f"round {i}", "zeros", zeros, "k", k, "score<=thr", ref["removed"],
                        "by construction", fixed))
        if not all(set(np.unique(m)) <= {0, 1} for m in r["mask"]):
            bad.append((case.name, tag, f"round {i}", "mask bytes"))


@pytest.mark.parametrize("group", GROUPS)
def test_selection_edges(kern, group):
    bad = []
    for case in group_cases(group):
        accs, rounds, intact = run_hip(kern, case)
        compare(case, (accs, rounds), R.run_case(case), bad)
        if not intact:
            bad.append((case.name, "sentinels or inputs changed"))
    assert not bad, bad


def test_protected_then_plain_reuses_the_workspace(kern):
    """A plain call after a protected one on the same HipKernels (its workspace still holds the
    per-layer states and keys) equals the same plain call on a fresh HipKernels."""
    from ecoflap_amd import hip
    for mode in (0, 3):
        base = R.prune_cases()[f"protect-then-plain-mode{mode}"]
        assert base.rounds[0][1] is not None and base.rounds[1][1] is None
        want = R.run_case(base)
        _, chained, ok0 = run_hip(kern, base)
        after = base.clone()
        for l, w, m in zip(after.layers, chained[0]["w"], chained[0]["mask"]):
            l.w, l.mask = w, m
        plain = R.Case(base.name + "-plain", after.layers, mode, base.n_batches, [base.rounds[1]])
        _, fresh, ok1 = run_hip(hip.HipKernels(), plain)
        assert ok0 and ok1
        for what in ("mask", "w"):
            for x, y, ref in zip(chained[1][what], fresh[0][what], want[1][1][what]):
                assert np.array_equal(x, y) and np.array_equal(x, ref), (mode, what)


def test_misaligned_views(kern):
    """The ng = 0 scalar fallback: w, acc and mask offset inside their buffers, each alone and
    all together, equal the aligned run and the reference; the neighbours stay untouched."""
    bad = []
    for case in R.alignment_cases():
        want = R.run_case(case)
        runs = {tag: run_hip(kern, case, off) for tag, off in R.OFFSETS.items()}
        for tag, (accs, rounds, intact) in runs.items():
            compare(case, (accs, rounds), want, bad, tag)
            if not intact:
                bad.append((case.name, tag, "sentinels or inputs changed"))
            for what in ("mask", "w"):
                if not np.array_equal(rounds[0][what][0], runs["aligned"][1][0][what][0]):
                    bad.append((case.name, tag, what, "differs from the aligned run"))
    assert not bad, bad


def test_grad_accum_multi_edges(kern):
    rows = R.grad_accum_rows()
    acc = [f32_buf(a, off) for _, a, _, off, _ in rows]
    g = [w_buf(bits, dt, off) for dt, _, bits, _, off in rows]
    assert sum(b.t.data_ptr() % 16 != 0 for b in acc) == 1 and sum(b.t.data_ptr() % 16 != 0 for b in g) == 1
    kern.grad_accum_multi([b.t for b in acc], [b.t for b in g])
    for (dt, a, bits, _, _), ab, gb in zip(rows, acc, g):
        got, intact = ab.read()
        want = R.grad_accum(a, bits, dt).view(np.uint32)
        assert np.array_equal(got, want), (dt, a.size, int((got != want).sum()))
        g_after, g_intact = gb.read()
        assert intact and g_intact and np.array_equal(g_after, bits), (dt, a.size)


def test_count_zeros_multi_edges(kern):
    rows = R.count_zero_rows()
    bufs = [w_buf(bits, dt, off) for dt, bits, off in rows]
    assert any(b.t.data_ptr() % 16 != 0 for b in bufs)
    want = [R.count_zeros(bits, dt) for dt, bits, _ in rows]
    assert kern.count_zeros_multi([b.t for b in bufs]) == want
    for b, (dt, bits, _) in zip(bufs, rows):
        got, intact = b.read()
        assert intact and np.array_equal(got, bits), (dt, bits.size)
