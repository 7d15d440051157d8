"""Plain numpy reference of csrc/global_prune.hip, and the edge cases that judge it.

The kernels' header states the arithmetic; it is restated here fp32 op for op:

    a      = acc / float32(n_batches)
    score  = |w|*|a|  (mode 0),  (w*w)*a  (1),  |a|  (2),  w  (3: the signed weight)
    score *= float32(mask)
    protection, per layer with num_to_set > 0:
             thr_l = sort(score_l)[numel - num_to_set];  score_l[score_l >= thr_l] = FLT_MAX
    thr    = sort(concat(scores))[k - 1]          np.sort puts NaN last, as torch.topk does
    keep   = score > thr
    w      = w * keep in w's own dtype, i.e. a pruned weight is a zero with w's sign

plus acc + |float32(g)| for the accumulate and `x == 0` for the zero count (both zeros count,
denormals and NaN do not).  Weights and gradients travel as bit patterns (uint16 / uint32), so
that bf16 needs no numpy dtype and every comparison is bit for bit.

tests/test_global_prune_reference.py pins this module against the torch oracle on the CPU;
tests/test_global_prune_edges_gpu.py holds the HIP kernels to it.  Both take their inputs from
the case builders below.
"""
import copy

import numpy as np

DTS = ("f32", "f16", "bf16")
UINT = {"f32": np.uint32, "f16": np.uint16, "bf16": np.uint16}
SIGN = {"f32": 0x80000000, "f16": 0x8000, "bf16": 0x8000}
FLT_MAX_BITS = 0x7f7fffff
INF_BITS = 0x7f800000
FLT_MAX = np.array([FLT_MAX_BITS], np.uint32).view(np.float32)[0]

# one sweep of the selection / zero-count grids is 64 blocks x 256 lanes x 8 elements, of the
# accumulate grid 256 x 256 x 8: these sizes send three groups of 8 round a second time and
# leave a scalar tail of 5
WRAP = 64 * 256 * 8 + 29
ACCUM_WRAP = 256 * 256 * 8 + 29


def f32_from_bits(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def decode(bits, dt):
    """bit patterns of `dt` -> fp32, exactly."""
    if dt == "f32":
        return bits.view(np.float32)
    if dt == "f16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def encode(x, dt):
    """fp32 (no NaN) -> bit patterns of `dt`, round to nearest even; what would round to inf
    becomes the largest finite value, so that no case holds an inf weight by accident."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dt == "f32":
        return x.view(np.uint32).copy()
    if dt == "f16":
        with np.errstate(over="ignore"):
            b = x.astype(np.float16).view(np.uint16).copy()
        b[(b & 0x7fff) == 0x7c00] -= 1
        return b
    u = x.view(np.uint32).astype(np.uint64)
    b = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    b[(b & 0x7fff) == 0x7f80] -= 1
    return b


class Layer:
    def __init__(self, dt, w, acc=None, mask=None):
        self.dt = dt
        self.w = np.ascontiguousarray(w, dtype=UINT[dt])
        self.acc = None if acc is None else np.ascontiguousarray(acc, dtype=np.float32)
        self.mask = (np.ones(self.w.size, np.uint8) if mask is None
                     else np.ascontiguousarray(mask, dtype=np.uint8))
        assert self.acc is None or self.acc.size == self.w.size
        assert self.mask.size == self.w.size

    @property
    def n(self):
        return self.w.size


class Case:
    """layers, then optionally `grad_steps` accumulate calls (grad_steps[s][l]: bit patterns of
    layer l's own dtype) into the accumulators, then `rounds` = [(k, protect_counts or None)]
    chained on the same weights and masks.  `pruned`: per round the number of zeros the new
    masks must hold where the case fixes it by construction, else None."""

    def __init__(self, name, layers, mode, n_batches, rounds, grad_steps=None, pruned=None):
        self.name, self.layers, self.mode, self.n_batches = name, layers, mode, n_batches
        self.rounds, self.grad_steps = rounds, grad_steps
        self.pruned = pruned if pruned is not None else [None] * len(rounds)
        self.total = sum(l.n for l in layers)
        for k, prot in rounds:
            assert 1 <= k <= self.total, (name, k)
            assert prot is None or len(prot) == len(layers)

    def clone(self):
        return copy.deepcopy(self)


# ------------------------------------------------------------------------------ the reference
def grad_accum(acc, g_bits, dt):
    with np.errstate(all="ignore"):
        return acc + np.abs(decode(g_bits, dt))


def count_zeros(bits, dt):
    return int((decode(bits, dt) == 0).sum())


def scores(layer, mode, n_batches):
    w = decode(layer.w, layer.dt)
    with np.errstate(all="ignore"):
        if mode == 3:
            s = w.copy()
        else:
            a = layer.acc / np.float32(n_batches)
            if mode == 0:
                s = np.abs(w) * np.abs(a)
            elif mode == 1:
                s = (w * w) * a
            else:
                s = np.abs(a)
        s = s * layer.mask.astype(np.float32)
    assert s.dtype == np.float32
    return s


def prune_round(layers, mode, n_batches, k, protect_counts=None):
    """One round in place.  Returns (thr, the scores the threshold was taken over)."""
    sc = [scores(l, mode, n_batches) for l in layers]
    if protect_counts is not None:
        for s, num_to_set in zip(sc, protect_counts):
            if num_to_set > 0:
                thr_l = np.sort(s)[s.size - int(num_to_set)]
                s[s >= thr_l] = FLT_MAX
    thr = np.sort(np.concatenate(sc))[k - 1]
    for l, s in zip(layers, sc):
        with np.errstate(invalid="ignore"):
            keep = s > thr
        l.mask = keep.astype(np.uint8)
        l.w = np.where(keep, l.w, l.w & UINT[l.dt](SIGN[l.dt])).astype(UINT[l.dt])
    return thr, sc


def count_not_above(sc, thr):
    """How many scores a threshold removes, counted without a sort: score <= thr, and every NaN
    score (`NaN > thr` is false, so a NaN score is never kept); a NaN threshold removes all."""
    allv = np.concatenate(sc)
    if np.isnan(thr):
        return allv.size
    with np.errstate(invalid="ignore"):
        return int((allv <= thr).sum() + np.isnan(allv).sum())


def run_case(case):
    """The whole case on a copy.  Returns (accumulators after the accumulate calls, per round
    {"w": bits per layer, "mask": per layer, "thr", "scores", "removed"})."""
    c = case.clone()
    for step in c.grad_steps or []:
        for l, g in zip(c.layers, step):
            l.acc = grad_accum(l.acc, g, l.dt)
    accs = [None if l.acc is None else l.acc.copy() for l in c.layers]
    rounds = []
    for k, prot in c.rounds:
        thr, sc = prune_round(c.layers, c.mode, c.n_batches, k, prot)
        rounds.append({"w": [l.w.copy() for l in c.layers], "mask": [l.mask.copy() for l in c.layers],
                       "thr": thr, "scores": sc, "removed": count_not_above(sc, thr)})
    return accs, rounds


# ------------------------------------------------------------------------------ case builders
def _split(arr, sizes):
    assert sum(sizes) == arr.size
    out, at = [], 0
    for s in sizes:
        out.append(arr[at:at + s])
        at += s
    return out


def _acc_layers(acc_bits, sizes, dt="f32"):
    """mode 2 with n_batches = 1: score == acc bit for bit; the weights only get pruned."""
    rng = np.random.default_rng(acc_bits.size)
    out = []
    for part in _split(acc_bits, sizes):
        w = encode(rng.choice(np.array([-2.5, -1.0, 0.75, 3.0], np.float32), part.size), dt)
        out.append(Layer(dt, w, f32_from_bits(part)))
    return out


def _consecutive():
    rng = np.random.default_rng(1)
    bits = (0x3f800000 - 1500 + np.arange(3000)).astype(np.uint32)
    assert len({int(b) >> 21 for b in bits}) == 2 and len({(int(b) >> 10) & 2047 for b in bits}) > 2
    bits = bits[rng.permutation(3000)]
    for k in (1, 2, 1499, 1500, 1501, 1502, 2999, 3000):
        yield Case(f"consecutive-k{k}", _acc_layers(bits, (1, 999, 2000)), 2, 1, [(k, None)], pruned=[k])


def _runs():
    rng = np.random.default_rng(2)
    lens = [1 + 13 * (j % 5) for j in range(50)]
    bits = np.concatenate([np.full(n, 0x3f000000 + 7 * j, np.uint32) for j, n in enumerate(lens)])
    ends = np.cumsum(lens)
    assert bits.size == 1350
    bits = bits[rng.permutation(bits.size)]
    for j in (0, 1, 4, 27, 48, 49):
        first, last = int(ends[j]) - lens[j] + 1, int(ends[j])
        for k in sorted({first, (first + last) // 2, last}):
            yield Case(f"runs-j{j}-k{k}", _acc_layers(bits, (1, 449, 900)), 2, 1, [(k, None)],
                       pruned=[last])


def _degenerate():
    n = 3000
    for k in (1, n):
        yield Case(f"degenerate-equal-k{k}", _acc_layers(np.full(n, 0x3fc00000, np.uint32), (1, 999, 2000)),
                   2, 1, [(k, None)], pruned=[n])
        layers = _acc_layers((0x3f800000 + np.arange(n)).astype(np.uint32), (1, 999, 2000))
        for l in layers:
            l.mask[:] = 0
        yield Case(f"degenerate-masked-k{k}", layers, 2, 1, [(k, None)], pruned=[n])


FULL_SIZES = (WRAP, 1, 7, 8, 9, 15)


def _full_range():
    n = sum(FULL_SIZES)
    for k in (1, n // 3, n - 3, n - 2, n):
        rng = np.random.default_rng(3)
        bits = rng.integers(0, INF_BITS + 1, n, dtype=np.uint64).astype(np.uint32)
        # planted: in the first group of 8, in a group of the second sweep, in the scalar tail
        # of the WRAP layer, and in the small layers behind it
        bits[3] = 0
        bits[64 * 256 * 8 + 9] = 0x00000001
        bits[WRAP - 1] = INF_BITS
        bits[WRAP - 2] = 0x007fffff
        bits[WRAP] = 0x00800000                   # the layer of one element
        bits[WRAP + 1 + 6] = FLT_MAX_BITS
        bits[WRAP + 1 + 7 + 7] = INF_BITS
        bits[n - 1] = INF_BITS
        assert int((bits == INF_BITS).sum()) == 3
        yield Case(f"fullrange-k{k}", _acc_layers(bits, FULL_SIZES), 2, 1, [(k, None)])


def _signed_values():
    rng = np.random.default_rng(4)
    bits = rng.integers(0, 1 << 32, 2976, dtype=np.uint64).astype(np.uint32)
    bits = bits[(bits & 0x7f800000) != 0x7f800000]          # finite
    bits = bits[(bits & 0x7fffffff) != 0][:2900]
    assert bits.size == 2900
    planted = np.array([0x80000000] * 5 + [0] * 5 + [0x00000001, 0x80000001, FLT_MAX_BITS,
                                                      0x80000000 | FLT_MAX_BITS], np.uint32)
    bits = np.concatenate([bits, planted])
    return f32_from_bits(bits[rng.permutation(bits.size)])


SIGNED_SIZES = (1, 1000, 9, 1904)


def _signed():
    vals = _signed_values()
    for dt in DTS:
        w = encode(vals, dt)
        v = decode(w, dt)
        nneg, nzero = int((v < 0).sum()), int((v == 0).sum())
        assert nneg > 100 and nzero >= 10 and nneg + nzero < v.size - 100
        sign = SIGN[dt]
        assert ((w == sign).sum() >= 5) and ((w == 0).sum() >= 5)

        def layers():
            return [Layer(dt, part) for part in _split(w, SIGNED_SIZES)]

        at_zero = nneg + nzero
        for tag, k, pruned in (("min", 1, None), ("neg", nneg // 2, None), ("lastneg", nneg, nneg),
                               ("zero0", nneg + 1, at_zero), ("zero1", at_zero, at_zero),
                               ("pos0", at_zero + 1, None), ("max", v.size, v.size)):
            yield Case(f"signed-{dt}-{tag}", layers(), 3, 1, [(k, None)], pruned=[pruned])
        # chained: the entries round 1 masks score +0 in round 2 and lie ABOVE its negative
        # threshold, so `score > thr` keeps them (their mask returns to 1 over a weight of -0)
        yield Case(f"signed-{dt}-chained", layers(), 3, 1, [(nneg // 2, None), (nneg // 4, None)])
        yield Case(f"signed-{dt}-chained-up", layers(), 3, 1, [(nneg // 2, None), (at_zero + 50, None)])


MIXED_SIZES = (1, 7, 9, 2049, WRAP)


def _mixed():
    for mode in (0, 1):
        rng = np.random.default_rng(5)
        layers, steps = [], [[], [], []]
        for n in MIXED_SIZES:
            for dt in DTS:
                layers.append(Layer(dt, encode(rng.standard_normal(n).astype(np.float32), dt),
                                    np.zeros(n, np.float32)))
                for s in range(3):
                    mag = np.exp2(rng.uniform(-20, 10, n)) * rng.uniform(1, 2, n)
                    g = (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
                    steps[s].append(encode(g, dt))
        f16_grads = np.concatenate([g for s in steps for l, g in zip(layers, s) if l.dt == "f16"])
        assert int((((f16_grads & 0x7c00) == 0) & ((f16_grads & 0x3ff) != 0)).sum()) > 100   # denormals
        total = sum(l.n for l in layers)
        yield Case(f"mixed-mode{mode}", layers, mode, 3, [(int(0.3 * total), None), (int(0.6 * total), None)],
                   grad_steps=steps)


def _overflow():
    """fp16 gradients that overflowed: acc = inf, and 0 * inf = NaN for a weight of zero.  The
    sort ranks every NaN above +inf, so the kernel's integer key has to as well (it does for a
    NaN with a clear sign bit); `NaN > thr` is false, so a NaN score is removed at every k."""
    sizes = (9, 1500, 500)
    n = sum(sizes)
    for tag, k in (("below", n // 2), ("lastfinite", n - 7), ("inf0", n - 6), ("inf1", n - 3),
                   ("nan0", n - 2), ("nan1", n)):
        rng = np.random.default_rng(6)
        w = rng.standard_normal(n).astype(np.float32)
        w[np.abs(w) < 1e-3] = 0.5
        acc = (np.abs(rng.standard_normal(n)) * 1000).astype(np.float32)
        w[[2, 700, 1999]] = 0.0                    # 0 * inf: NaN
        w[[5, 1777]] = 0.0                         # 0 * finite: 0
        acc[[2, 700, 1999, 0, 8, 1234, 2008]] = np.inf
        layers = [Layer("f16", encode(wp, "f16"), ap) for wp, ap in zip(_split(w, sizes), _split(acc, sizes))]
        sc = np.concatenate([scores(l, 0, 3) for l in layers])
        assert int(np.isnan(sc).sum()) == 3 and int(np.isinf(sc).sum()) == 4
        yield Case(f"overflow-{tag}", layers, 0, 3, [(k, None)])


PROT_SIZES = (1500, 1203, 509)
PROT_COUNTS = (0, 1203 // 4, 509)


def _prot_layers(kind):
    rng = np.random.default_rng(7)
    n = sum(PROT_SIZES)
    bits = (0x3f000000 + 5 * rng.permutation(n)).astype(np.uint32)       # distinct, positive
    a, b, c = _split(bits, PROT_SIZES)
    mask_b = np.ones(b.size, np.uint8)
    if kind == "masked":          # 100 scores survive the mask: the 300th largest is 0
        mask_b[rng.permutation(b.size)[100:]] = 0
    if kind == "ties":            # the 300th largest sits inside a run of 40 equal scores
        order = np.argsort(b)
        b[order[b.size - 320:b.size - 280]] = b[order[b.size - 300]]
    if kind == "fltmax":
        a[77] = FLT_MAX_BITS
    layers = _acc_layers(np.concatenate([a, b, c]), PROT_SIZES)
    layers[1].mask = mask_b
    return layers


def _prot_signed_layers(dt):
    """400 free weights | 200 negative, 110 scores of zero, 190 positive | 9, all protected."""
    rng = np.random.default_rng(11)

    def away_from_zero(n):
        x = rng.standard_normal(n).astype(np.float32)
        return x + np.copysign(np.float32(0.01), x)

    neg, pos, masked = -np.abs(away_from_zero(200)), np.abs(away_from_zero(190)), away_from_zero(100)
    assert 30 < int((masked < 0).sum()) < 70
    zeros = np.array([-0.0] * 5 + [0.0] * 5, np.float32)
    order = rng.permutation(500)
    vals = np.concatenate([neg, pos, zeros, masked])[order]
    mask = np.concatenate([np.ones(400, np.uint8), np.zeros(100, np.uint8)])[order]
    return [Layer(dt, encode(away_from_zero(400), dt)), Layer(dt, encode(vals, dt), None, mask),
            Layer(dt, encode(away_from_zero(9), dt))]


def _protection():
    free = PROT_SIZES[0] + PROT_SIZES[1] - PROT_COUNTS[1]            # unprotected, no ties: 2403
    n = sum(PROT_SIZES)
    P = PROT_COUNTS
    yield Case("protect-below", _prot_layers(""), 2, 1, [(700, P)], pruned=[700])
    yield Case("protect-all-free", _prot_layers(""), 2, 1, [(free, P)], pruned=[free])
    yield Case("protect-above", _prot_layers(""), 2, 1, [(free + 1, P)], pruned=[n])
    yield Case("protect-total", _prot_layers(""), 2, 1, [(n, P)], pruned=[n])
    # all of the masked layer is protected (score >= 0): only layer 0 is free
    yield Case("protect-masked-below", _prot_layers("masked"), 2, 1, [(PROT_SIZES[0], P)], pruned=[PROT_SIZES[0]])
    yield Case("protect-masked-above", _prot_layers("masked"), 2, 1, [(PROT_SIZES[0] + 1, P)], pruned=[n])
    # 320 scores of layer 1 are >= its threshold: 883 + 1500 are free
    yield Case("protect-ties-below", _prot_layers("ties"), 2, 1, [(free - 20, P)], pruned=[free - 20])
    yield Case("protect-ties-above", _prot_layers("ties"), 2, 1, [(free - 19, P)], pruned=[n])
    # a real FLT_MAX in the unprotected layer ranks among the protected scores
    yield Case("protect-fltmax-below", _prot_layers("fltmax"), 2, 1, [(free - 1, P)], pruned=[free - 1])
    yield Case("protect-fltmax-at", _prot_layers("fltmax"), 2, 1, [(free, P)], pruned=[n])
    # mode 3, a per-layer threshold of zero among scores of -0 (masked negative weights, -0
    # weights) and +0: all of them are >= it and protected, whichever zero the rank lands on
    for dt in ("f32", "bf16"):
        for tag, k, pruned in (("below", 600, 600), ("above", 601, 909)):
            yield Case(f"protect-signed-zeros-{dt}-{tag}", _prot_signed_layers(dt), 3, 1,
                       [(k, (0, 210, 9))], pruned=[pruned])
    # modes that form the score from the weight, two dtypes, a chained plain round (workspace reuse)
    for mode in (0, 3):
        rng = np.random.default_rng(8)
        layers = [Layer(dt, encode(rng.standard_normal(s).astype(np.float32), dt),
                        np.abs(rng.standard_normal(s)).astype(np.float32))
                  for dt, s in zip(("f16", "f32", "bf16"), PROT_SIZES)]
        yield Case(f"protect-then-plain-mode{mode}", layers, mode, 2, [(900, P), (1800, None)])


def alignment_cases():
    """One layer each; the GPU test runs every case aligned and through offset views."""
    for dt in DTS:
        for n in (9, 2049):
            for mode in (0, 3):
                rng = np.random.default_rng(n + mode)
                layer = Layer(dt, encode(rng.standard_normal(n).astype(np.float32), dt),
                              np.abs(rng.standard_normal(n)).astype(np.float32),
                              (rng.uniform(size=n) < 0.8).astype(np.uint8))
                yield Case(f"align-{dt}-n{n}-mode{mode}", [layer], mode, 2, [(n // 2, None)])


# element offsets of (w, acc, mask) inside their buffers: each alone, then all together
OFFSETS = {"aligned": (0, 0, 0), "w": (1, 0, 0), "acc": (0, 1, 0), "mask": (0, 0, 3), "all": (1, 1, 3)}


_BUILDERS = (_consecutive, _runs, _degenerate, _full_range, _signed, _mixed, _overflow, _protection)
_CACHE = {}


def prune_cases():
    """id -> Case, every selection case above (built once; take .clone() before running one)."""
    if not _CACHE:
        for build in _BUILDERS:
            for c in build():
                assert c.name not in _CACHE
                _CACHE[c.name] = c
    return _CACHE


def grad_accum_rows():
    """rows of one accumulate table: (dt, acc fp32, gradient bits, acc offset, gradient offset)."""
    rng = np.random.default_rng(9)
    # -0, denormals, +-inf, then 1 (onto 2^24: stays) and 2^-24 (onto 1: a tie, rounds to even)
    special = {"f32": [0x80000000, 0x00000001, 0x807fffff, INF_BITS, 0xff800000, 0x3f800000, 0x33800000],
               "f16": [0x8000, 0x0001, 0x83ff, 0x7c00, 0xfc00, 0x3c00, 0x0001],
               "bf16": [0x8000, 0x0001, 0x807f, 0x7f80, 0xff80, 0x3f80, 0x3380]}
    rows = []
    for i, (n, dt) in enumerate([(1, "bf16"), (7, "f16"), (8, "f32"), (9, "bf16"), (9, "f16"),
                                 (ACCUM_WRAP, "f16"), (2049, "f32"), (2049, "bf16")]):
        g = encode((rng.standard_normal(n) * np.exp2(rng.uniform(-30, 12, n))).astype(np.float32), dt)
        acc = np.abs(rng.standard_normal(n)).astype(np.float32)
        sp = np.array(special[dt], UINT[dt])
        if n >= 7:
            g[:7] = sp
            g[-7:] = sp[::-1]
            acc[:7] = np.array([0.0, 0.0, 1.0, 3.0, np.inf, 16777216.0, 1.0], np.float32)
        else:
            g[0] = sp[0]                            # -0 onto +0
            acc[0] = 0.0
        rows.append((dt, acc, g, 1 if i == 6 else 0, 1 if i == 4 else 0))
    return rows


def count_zero_rows():
    """rows of one zero-count table: (dt, bits, offset); the expectation is count_zeros()."""
    rng = np.random.default_rng(10)
    special = {"f32": [0x80000000, 0, 0x00000001, 0x80000001, 0x007fffff, 0x7fc00000, 0xffc00000],
               "f16": [0x8000, 0, 0x0001, 0x8001, 0x03ff, 0x7e00, 0xfe00],
               "bf16": [0x8000, 0, 0x0001, 0x8001, 0x007f, 0x7fc0, 0xffc0]}
    rows = []
    for dt in DTS:
        sp = np.array(special[dt], UINT[dt])
        one = encode(np.array([1.0], np.float32), dt)[0]
        rows.append((dt, sp.copy(), 0))                                      # 7: only two count
        rows.append((dt, np.array([SIGN[dt]], UINT[dt]), 0))                 # 1: -0
        rows.append((dt, np.full(9, one, UINT[dt]), 0))                      # no zero
        z = np.zeros(9, UINT[dt])
        z[1::2] = SIGN[dt]
        rows.append((dt, z, 1 if dt == "f16" else 0))                        # all zero, both signs
        big = encode(rng.standard_normal(WRAP).astype(np.float32), dt)
        big[rng.permutation(WRAP)[:5000]] = 0
        big[rng.permutation(WRAP)[:5000]] = SIGN[dt]
        big[[0, 64 * 256 * 8 + 3, WRAP - 1]] = [0, SIGN[dt], 0]              # first group, second sweep, tail
        big[[1, 64 * 256 * 8 + 4, WRAP - 2]] = sp[[2, 5, 3]]                 # denormal, NaN, -denormal
        rows.append((dt, big, 1 if dt == "bf16" else 0))
    return rows
