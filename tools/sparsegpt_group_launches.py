#!/usr/bin/env python3
"""Time the SparseGPT column sweeps of a twin set (Linears that share one Hinv) two ways in one
process: side by side through `ecoflap_sparsegpt_matrix_group` (one host call; per column block
the launches of one matrix) and one by one through `ecoflap_sparsegpt_matrix` (one host call per
member).  Warm, the two forms alternating, device time by events around every repetition and host
time from the call to the return of the last enqueue; per form the median, the minimum and
max - min.  The two forms are also compared bit for bit.

    python tools/sparsegpt_group_launches.py [--reps 25] [--warmup 3] [--sets 3x4096x4096 2x11008x4096]

-> one JSON line per set (MEMBERSxROWSxCOLS).  Defaults: q / k / v and gate / up of a LLaMA-7B
block, fp16, sparsity 0.6, Hinv from a seeded SPD matrix built on the device."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

BLOCK = 128


def inverse_factor(cols, seed):
    """Upper Cholesky factor of the inverse of a seeded SPD matrix, built on the device in fp64."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(2 * cols + 64, cols, generator=g, device="cuda", dtype=torch.float64)
    x = x + 0.3 * torch.roll(x, 1, dims=1)             # neighbouring columns correlated
    H = x.t() @ x * (2.0 / x.shape[0])
    return torch.linalg.cholesky(torch.linalg.inv(H), upper=True).float().contiguous()


def ranks_of(rows, cols, sparsity):
    return [int(rows * (min(i1 + BLOCK, cols) - i1) * sparsity) for i1 in range(0, cols, BLOCK)]


def one_by_one(kern, ws, Hinv, ranks):
    for w in ws:
        kern.sparsegpt_matrix(w, Hinv, None, BLOCK, ranks)


def grouped(kern, ws, Hinv, ranks):
    return kern.sparsegpt_matrix_group(ws, Hinv, None, BLOCK, [ranks] * len(ws))


def once(fn, kern, ws0, Hinv, ranks):
    ws = [w.clone() for w in ws0]
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn(kern, ws, Hinv, ranks)
    b.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3, (t1 - t0) * 1e6, ws


def summary(dev, host):
    return {"device_us_median": round(statistics.median(dev), 1), "device_us_min": round(min(dev), 1),
            "device_us_max_minus_min": round(max(dev) - min(dev), 1),
            "host_enqueue_us_median": round(statistics.median(host), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sparsity", type=float, default=0.6)
    ap.add_argument("--dtype", default="float16")
    ap.add_argument("--sets", nargs="*", default=["3x4096x4096", "2x11008x4096"])
    args = ap.parse_args()
    from ecoflap_amd import hip
    kern = hip.HipKernels()
    factors = {}
    for s in args.sets:
        members, rows, cols = (int(v) for v in s.split("x"))
        if cols not in factors:
            factors[cols] = inverse_factor(cols, cols)
        Hinv = factors[cols]
        g = torch.Generator().manual_seed(rows + cols)
        ws0 = [(torch.randn(rows, cols, generator=g) * 0.05).to(getattr(torch, args.dtype)).cuda()
               for _ in range(members)]
        ranks = ranks_of(rows, cols, args.sparsity)
        t = {"one_by_one": ([], []), "grouped": ([], [])}
        out = {}
        for i in range(args.warmup + args.reps):            # alternating: the same clocks and caches
            for name, fn in (("one_by_one", one_by_one), ("grouped", grouped)):
                dev, host, out[name] = once(fn, kern, ws0, Hinv, ranks)
                if i >= args.warmup:
                    t[name][0].append(dev)
                    t[name][1].append(host)
        view = torch.int32 if ws0[0].dtype == torch.float32 else torch.int16
        equal = all(torch.equal(a.view(view), b.view(view)) for a, b in zip(out["one_by_one"], out["grouped"]))
        res = {"members": members, "rows": rows, "cols": cols, "dtype": args.dtype, "sparsity": args.sparsity,
               "reps": args.reps, "column_blocks": len(ranks), "bit_for_bit": equal,
               "zero_fraction": round(float((out["grouped"][0] == 0).float().mean()), 4),
               "launches_grouped": grouped(kern, [w.clone() for w in ws0], Hinv, ranks),
               "one_by_one": summary(*t["one_by_one"]), "grouped": summary(*t["grouped"])}
        gain = res["one_by_one"]["device_us_median"] - res["grouped"]["device_us_median"]
        res["median_gain_us"] = round(gain, 1)
        res["gain_exceeds_one_by_one_spread"] = gain > res["one_by_one"]["device_us_max_minus_min"]
        torch.cuda.synchronize()
        print(json.dumps(res), flush=True)
        del ws0, out


if __name__ == "__main__":
    main()
