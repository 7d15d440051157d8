#!/usr/bin/env python3
"""Time the SparseGPT column sweep of one matrix two ways: through the one-call form
(`ecoflap_sparsegpt_matrix`: widen, every block step, every trailing update, round back, queued by
one host call) and through the per-step form `SparseGPT.fasterprune` drives from Python (per 128
columns: a torch allocation, `ecoflap_sparsegpt_block`, a library GEMM and a subtraction; torch's
`.clone().float()` before and `.to(dtype)` after).  Per shape: the median of the timed calls, device
time by events and host wall time (call to return of the last enqueue, then to the end of a
synchronize), for both forms.

    python tools/sgpt_sweep_launches.py [--calls 30] [--warmup 5] [--shapes clip | ROWSxCOLS ...]

-> one JSON line per shape.  `clip`: the four ViT-B/16 shapes of the visual tower and the four of
the text tower."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CLIP_SHAPES = [(2304, 768), (768, 768), (3072, 768), (768, 3072),       # visual: in_proj, out_proj, c_fc, c_proj
               (1536, 512), (512, 512), (2048, 512), (512, 2048)]       # text


def inverse_factor(cols, g):
    mix = 0.3 * torch.randn(cols, cols, generator=g) / cols ** 0.5 + torch.eye(cols)
    x = torch.randn(2 * cols + 64, cols, generator=g) @ mix
    H = (x.t() @ x * (2.0 / x.shape[0])).double()
    return torch.linalg.cholesky(torch.linalg.inv(H), upper=True).float().contiguous().cuda()


def per_step(kern, w, Hinv, sparsity, blocksize=128):
    """The sweep as `fasterprune` runs it with `whole_matrix_sweep` off."""
    rows, cols = w.shape
    W = w.clone().float()
    for i1 in range(0, cols, blocksize):
        i2 = min(i1 + blocksize, cols)
        err = torch.empty((rows, i2 - i1), dtype=torch.float32, device=W.device)
        kern.sparsegpt_block(W, Hinv, i1, i2 - i1, int(rows * (i2 - i1) * sparsity), err)
        if i2 < cols:
            W[:, i2:] -= err.matmul(Hinv[i1:i2, i2:])
    w.copy_(W.to(w.dtype))


def one_call(kern, w, Hinv, sparsity, blocksize=128):
    rows, cols = w.shape
    ranks = [int(rows * (min(i1 + blocksize, cols) - i1) * sparsity) for i1 in range(0, cols, blocksize)]
    kern.sparsegpt_matrix(w, Hinv, None, blocksize, ranks)


def timed(fn, kern, w0, Hinv, sparsity, calls, warmup):
    dev, host, wall = [], [], []
    for i in range(warmup + calls):
        w = w0.clone()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn(kern, w, Hinv, sparsity)
        b.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= warmup:
            dev.append(a.elapsed_time(b) * 1e3)
            host.append((t1 - t0) * 1e6)
            wall.append((t2 - t0) * 1e6)
    return {"device_us": round(statistics.median(dev), 1), "host_enqueue_us": round(statistics.median(host), 1),
            "host_wall_us": round(statistics.median(wall), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sparsity", type=float, default=0.4)
    ap.add_argument("--dtype", default="float16")
    ap.add_argument("--shapes", nargs="*", default=["clip"])
    args = ap.parse_args()
    from ecoflap_amd import hip
    kern = hip.HipKernels()
    shapes = []
    for s in args.shapes:
        shapes += CLIP_SHAPES if s == "clip" else [tuple(int(v) for v in s.split("x"))]
    factors = {}
    for rows, cols in shapes:
        g = torch.Generator().manual_seed(rows + cols)
        if cols not in factors:
            factors[cols] = inverse_factor(cols, g)
        Hinv = factors[cols]
        w0 = (torch.randn(rows, cols, generator=g) * 0.05).to(getattr(torch, args.dtype)).cuda()
        # interleaved: both forms see the same clock and cache state
        res = {"rows": rows, "cols": cols, "dtype": args.dtype, "calls": args.calls}
        res["per_step"] = timed(per_step, kern, w0, Hinv, args.sparsity, args.calls, args.warmup)
        res["one_call"] = timed(one_call, kern, w0, Hinv, args.sparsity, args.calls, args.warmup)
        res["host_wall_ratio_one_call_over_per_step"] = round(
            res["one_call"]["host_wall_us"] / res["per_step"]["host_wall_us"], 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
