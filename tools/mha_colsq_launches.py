#!/usr/bin/env python3
"""`ecoflap_mha_attention_colsq` against what it replaces, at the CLIP towers' shapes (visual 197
tokens x 12 heads, text 77 tokens x 8 heads) and batch 16 (the reference's calibration batch) and
256: the fused call (with the output: the visual tower's case; without: the text tower's) and the
pair `fused.mha_attention(causal=False)` + `ecoflap_colsqnorm_accum` on its output, alternating in
one process.  Meant to run under `rocprofv3 --kernel-trace --stats -- python
tools/mha_colsq_launches.py` (the kernels' own durations are the profiler's); on its own it prints
device-event medians of 7 rounds of 20 launches and the share of the HBM bound (3 B N H D 2 bytes
read, + B N H D 2 written with the output; the pair reads the output again).  One JSON line."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("TENSILE_STREAMK_DATA_PARALLEL", "1")
from ecoflap_amd import hip  # noqa: E402
from ecoflap_amd.shapes import fused  # noqa: E402

D = 64


def timed(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    kernels = hip.HipKernels()
    rows = []
    for name, L, H in (("visual", 197, 12), ("text", 77, 8)):
        for B in (16, 256):
            qkv = (torch.randn(L, B, 3 * H * D, device="cuda") * 0.7).half()
            row = torch.zeros(H * D, device="cuda")

            def with_out():
                return fused.mha_attention_colsq(qkv, H, D ** -0.5, out=True, seq_first=True)

            def without_out():
                return fused.mha_attention_colsq(qkv, H, D ** -0.5, out=False, seq_first=True)

            def pair():
                y = fused.mha_attention(qkv, H, D ** -0.5, causal=False, seq_first=True)
                kernels.colsqnorm_accum(row, y.view(L * B, H * D), 0, B)
                return y

            with torch.no_grad():
                for _ in range(3):
                    with_out(), without_out(), pair()
                torch.cuda.synchronize()
                t = {"with_out": [], "without_out": [], "pair": []}
                for _ in range(7):
                    t["with_out"].append(timed(with_out))
                    t["without_out"].append(timed(without_out))
                    t["pair"].append(timed(pair))
            read, write = 3 * B * L * H * D * 2, B * L * H * D * 2
            med = {k: statistics.median(v) for k, v in t.items()}
            rows.append({"tower": name, "tokens": L, "heads": H, "batch": B,
                         **{k + "_us": round(v, 1) for k, v in med.items()},
                         **{k + "_spread_us": round(max(v) - min(v), 1) for k, v in t.items()},
                         "with_out_pct_of_hbm_bound": round(100 * (read + write) / 8e12 / (med["with_out"] * 1e-6), 1),
                         "without_out_pct_of_hbm_bound": round(100 * read / 8e12 / (med["without_out"] * 1e-6), 1),
                         "pair_pct_of_hbm_bound": round(100 * (read + 2 * write) / 8e12 / (med["pair"] * 1e-6), 1)})
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
