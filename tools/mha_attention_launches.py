#!/usr/bin/env python3
"""The CLIP towers' attention at the shapes stage 1 produces (visual 197 tokens x 12 heads, text
77 tokens x 8 heads causal, batch 16 * k for k in 1, 16, 32): `fused.mha_attention` against
torch's library attention (`F.scaled_dot_product_attention` on the same in-projection output, with
the head split / merge copies a model on it pays), alternating the two in one process, device
events, 7 rounds of 20 launches each: median and spread (max - min over the rounds) per path,
achieved FLOP/s from 4 B H N^2 D (half for causal) and bytes/s from 4 B N H D 2.  One JSON line."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("TENSILE_STREAMK_DATA_PARALLEL", "1")
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
    rows = []
    for name, L, H, causal in (("visual", 197, 12, False), ("text", 77, 8, True)):
        for k in (1, 16, 32):
            B = 16 * k
            qkv = (torch.randn(L, B, 3 * H * D, device="cuda") * 0.7).half()       # [L, N, 3D] as the blocks keep it

            def own():
                return fused.mha_attention(qkv, H, D ** -0.5, causal=causal, seq_first=True)

            def lib():
                q, k_, v = qkv.reshape(L, B, 3, H, D).permute(2, 1, 3, 0, 4)       # 3 x [B, H, L, D]
                o = F.scaled_dot_product_attention(q, k_, v, is_causal=causal, scale=D ** -0.5)
                return o.permute(2, 0, 1, 3).reshape(L, B, H * D)

            with torch.no_grad():
                assert own() is not None
                for _ in range(3):
                    own(), lib()
                torch.cuda.synchronize()
                t_own, t_lib = [], []
                for _ in range(7):
                    t_own.append(timed(own))
                    t_lib.append(timed(lib))
            flops = 4.0 * B * H * L * L * D * (0.5 if causal else 1.0)
            nbytes = 4 * B * L * H * D * 2
            m_own, m_lib = statistics.median(t_own), statistics.median(t_lib)
            t_flops, t_bytes = flops / 2.5e15, nbytes / 8e12
            rows.append({"tower": name, "tokens": L, "heads": H, "causal": causal, "batch": B,
                         "own_us": round(m_own, 1), "own_spread_us": round(max(t_own) - min(t_own), 1),
                         "library_us": round(m_lib, 1), "library_spread_us": round(max(t_lib) - min(t_lib), 1),
                         "own_tflops": round(flops / m_own / 1e6, 1), "own_gbs": round(nbytes / m_own / 1e3, 1),
                         "bound": "HBM" if t_bytes >= t_flops else "MFMA",
                         "own_pct_of_bound": round(100 * max(t_bytes, t_flops) / (m_own * 1e-6), 1),
                         "own_faster_beyond_spread": bool(
                             m_lib - m_own > max(max(t_own) - min(t_own), max(t_lib) - min(t_lib)))})
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
