#!/usr/bin/env python3
"""The LLaMA block's causal rotary attention at the reference's calibration shape (batch 1, 32
heads of 128, 2048 tokens) and at 512 tokens: `fused.causal_attention` (rotation, mask, softmax
and both products in one kernel, the projections' outputs read in place) against torch's path on
the same random data (`q * cos + rotate_half(q) * sin` for q and k, the head transposes a model
pays, `F.scaled_dot_product_attention(is_causal=True)`, the merge), alternating the two in one
process, device events, 7 rounds of 20 launches each: median and spread (max - min over the
rounds) per path, and the achieved MFMA rate against the causal flop count 2 * 2 * T^2 / 2 * 128
per head.

Then one `llama_7b` block (true width, fp16) at 2048 tokens: its fused forward against the same
block with the fused ops refused (the module's torch path), back to back on one device, median of
25 runs each after warm-up.  One JSON line."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("TENSILE_STREAMK_DATA_PARALLEL", "1")
from ecoflap_amd.shapes import fused  # noqa: E402
from ecoflap_amd.shapes import llama as L  # noqa: E402

D = 128
PEAK_F16_FLOPS = 2.5e15


def timed(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def attention_rows():
    rows = []
    for T in (2048, 512):
        B, H = 1, 32
        q, k, v = (torch.randn(B, T, H * D, device="cuda").half() for _ in range(3))
        cos, sin = L.rotary_table(T, D, 10000.0, torch.device("cuda"))
        cos16 = torch.cat((cos, cos), -1).half()[None, None]
        sin16 = torch.cat((sin, sin), -1).half()[None, None]

        def own():
            return fused.causal_attention(q, k, v, H, D ** -0.5, rope=(cos, sin))

        def lib():
            qh, kh, vh = (t.view(B, T, H, D).transpose(1, 2) for t in (q, k, v))
            qh = (qh * cos16) + (L.rotate_half(qh) * sin16)
            kh = (kh * cos16) + (L.rotate_half(kh) * sin16)
            o = F.scaled_dot_product_attention(qh, kh, vh, is_causal=True, scale=D ** -0.5)
            return o.transpose(1, 2).reshape(B, T, H * D)

        with torch.no_grad():
            assert own() is not None
            err = (own().float() - lib().float()).abs().max().item()
            for _ in range(3):
                own(), lib()
            torch.cuda.synchronize()
            t_own, t_lib = [], []
            for _ in range(7):
                t_own.append(timed(own))
                t_lib.append(timed(lib))
        flops = B * H * 2.0 * 2.0 * T * T / 2.0 * D
        m_own, m_lib = statistics.median(t_own), statistics.median(t_lib)
        rows.append({"tokens": T, "heads": H, "batch": B, "max_abs_diff_vs_torch": round(err, 5),
                     "own_us": round(m_own, 1), "own_spread_us": round(max(t_own) - min(t_own), 1),
                     "torch_us": round(m_lib, 1), "torch_spread_us": round(max(t_lib) - min(t_lib), 1),
                     "own_tflops": round(flops / m_own / 1e6, 1),
                     "own_pct_of_mfma_peak": round(100 * flops / PEAK_F16_FLOPS / (m_own * 1e-6), 1),
                     "own_faster_beyond_spread": bool(
                         m_lib - m_own > max(max(t_own) - min(t_own), max(t_lib) - min(t_lib)))})
    return rows


def block_row(T=2048, runs=25):
    torch.manual_seed(0)
    cfg = L.llama_config(4096, 32, 11008, 1, 32000)                 # llama_7b's block, without the embeddings
    blk = L.LlamaDecoderLayer(cfg, L._RopeCache(cfg.head_dim, cfg.rope_theta)).half().eval().cuda()
    x = torch.randn(1, T, 4096, device="cuda").half()
    refused = {}

    def fused_forward():
        return blk(x)

    def torch_forward():
        os.environ["ECOFLAP_NO_FUSED_ATTENTION"] = "1"
        try:
            for name in ("t5_rmsnorm", "t5_add_rmsnorm", "silu_mul", "linear"):
                refused[name] = getattr(fused, name)
                setattr(fused, name, lambda *a, **k: None)
            return blk(x)
        finally:
            for name, fn in refused.items():
                setattr(fused, name, fn)
            del os.environ["ECOFLAP_NO_FUSED_ATTENTION"]

    with torch.no_grad():
        for _ in range(3):
            a, b = fused_forward(), torch_forward()
        torch.cuda.synchronize()
        diff = (a.float() - b.float()).abs().max().item()
        t_f, t_t = [], []
        for _ in range(runs):
            t_f.append(timed(fused_forward, reps=1))
            t_t.append(timed(torch_forward, reps=1))
    return {"block": "llama_7b", "tokens": T, "runs": runs, "max_abs_diff_between_paths": round(diff, 5),
            "fused_us_median": round(statistics.median(t_f), 1), "fused_us_min": round(min(t_f), 1),
            "torch_us_median": round(statistics.median(t_t), 1), "torch_us_min": round(min(t_t), 1),
            "fused_not_slower": bool(statistics.median(t_f) <= statistics.median(t_t))}


def main():
    print(json.dumps({"attention": attention_rows(), "block": block_row()}))


if __name__ == "__main__":
    main()
