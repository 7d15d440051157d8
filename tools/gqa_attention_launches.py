#!/usr/bin/env python3
"""Grouped-query causal rotary attention at the shapes of Llama-3-8B / Mistral-7B (32 query heads on
8 key / value heads) and Llama-2-70B / Llama-3-70B (64 on 8), batch 1, 2048 and 512 tokens, fp16:
four forms on the same random data, in one process, warm, alternating, device events around each of
25 repetitions (a repetition is `--inner` launches back to back, 10 by default; the time is per
launch):

    expanded   `ecoflap_causal_attention` on K / V expanded to all heads, the expanding copy
               (`repeat_interleave` of k and of v) inside the timed region: what grouped-query
               attention costs with the kernel as it was
    torch      rotate q and k, `repeat_kv`, `F.scaled_dot_product_attention(is_causal=True)`, the merge
    P1         `ecoflap_causal_attention_gqa`, one head per workgroup (k / v read in place)
    P2, P4, P8 the same entry with 2, 4, 8 heads of a KV group per workgroup (those that divide G)

Per form: median, min and max - min over the repetitions, in microseconds.  Per group size G the
tool then applies the rule for `heads_per_workgroup == 0`: a P > 1 may be the default
for a G only where its median is below P1's median by more than P1's own max - min, at both token
counts.  All forms of the entry are checked to give the same bits before anything is timed.  One JSON
line."""
import argparse
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
SCALE = D ** -0.5


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def forms(H, KVH, T):
    G = H // KVH
    q = torch.randn(1, T, H * D, device="cuda").half()
    k, v = (torch.randn(1, T, KVH * D, device="cuda").half() for _ in range(2))
    cos, sin = L.rotary_table(T, D, 10000.0, torch.device("cuda"))
    cos16 = torch.cat((cos, cos), -1).half()[None, None]
    sin16 = torch.cat((sin, sin), -1).half()[None, None]

    def expanded():
        ke = k.view(1, T, KVH, D).repeat_interleave(G, dim=2).view(1, T, H * D)
        ve = v.view(1, T, KVH, D).repeat_interleave(G, dim=2).view(1, T, H * D)
        return fused.causal_attention(q, ke, ve, H, SCALE, rope=(cos, sin))

    def torch_path():
        qh = q.view(1, T, H, D).transpose(1, 2)
        kh, vh = (t.view(1, T, KVH, D).transpose(1, 2) for t in (k, v))
        qh = (qh * cos16) + (L.rotate_half(qh) * sin16)
        kh = (kh * cos16) + (L.rotate_half(kh) * sin16)
        kh, vh = (t[:, :, None].expand(1, KVH, G, T, D).reshape(1, H, T, D) for t in (kh, vh))
        o = F.scaled_dot_product_attention(qh, kh, vh, is_causal=True, scale=SCALE)
        return o.transpose(1, 2).reshape(1, T, H * D)

    def entry(P):
        return lambda: fused.causal_attention(q, k, v, H, SCALE, rope=(cos, sin), kv_heads=KVH,
                                              heads_per_workgroup=P)

    out = {"expanded": expanded, "torch": torch_path}
    for P in (1, 2, 4, 8):
        if G % P == 0:
            out[f"P{P}"] = entry(P)
    return out


def measure(H, KVH, T, reps, inner):
    fs = forms(H, KVH, T)
    with torch.no_grad():
        want = fs["expanded"]()
        assert want is not None
        for name, fn in fs.items():
            if name.startswith("P"):
                got = fn()
                assert got is not None and torch.equal(got, want), name     # the schedule alone differs
        err = (want.float() - fs["torch"]().float()).abs().max().item()
        for _ in range(3):
            for fn in fs.values():
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in fs}
        for _ in range(reps):                       # alternating: one repetition of every form per round
            for name, fn in fs.items():
                times[name].append(timed(fn, inner))
    row = {"heads": H, "kv_heads": KVH, "group": H // KVH, "tokens": T, "batch": 1,
           "max_abs_diff_vs_torch": round(err, 5), "forms": {}}
    for name, ts in times.items():
        row["forms"][name] = {"median_us": round(statistics.median(ts), 1), "min_us": round(min(ts), 1),
                              "spread_us": round(max(ts) - min(ts), 1)}
    return row


def decide(rows):
    """Per group size: of the P whose median beats P1's by more than P1's max - min at every
    token count measured, the one with the smallest medians, else 1; and whether the entry (at that P) beats `expanded` the same way."""
    out = {}
    for G in sorted({r["group"] for r in rows}):
        mine = [r for r in rows if r["group"] == G]
        passing = [P for P in (2, 4, 8)
                   if all(f"P{P}" in r["forms"] and r["forms"][f"P{P}"]["median_us"]
                          < r["forms"]["P1"]["median_us"] - r["forms"]["P1"]["spread_us"] for r in mine)]
        best = min(passing, key=lambda P: sum(r["forms"][f"P{P}"]["median_us"] for r in mine)) if passing else 1
        faster = all(r["forms"][f"P{best}"]["median_us"]
                     < r["forms"]["expanded"]["median_us"] - r["forms"]["expanded"]["spread_us"] for r in mine)
        out[str(G)] = {"default_heads_per_workgroup_by_the_rule": best,
                       "faster_than_expanded_beyond_its_spread": bool(faster)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--tokens", type=int, nargs="+", default=[2048, 512])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here is measured on a CPU"
    rows = [measure(H, KVH, T, args.reps, args.inner) for H, KVH in ((32, 8), (64, 8)) for T in args.tokens]
    print(json.dumps({"reps": args.reps, "launches_per_rep": args.inner, "rows": rows, "rule": decide(rows)}))


if __name__ == "__main__":
    main()
