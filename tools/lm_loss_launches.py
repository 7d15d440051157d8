#!/usr/bin/env python3
"""The causal LM loss at LLaMA-7B's shape: `fused.causal_lm_loss` (csrc/lm_loss.hip: the shift inside
the kernel, every fp16 logit read once) against the torch chain the model ran before it
(`F.pad(labels)`, the shifted slice with `.contiguous()`, `logits.float()`, `F.cross_entropy`) on one
set of fp16 logits [2048, 32000] and [512, 32000], alternating the two in one process, device events,
warm-up, 25 rounds of 10 launches each: median and spread (max - min over the rounds) per path, and
the kernel's share of the 8 TB/s HBM peak for the bytes it has to read (rows x vocab x 2).  131 MB of
logits fit the 256 MiB Infinity Cache, so the same measurement is repeated rotating over five
buffers (655 MB), where every read comes from memory: `*_rotating_us`.

Then one `head` stage of `llama_7b` (final norm, lm_head, loss; the model's own weights shapes, no
decoder blocks) at 2048 tokens with the fused loss and with ECOFLAP_NO_FUSED_LOSS=1, median of 25.

    python tools/lm_loss_launches.py            # every step in a child of its own, under a time limit
    python tools/lm_loss_launches.py --step kernel | head

One JSON line per step."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TENSILE_STREAMK_DATA_PARALLEL", "1")

VOCAB = 32000
PEAK_HBM_BYTES = 8.0e12
STEPS = {"kernel": 240, "head": 240}       # step -> seconds allowed


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _stats(ts):
    return statistics.median(ts), max(ts) - min(ts)


def kernel_step(rounds=25, reps=10, buffers=5):
    import torch
    import torch.nn.functional as F
    from ecoflap_amd.shapes import fused
    rows_out = []
    for T in (2048, 512):
        g = torch.Generator(device="cuda").manual_seed(T)
        logits = [(4 * torch.randn(1, T, VOCAB, device="cuda", generator=g)).half() for _ in range(buffers)]
        labels = torch.randint(0, VOCAB, (1, T), device="cuda", generator=g)

        def own(i, rotate=False):
            return fused.causal_lm_loss(logits[i % buffers if rotate else 0], labels)

        def chain(i, rotate=False):
            x = logits[i % buffers if rotate else 0]
            shifted = F.pad(labels, (0, 1), value=-100)[..., 1:].contiguous()
            return F.cross_entropy(x.float().view(-1, VOCAB), shifted.view(-1), ignore_index=-100, reduction="mean")

        with torch.no_grad():
            a, b = own(0), chain(0)
            assert a is not None
            diff = abs(float(a) - float(b))
            for i in range(3 * buffers):
                own(i, True), chain(i, True)
            torch.cuda.synchronize()
            t = {"own": [], "chain": [], "own_rot": [], "chain_rot": []}
            for _ in range(rounds):
                t["own"].append(timed(own, reps))
                t["chain"].append(timed(chain, reps))
                t["own_rot"].append(timed(lambda i: own(i, True), reps))
                t["chain_rot"].append(timed(lambda i: chain(i, True), reps))
        (m_own, s_own), (m_chain, s_chain) = _stats(t["own"]), _stats(t["chain"])
        (m_own_r, s_own_r), (m_chain_r, s_chain_r) = _stats(t["own_rot"]), _stats(t["chain_rot"])
        bytes_needed = T * VOCAB * 2
        rows_out.append({
            "rows": T, "vocab": VOCAB, "rounds": rounds, "launches_per_round": reps,
            "loss_fused": float(a), "loss_chain": float(b), "abs_diff": diff,
            "own_us": round(m_own, 1), "own_spread_us": round(s_own, 1),
            "chain_us": round(m_chain, 1), "chain_spread_us": round(s_chain, 1),
            "own_rotating_us": round(m_own_r, 1), "own_rotating_spread_us": round(s_own_r, 1),
            "chain_rotating_us": round(m_chain_r, 1), "chain_rotating_spread_us": round(s_chain_r, 1),
            "bytes_needed": bytes_needed,
            "own_pct_of_8TBps": round(100 * bytes_needed / PEAK_HBM_BYTES / (m_own * 1e-6), 1),
            "own_rotating_pct_of_8TBps": round(100 * bytes_needed / PEAK_HBM_BYTES / (m_own_r * 1e-6), 1),
            "own_faster_beyond_spread": bool(m_chain - m_own > max(s_own, s_chain)),
            "own_rotating_faster_beyond_spread": bool(m_chain_r - m_own_r > max(s_own_r, s_chain_r))})
        del logits
        torch.cuda.empty_cache()
    return {"step": "kernel", "shapes": rows_out}


def head_step(T=2048, runs=25):
    import torch
    from ecoflap_amd.shapes import llama as L
    torch.manual_seed(0)
    cfg = L.llama_config(4096, 32, 11008, 0, VOCAB)          # llama_7b's embedding, norm and lm_head, no blocks
    with torch.device("cuda"):
        model = L._build(cfg, torch.float16, T).eval()
    head = model.stage_plan()[-1][2]
    state = {"x": torch.randn(1, T, 4096, device="cuda").half(),
             "labels": torch.randint(0, VOCAB, (1, T), device="cuda")}

    def fused_head(_):
        return head(state)["loss"]

    def chain_head(_):
        os.environ["ECOFLAP_NO_FUSED_LOSS"] = "1"
        try:
            return head(state)["loss"]
        finally:
            del os.environ["ECOFLAP_NO_FUSED_LOSS"]

    with torch.no_grad():
        for _ in range(3):
            a, b = fused_head(0), chain_head(0)
        torch.cuda.synchronize()
        t_f, t_c = [], []
        for _ in range(runs):
            t_f.append(timed(fused_head, 1))
            t_c.append(timed(chain_head, 1))
    (m_f, s_f), (m_c, s_c) = _stats(t_f), _stats(t_c)
    return {"step": "head", "stage": "llama_7b head", "tokens": T, "runs": runs,
            "loss_fused": float(a), "loss_chain": float(b),
            "fused_us_median": round(m_f, 1), "fused_us_min": round(min(t_f), 1), "fused_spread_us": round(s_f, 1),
            "chain_us_median": round(m_c, 1), "chain_us_min": round(min(t_c), 1), "chain_spread_us": round(s_c, 1),
            "fused_faster_beyond_spread": bool(m_c - m_f > max(s_f, s_c))}


def main(argv):
    if len(argv) == 2 and argv[0] == "--step":
        print(json.dumps({"kernel": kernel_step, "head": head_step}[argv[1]]()), flush=True)
        return 0
    # every GPU step in a fresh process under its own time limit; the first failure ends the run
    for step, seconds in STEPS.items():
        rc = subprocess.call(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__),
                              "--step", step], cwd=ROOT)
        if rc != 0:
            print(f"step {step} ended with status {rc}: nothing more is started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
