"""Shared by the two LLaMA launchers: the values of the reference's shell scripts as harness flags."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# LLaMA/scripts/ecoflap_zero.sh, ecoflap_first.sh and the defaults of LLaMA/main.py:31-46
SPARSITY_RATIO = 0.6
MAX_SPARSITY_PER_LAYER = 0.7
NSAMPLES = 128                      # --nsamples
SEED = 0                            # --seed
LAYERS = 32                         # huggyllama/llama-7b


PRUNERS = {"wanda": "llama_wanda_pruner", "sparsegpt": "llama_sparsegpt_pruner"}     # LLaMA/main.py:36


def harness_flags(tag, score_method, num_samples_for_first_stage, out_root="out", prune_method="wanda"):
    """--approach_for_sparsity block --aggregate_method sum --score_method GradOnly [--use_mezo]
    -> `--sparsity_ratio_granularity block --score_method [MEZO-]GradOnly_sum`; --prune_method
    {wanda, sparsegpt} -> the registered pruner (outputs of a SparseGPT run carry `_sparsegpt`)."""
    keep = round(1 - SPARSITY_RATIO, 6)
    if prune_method != "wanda":
        tag = f"{tag}_{prune_method}"
    return ["--shape", "llama", "--pruning_method", PRUNERS[prune_method],
            "--llama_prune_spec", f"{LAYERS}-{keep}-1-1",
            "--sparsity_ratio_granularity", "block", "--score_method", score_method,
            "--max_sparsity_per_layer", str(MAX_SPARSITY_PER_LAYER),
            "--num_data", str(NSAMPLES), "--num_data_first_stage", str(num_samples_for_first_stage),
            "--seed", str(SEED), "--job_id", tag,
            "--out_dir", os.path.join(out_root, "llama_7b", "unstructured", f"{tag}{SPARSITY_RATIO}")]


def split_args(argv):
    """-> (prune_method, the other arguments, passed to the harness as they are)."""
    import argparse
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--prune_method", choices=sorted(PRUNERS), default="wanda")
    known, extra = p.parse_known_args(list(argv))
    return known.prune_method, extra


def run(flags, extra=()):
    cmd = [sys.executable, "-m", "ecoflap_amd.harness"] + list(flags) + list(extra)
    print(" ".join(cmd), flush=True)
    return subprocess.call(cmd, cwd=ROOT)
