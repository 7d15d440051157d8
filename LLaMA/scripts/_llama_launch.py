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


def harness_flags(tag, score_method, num_samples_for_first_stage, out_root="out"):
    """--approach_for_sparsity block --aggregate_method sum --score_method GradOnly [--use_mezo]
    -> `--sparsity_ratio_granularity block --score_method [MEZO-]GradOnly_sum`."""
    keep = round(1 - SPARSITY_RATIO, 6)
    return ["--shape", "llama", "--pruning_method", "llama_wanda_pruner",
            "--llama_prune_spec", f"{LAYERS}-{keep}-1-1",
            "--sparsity_ratio_granularity", "block", "--score_method", score_method,
            "--max_sparsity_per_layer", str(MAX_SPARSITY_PER_LAYER),
            "--num_data", str(NSAMPLES), "--num_data_first_stage", str(num_samples_for_first_stage),
            "--seed", str(SEED), "--job_id", tag,
            "--out_dir", os.path.join(out_root, "llama_7b", "unstructured", f"{tag}{SPARSITY_RATIO}")]


def run(flags, extra=()):
    cmd = [sys.executable, "-m", "ecoflap_amd.harness"] + list(flags) + list(extra)
    print(" ".join(cmd), flush=True)
    return subprocess.call(cmd, cwd=ROOT)
