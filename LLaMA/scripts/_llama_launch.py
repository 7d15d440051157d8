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
MODEL = "huggyllama/llama-7b"       # --model of the two shell scripts

# --model (LLaMA/main.py:31, any hub name or path), by its basename in lower case ->
# (the harness's --llama_model, decoder layers, the name of the output folder)
MODELS = {"llama-7b": ("7b", LAYERS, "llama_7b"),
          "meta-llama-3-8b": ("3-8b", 32, "llama3_8b"), "llama-3-8b": ("3-8b", 32, "llama3_8b"),
          "llama-2-70b-hf": ("2-70b", 80, "llama2_70b"), "llama-2-70b": ("2-70b", 80, "llama2_70b")}


PRUNERS = {"wanda": "llama_wanda_pruner", "sparsegpt": "llama_sparsegpt_pruner"}     # LLaMA/main.py:36


def model_entry(model):
    """`--model` -> its entry of MODELS; an unknown basename is an error, not a guess."""
    base = os.path.basename(str(model).rstrip("/")).lower()
    if base not in MODELS:
        raise SystemExit(f"--model {model}: no shape for '{base}' (known: {', '.join(sorted(MODELS))})")
    return MODELS[base]


def harness_flags(tag, score_method, num_samples_for_first_stage, out_root="out", prune_method="wanda",
                  model=MODEL):
    """--approach_for_sparsity block --aggregate_method sum --score_method GradOnly [--use_mezo]
    -> `--sparsity_ratio_granularity block --score_method [MEZO-]GradOnly_sum`; --prune_method
    {wanda, sparsegpt} -> the registered pruner (outputs of a SparseGPT run carry `_sparsegpt`);
    --model -> the shape (`--llama_model`, absent for the default), the layer count of the prune
    spec and the output folder."""
    keep = round(1 - SPARSITY_RATIO, 6)
    if prune_method != "wanda":
        tag = f"{tag}_{prune_method}"
    key, layers, folder = model_entry(model)
    return ["--shape", "llama", "--pruning_method", PRUNERS[prune_method]] + \
           ([] if key == "7b" else ["--llama_model", key]) + [
            "--llama_prune_spec", f"{layers}-{keep}-1-1",
            "--sparsity_ratio_granularity", "block", "--score_method", score_method,
            "--max_sparsity_per_layer", str(MAX_SPARSITY_PER_LAYER),
            "--num_data", str(NSAMPLES), "--num_data_first_stage", str(num_samples_for_first_stage),
            "--seed", str(SEED), "--job_id", tag,
            "--out_dir", os.path.join(out_root, folder, "unstructured", f"{tag}{SPARSITY_RATIO}")]


def split_args(argv):
    """-> (prune_method, the other arguments, passed to the harness as they are)."""
    import argparse
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--prune_method", choices=sorted(PRUNERS), default="wanda")
    known, extra = p.parse_known_args(list(argv))
    return known.prune_method, extra


def split_model(argv):
    """-> (--model, the other arguments); `huggyllama/llama-7b` without the flag."""
    import argparse
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--model", type=str, default=MODEL)
    known, extra = p.parse_known_args(list(argv))
    return known.model, extra


def run(flags, extra=()):
    cmd = [sys.executable, "-m", "ecoflap_amd.harness"] + list(flags) + list(extra)
    print(" ".join(cmd), flush=True)
    return subprocess.call(cmd, cwd=ROOT)
