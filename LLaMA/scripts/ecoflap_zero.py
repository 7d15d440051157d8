"""ECoFLaP (zeroth order) + Wanda on LLaMA-7B (reference: LLaMA/scripts/ecoflap_zero.sh — `main.py
--model huggyllama/llama-7b --prune_method wanda --sparsity_ratio 0.6 --sparsity_type unstructured
--approach_for_sparsity block --aggregate_method sum --score_method GradOnly --max_sparsity_per_layer
0.7 --use_mezo --num_samples_for_first_stage 32`, 128 calibration samples of 2048 tokens, seed 0).
The model is the random-init decoder of that shape and the calibration ids are synthetic; the
perplexity evaluation behind the pruning is the model zoo's and is not reproduced.

    python LLaMA/scripts/ecoflap_zero.py [--prune_method {wanda,sparsegpt}] [--model NAME] [extra harness flags]

`--prune_method sparsegpt` (LLaMA/main.py:36) runs `llama_sparsegpt_pruner` on the same table and
writes under out/llama_7b/unstructured/ecoflap_zero_sparsegpt0.6/.

`--model` (LLaMA/main.py:31; by basename: `huggyllama/llama-7b`, `meta-llama/Meta-Llama-3-8B`,
`meta-llama/Llama-2-70b-hf`) picks the shape and the layer count of the prune spec; the last two are
grouped-query decoders and write under out/llama3_8b/ and out/llama2_70b/.

Outputs go under out/llama_7b/unstructured/ecoflap_zero0.6/ with --save_pruned_model."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _llama_launch import MODEL, harness_flags, run, split_args, split_model  # noqa: E402

NUM_SAMPLES_FOR_FIRST_STAGE = 32


def flags(prune_method="wanda", model=MODEL):
    return harness_flags("ecoflap_zero", "MEZO-GradOnly_sum", NUM_SAMPLES_FOR_FIRST_STAGE, prune_method=prune_method,
                         model=model)


if __name__ == "__main__":
    method, extra = split_args(sys.argv[1:])
    model, extra = split_model(extra)
    sys.exit(run(flags(method, model), extra))
