#!/usr/bin/env python3
"""Generate tests/golden/g26_llama_gqa_pruners.npz: the recipes of g23_llama_wanda.npz and
g24_llama_sparsegpt.npz (make_golden_llama_pruner.py, make_golden_llama_sparsegpt.py: their adapter,
their stage 1, their seeds, imported from those modules as they are) on the grouped-query toy decoder
of tests/llama_gqa_fixture.py, 4 query heads on 2 key / value heads, so that `k_proj` / `v_proj` have
half the rows of `q_proj`:

    ECOFLAP_REFERENCE_CHECKOUT=/path/to/ECoFLaP python tests/golden/make_golden_llama_gqa_pruners.py

Stage 1 is the reference's `LayerSparsity(...).return_sparsity()`, stage 2 its
`T5LayerWandaPruner._prune` or its `T5LayerSparseGPTPruner._prune`, on the CPU in fp32 with one
thread.  Nothing of the reference's source is copied: the fixture holds the seeds' results only — per
case the sparsity table (keys + float64 values), the sha256 of every pruned matrix, the packed zero
masks (`stored_masks`) and the sha256 of the final state.

Cases: `wanda_zeroth_block`, `wanda_uniform` (4 batches of 2 samples) and `sparsegpt_zeroth_block`
(8 batches of one sample, as that loop demands)."""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_golden_llama_pruner as W  # noqa: E402
import make_golden_llama_sparsegpt as S  # noqa: E402
from ecoflap_amd.pruners.losses import loss_causal_lm  # noqa: E402
from llama_gqa_fixture import CONFIG, TINY_KEYS  # noqa: E402
from llama_pruner_fixture import batches, prunable_names, seeded_tiny, sha256  # noqa: E402

# case -> (recipe module, its case name)
CASES = {"wanda_zeroth_block": (W, "zeroth_block"), "wanda_uniform": (W, "uniform"),
         "sparsegpt_zeroth_block": (S, "zeroth_block")}


# The packed zero masks of a case are ONE array, the matrices' `np.packbits` in `prunable_names` order
# one after the other.  The uniform Wanda masks differ from the zeroth-order ones in few places (the
# block ratios are 0.58 / 0.62 against 0.6) and are stored as their XOR with them: the file stays
# no larger than g24_llama_sparsegpt.npz although q_proj / o_proj are twice as large here.
MASKS_XOR = {"wanda_uniform": "wanda_zeroth_block"}


def packed_masks(state, names):
    return np.concatenate([np.packbits((state[n].data == 0).numpy().reshape(-1)) for n in names])


def stored_masks(golden, case):
    masks = golden[case + "_masks"]
    return masks ^ golden[MASKS_XOR[case] + "_masks"] if case in MASKS_XOR else masks


def gqa_tiny(dtype=torch.float32):
    return seeded_tiny(dtype=dtype, **{k: CONFIG[k] for k in TINY_KEYS})


def calibration(case, vocab):
    recipe = CASES[case][0]
    return batches(vocab=vocab) if recipe is W else S.calibration(vocab)


def pruner_config(case):
    recipe, name = CASES[case]
    return recipe.pruner_config(name)


def main():
    ref = S.load_reference_sparsegpt(os.environ["ECOFLAP_REFERENCE_CHECKOUT"])
    LayerSparsity = ref["layer_single_base_pruner"].LayerSparsity
    stage2 = {W: ref["wanda_pruner"].T5LayerWandaPruner, S: ref["sparsegpt_pruner"].T5LayerSparseGPTPruner}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    real_sync = torch.cuda.synchronize
    torch.cuda.synchronize = lambda *a, **k: None       # (the reference's fasterprune ends in one)
    out = {}
    try:
        for case, (recipe, name) in CASES.items():
            granularity, method = recipe.CASES[name]
            model = gqa_tiny()
            out[case + "_state_sha256"] = np.array(W.state_sha256(model.state_dict()))
            loader = calibration(case, model.config.vocab_size)
            cfg = pruner_config(case)
            for p in model.parameters():
                p.requires_grad = True
            W.seed_run()
            table = LayerSparsity(model, loader, loss_causal_lm, cfg["num_data_first_stage"], 1 - W.KEEP,
                                  cfg["max_sparsity_per_layer"], method, cfg["num_noise"], cfg["noise_eps"],
                                  W.mapping(model, granularity)).return_sparsity()
            names = prunable_names(model)
            out[case + "_table_keys"] = np.array(list(table.keys()) if granularity else [], dtype=str)
            out[case + "_table_values"] = np.array([float(table[k]) for k in table] if granularity else [],
                                                   dtype=np.float64)
            if granularity is None:
                assert all(float(table[k]) == 1 - W.KEEP for k in names)
            adapter = W._Adapter(model)
            with_image = [dict(b, image=torch.zeros(len(b["input_ids"]), 1)) for b in loader]
            pruner = stage2[recipe](model=adapter, data_loader=with_image, model_prefix="model", **cfg)
            pruner._prune(adapter, with_image, torch.device("cpu"), model_prefix="model",
                          module_to_process="model.layers", n_samples=cfg["num_samples"], sparsity_ratio=table)
            adapter.release()
            for p in model.parameters():
                p.requires_grad = False
            state = dict(model.named_parameters())
            out[case + "_matrix_names"] = np.array(names, dtype=str)
            out[case + "_matrix_sha256"] = np.array([sha256(state[n].data) for n in names], dtype=str)
            masks = packed_masks(state, names)
            out[case + "_masks"] = masks ^ out[MASKS_XOR[case] + "_masks"] if case in MASKS_XOR else masks
            out[case + "_final_state_sha256"] = np.array(W.state_sha256(model.state_dict()))
            zeros = sum(int((state[n].data == 0).sum()) for n in names)
            print(case, len(out[case + "_table_keys"]), "table entries,", zeros, "zeros of",
                  sum(state[n].numel() for n in names))
    finally:
        torch.cuda.synchronize = real_sync
        torch.set_num_threads(threads)
    np.savez_compressed(os.path.join(HERE, "g26_llama_gqa_pruners.npz"), **out)


if __name__ == "__main__":
    main()
