#!/usr/bin/env python3
"""Generate tests/golden/g24_llama_sparsegpt.npz by running the reference's OWN classes on the
build's LLaMA shape module, on the CPU in fp32 with one thread, from fixed seeds:

    ECOFLAP_REFERENCE_CHECKOUT=/path/to/ECoFLaP python tests/golden/make_golden_llama_sparsegpt.py

The recipe of make_golden_llama_pruner.py (its adapter, its stage 1, its seeds) with stage 2 by the
reference's `T5LayerSparseGPTPruner._prune` (LAVIS/lavis/compression/pruners/sparsegpt_pruner.py:
349-407) and its own `SparseGPT` (:56-222).  That loop asserts `nsamples == len(inps)` (:390), a sample
count against a batch count, which holds for calibration batches of ONE sample only: 8 batches of
1 x 24 tokens.  With 192 tokens the 256-column Hessian of `o_proj` (2 heads of 128) is rank
deficient; the 64-column Hessians of q / k / v / gate / up and the 176-column one of `down_proj` are
not.

Nothing of the reference's source is copied: the fixture holds the seeds' results only — per case
the sparsity table (keys + float64 values), the sha256 of every pruned matrix, the packed zero
masks, and the sha256 of the final state.  Weights and batches are regenerated from seeds
(tests/llama_pruner_fixture.py).  The reference's `fasterprune` ends in `torch.cuda.synchronize()`
(:215), which a CPU-only torch refuses: it is a no-op for the duration of the reference's run.

Cases: zeroth order (MEZO-GradOnly_sum) at granularity block, first order (GradOnly_sum) at block,
and the uniform case (None)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from ecoflap_amd.pruners.losses import loss_causal_lm  # noqa: E402
from llama_pruner_fixture import batches, prunable_names, seeded_tiny, sha256  # noqa: E402
from make_golden_llama_pruner import (KEEP, MAX_SPARSITY, _Adapter, load_reference, mapping, seed_run,  # noqa: E402
                                      state_sha256)

N_BATCHES, BATCH_SIZE = 8, 1
# case -> (granularity, score method)
CASES = {"zeroth_block": ("block", "MEZO-GradOnly_sum"), "first_block": ("block", "GradOnly_sum"),
         "uniform": (None, "GradOnly_sum")}


def calibration(vocab):
    return batches(vocab=vocab, n=N_BATCHES, batch_size=BATCH_SIZE)


def pruner_config(case):
    granularity, method = CASES[case]
    return dict(prune_spec=f"2-{KEEP}-1-1", num_samples=N_BATCHES * BATCH_SIZE,
                num_data_first_stage=N_BATCHES * BATCH_SIZE, sparsity_ratio_granularity=granularity,
                max_sparsity_per_layer=MAX_SPARSITY, score_method=method, num_noise=1, noise_eps=1e-3)


def load_reference_sparsegpt(ref_root):
    """The reference's sparsegpt_pruner.py by path, on top of the stubs of `load_reference`."""
    ref = load_reference(ref_root)
    try:
        import transformers  # noqa: F401
    except Exception:           # (imported by the file, used by none of the code that runs here)
        sys.modules["transformers"] = types.ModuleType("transformers")
    name = "lavis.compression.pruners.sparsegpt_pruner"
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ref_root, "LAVIS/lavis/compression/pruners/sparsegpt_pruner.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    ref["sparsegpt_pruner"] = m
    return ref


def main():
    ref = load_reference_sparsegpt(os.environ["ECOFLAP_REFERENCE_CHECKOUT"])
    LayerSparsity = ref["layer_single_base_pruner"].LayerSparsity
    T5LayerSparseGPTPruner = ref["sparsegpt_pruner"].T5LayerSparseGPTPruner
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    real_sync = torch.cuda.synchronize
    torch.cuda.synchronize = lambda *a, **k: None
    out = {}
    try:
        for case, (granularity, method) in CASES.items():
            model = seeded_tiny()
            out[case + "_state_sha256"] = np.array(state_sha256(model.state_dict()))
            loader = calibration(model.config.vocab_size)
            cfg = pruner_config(case)
            for p in model.parameters():
                p.requires_grad = True
            seed_run()
            table = LayerSparsity(model, loader, loss_causal_lm, cfg["num_data_first_stage"], 1 - KEEP,
                                  cfg["max_sparsity_per_layer"], method, cfg["num_noise"], cfg["noise_eps"],
                                  mapping(model, granularity)).return_sparsity()
            names = prunable_names(model)
            out[case + "_table_keys"] = np.array(list(table.keys()) if granularity else [], dtype=str)
            out[case + "_table_values"] = np.array([float(table[k]) for k in table] if granularity else [],
                                                   dtype=np.float64)
            if granularity is None:
                assert all(float(table[k]) == 1 - KEEP for k in names)
            adapter = _Adapter(model)
            with_image = [dict(b, image=torch.zeros(len(b["input_ids"]), 1)) for b in loader]
            pruner = T5LayerSparseGPTPruner(model=adapter, data_loader=with_image, model_prefix="model", **cfg)
            pruner._prune(adapter, with_image, torch.device("cpu"), model_prefix="model",
                          module_to_process="model.layers", n_samples=cfg["num_samples"], sparsity_ratio=table)
            adapter.release()
            for p in model.parameters():
                p.requires_grad = False
            state = dict(model.named_parameters())
            out[case + "_matrix_names"] = np.array(names, dtype=str)
            out[case + "_matrix_sha256"] = np.array([sha256(state[n].data) for n in names], dtype=str)
            for n in names:
                out[f"{case}_mask_{n}"] = np.packbits((state[n].data == 0).numpy().reshape(-1))
            out[case + "_final_state_sha256"] = np.array(state_sha256(model.state_dict()))
            zeros = sum(int((state[n].data == 0).sum()) for n in names)
            print(case, len(out[case + "_table_keys"]), "table entries,", zeros, "zeros of",
                  sum(state[n].numel() for n in names))
    finally:
        torch.cuda.synchronize = real_sync
        torch.set_num_threads(threads)
    np.savez_compressed(os.path.join(HERE, "g24_llama_sparsegpt.npz"), **out)


if __name__ == "__main__":
    main()
