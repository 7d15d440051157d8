#!/usr/bin/env python3
"""Generate tests/golden/g21_clip_sparsegpt.npz by running the reference's OWN
`CLIPLayerSparseGPTPruner` (CoOp/trainers/pruners/sparsegpt_pruner.py, loaded with its sibling
files by path from a checkout of ylsung/ECoFLaP under a synthetic package name) on the build's
CLIP shape modules, on the CPU with one torch thread, from fixed seeds:

    ECOFLAP_REFERENCE_CHECKOUT=/path/to/ECoFLaP python tests/golden/make_golden_clip_sparsegpt.py

Models, batches, seeds, the closure and the hash helpers are `make_golden_clip_pruner.py`'s, and so
are the cases: `clip_toy(2, 2)` in fp32 and fp16 under granularity None / block / layer / model,
`clip_slice(1, 1)` in fp16 uniform and block.  Nothing of the reference's source is copied: the
fixture holds per case the returned sparsity table (keys + float64 values; empty when uniform), the
sha256 of every pruned matrix, the packed zero masks of the toy cases, and the sha256 of the
initial and the final state.

The reference's `fasterprune` ends in `torch.cuda.synchronize()` (:304), which a CPU-only torch
refuses: it is a no-op for the duration of the reference's run.  Should `transformers` not import
(`sparsegpt_pruner.py` wants its `Conv1D` for an isinstance test), a stub module carrying an empty
`Conv1D` class stands in."""
import importlib
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_clip_pruner as G  # noqa: E402

CASES = G.CASES
case_key = G.case_key


def load_reference_sparsegpt(ref_root):
    try:
        import transformers  # noqa: F401
    except Exception:
        stub = types.ModuleType("transformers")
        stub.Conv1D = type("Conv1D", (torch.nn.Module,), {})
        sys.modules["transformers"] = stub
    folder = os.path.join(ref_root, "CoOp", "trainers", "pruners")
    pkg = types.ModuleType("reference_coop_pruners")
    pkg.__path__ = [folder]
    sys.modules["reference_coop_pruners"] = pkg
    return importlib.import_module("reference_coop_pruners.sparsegpt_pruner")


def main():
    R = load_reference_sparsegpt(os.environ["ECOFLAP_REFERENCE_CHECKOUT"])
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    real_sync = torch.cuda.synchronize
    torch.cuda.synchronize = lambda *a, **k: None
    out = {"seed": np.int64(G.SEED)}
    try:
        for name, granularity in CASES:
            model = G.build_model(name)
            key = case_key(name, granularity)
            out[key + "_state_sha256"] = np.array(G.state_sha256(model.state_dict()))
            loader, prompts = G.batches(name)
            G.seed_run()
            pruner = R.CLIPLayerSparseGPTPruner(model=model, data_loader=loader,
                                                **G.pruner_config(name, granularity))
            pruner.forward_to_cache = G.closure(prompts)
            model, table = pruner.prune()
            assert (table is None) == (granularity is None)
            table = table or {}
            out[key + "_table_keys"] = np.array(list(table.keys()), dtype=str)
            out[key + "_table_values"] = np.array([float(v) for v in table.values()], dtype=np.float64)
            mats = G.prunable(model)
            out[key + "_matrix_names"] = np.array([n for n, _ in mats], dtype=str)
            out[key + "_matrix_sha256"] = np.array([G.tensor_sha256(p.data) for _, p in mats], dtype=str)
            if name.startswith("toy"):
                for n, p in mats:
                    out[f"{key}_mask_{n}"] = np.packbits((p.data == 0).numpy().reshape(-1))
            out[key + "_final_state_sha256"] = np.array(G.state_sha256(model.state_dict()))
            sp = [float((p.data == 0).float().mean()) for _, p in mats]
            print(key, len(table), "table entries, matrix sparsity", round(min(sp), 4), "to", round(max(sp), 4),
                  flush=True)
    finally:
        torch.cuda.synchronize = real_sync
        torch.set_num_threads(threads)
    np.savez_compressed(os.path.join(HERE, "g21_clip_sparsegpt.npz"), **out)


if __name__ == "__main__":
    main()
