#!/usr/bin/env python3
"""Generate tests/golden/g20_clip_wanda.npz by running the reference's OWN `CLIPLayerWandaPruner`
(CoOp/trainers/pruners/wanda_pruner.py, its three sibling files loaded with it by path from a
checkout of ylsung/ECoFLaP, under a synthetic package name: `trainers/__init__.py` imports Dassl
and is never imported) on the build's CLIP shape modules, on the CPU, from fixed seeds:

    ECOFLAP_REFERENCE_CHECKOUT=/path/to/ECoFLaP python tests/golden/make_golden_clip_pruner.py

Nothing of the reference's source is copied: the fixture holds seeds, the sha256 of each initial
state, and per case the returned sparsity table (keys + float64 values; empty for the uniform
case, whose table is None), the sha256 of every pruned matrix and, for the toy cases, the packed
zero masks.

Cases: `clip_toy(2, 2)` in fp32 and as `half_weights` leaves it, 4 batches of 4, granularity None
(GradMagSquare_avg) / block / layer / model (MEZO-GradOnly_sum); `clip_slice(1, 1)` in fp16 at
ViT-B/16's true widths, 2 batches of 4, uniform and block."""
import hashlib
import importlib
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from ecoflap_amd.pruners.losses import clip_contrastive  # noqa: E402
from ecoflap_amd.shapes import clip as C  # noqa: E402

SEED = 20
SPEC = "1-0.6-1-1"
MAX_SPARSITY = 0.5
NUM_CLASSES = 10

# model -> (constructor, image size, context, vocabulary, batches, batch size)
MODELS = {
    "toy_fp32": (lambda: C.clip_toy(2, 2), 32, 6, 64, 4, 4),
    "toy_fp16": (lambda: C.clip_toy(2, 2, fp16=True), 32, 6, 64, 4, 4),
    "b16_fp16": (lambda: C.clip_slice(1, 1, fp16=True), 224, 77, 49408, 2, 4),
}
GRANULARITIES = {None: "GradMagSquare_avg", "block": "MEZO-GradOnly_sum", "layer": "MEZO-GradOnly_sum",
                 "model": "MEZO-GradOnly_sum"}
CASES = ([(m, g) for m in ("toy_fp32", "toy_fp16") for g in (None, "block", "layer", "model")]
         + [("b16_fp16", None), ("b16_fp16", "block")])


def case_key(model, granularity):
    return f"{model}_{granularity or 'uniform'}"


def state_sha256(state):
    h = hashlib.sha256()
    for k in sorted(state):
        h.update(k.encode())
        h.update(state[k].detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def tensor_sha256(t):
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def build_model(name):
    torch.manual_seed(SEED)
    return MODELS[name][0]().eval()


def batches(name, device="cpu"):
    """`{"img", "label"}` batches with distinct labels within a batch (a contrastive batch needs
    distinct prompts), and the tokenised prompt of every class."""
    _, image, context, vocab, n, bs = MODELS[name]
    g = torch.Generator().manual_seed(SEED + 1)
    prompts = torch.randint(1, vocab - 1, (NUM_CLASSES, context), generator=g)
    prompts[torch.arange(NUM_CLASSES), torch.randint(1, context, (NUM_CLASSES,), generator=g)] = vocab - 1
    out = [{"img": torch.randn(bs, 3, image, image, generator=g).to(device),
            "label": torch.randperm(NUM_CLASSES, generator=g)[:bs].to(device)} for _ in range(n)]
    return out, prompts


def pruner_config(name, granularity):
    _, _, _, _, n, bs = MODELS[name]
    return dict(language_prune_spec=SPEC, visual_prune_spec=SPEC, language_pruning_method="none",
                visual_pruning_method="none", num_samples=n * bs, num_data_first_stage=n * bs,
                sparsity_ratio_granularity=granularity, max_sparsity_per_layer=MAX_SPARSITY,
                score_method=GRANULARITIES[granularity])


def closure(prompts):
    """`forward_to_cache(model, batch, device)`.  The reference's first-order pass hands
    `device != "cpu"` instead of a device (layer_single_base_pruner.py:435): anything that is not
    a device means the model's own."""
    inner = clip_contrastive(prompts)

    def forward_to_cache(model, batch, device):
        if not isinstance(device, (torch.device, str)):
            device = next(iter(model.parameters())).device
        return inner(model, batch, device)
    return forward_to_cache


def seed_run():
    np.random.seed(42)
    torch.manual_seed(42)


def prunable(model):
    return [(n, p) for n, p in model.named_parameters() if p.dim() == 2 and ".resblocks" in n]


def load_reference_pruners(ref_root):
    folder = os.path.join(ref_root, "CoOp", "trainers", "pruners")
    pkg = types.ModuleType("reference_coop_pruners")
    pkg.__path__ = [folder]
    sys.modules["reference_coop_pruners"] = pkg
    return importlib.import_module("reference_coop_pruners.wanda_pruner")


def main():
    R = load_reference_pruners(os.environ["ECOFLAP_REFERENCE_CHECKOUT"])
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    out = {"seed": np.int64(SEED)}
    try:
        for name, granularity in CASES:
            model = build_model(name)
            key = case_key(name, granularity)
            out[key + "_state_sha256"] = np.array(state_sha256(model.state_dict()))
            loader, prompts = batches(name)
            seed_run()
            pruner = R.CLIPLayerWandaPruner(model=model, data_loader=loader, **pruner_config(name, granularity))
            pruner.forward_to_cache = closure(prompts)
            model, table = pruner.prune()
            assert (table is None) == (granularity is None)
            table = table or {}
            out[key + "_table_keys"] = np.array(list(table.keys()), dtype=str)
            out[key + "_table_values"] = np.array([float(v) for v in table.values()], dtype=np.float64)
            mats = prunable(model)
            out[key + "_matrix_names"] = np.array([n for n, _ in mats], dtype=str)
            out[key + "_matrix_sha256"] = np.array([tensor_sha256(p.data) for _, p in mats], dtype=str)
            if name.startswith("toy"):
                for n, p in mats:
                    out[f"{key}_mask_{n}"] = np.packbits((p.data == 0).numpy().reshape(-1))
            out[key + "_final_state_sha256"] = np.array(state_sha256(model.state_dict()))
            zeros = sum(int((p.data == 0).sum()) for _, p in mats)
            print(key, len(table), "table entries,", zeros, "zeros of", sum(p.numel() for _, p in mats))
    finally:
        torch.set_num_threads(threads)
    np.savez_compressed(os.path.join(HERE, "g20_clip_wanda.npz"), **out)


if __name__ == "__main__":
    main()
