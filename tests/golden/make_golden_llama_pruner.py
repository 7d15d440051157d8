#!/usr/bin/env python3
"""Generate tests/golden/g23_llama_wanda.npz by running the reference's OWN classes on the build's
LLaMA shape module, on the CPU in fp32 with one thread, from fixed seeds:

    ECOFLAP_REFERENCE_CHECKOUT=/path/to/ECoFLaP python tests/golden/make_golden_llama_pruner.py

  stage 1   the reference's `LayerSparsity(...).return_sparsity()` (LAVIS/lavis/compression/pruners/
            layer_single_base_pruner.py) on `LlamaForCausalLM` itself, with the build's
            `loss_causal_lm` closure and a group per `model.layers.N` ("block") or per matrix ("layer");
  stage 2   the reference's `T5LayerWandaPruner._prune` (wanda_pruner.py:217-290 — the rows-mode loop,
            "the LLaMA loop" by its own comment at :233) over `model.layers`, on an adapter written
            here around the same model: its decoder layers accept and ignore the seven keyword
            arguments of a T5 block and return a tuple, its forward hands those seven keys to the
            first layer as None, it has a null `maybe_autocast`, `adapter.model.config.use_cache`,
            and its batches carry a dummy "image" of the batch length (the reference counts samples
            by it).  Parameter names stay LLaMA's.

The reference's LLaMA loops themselves (`LLaMA/lib/`) are not part of its tree.  Nothing of the
reference's source is copied: the fixture holds the seeds' results only — per case the sparsity
table (keys + float64 values), the sha256 of every pruned matrix, the packed zero masks, and the
sha256 of the final state (zeroth order: with the perturbation drift).  Weights and batches are
regenerated from seeds (tests/llama_pruner_fixture.py).

Cases: zeroth order (MEZO-GradOnly_sum) at granularity block and layer, first order (GradOnly_sum)
at block, and the uniform case (None)."""
import contextlib
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from ecoflap_amd.pruners.losses import loss_causal_lm  # noqa: E402
from ecoflap_amd.shapes.llama import LlamaDecoderLayer  # noqa: E402
from llama_pruner_fixture import N_BATCHES, BATCH_SIZE, batches, prunable_names, seeded_tiny, sha256  # noqa: E402

KEEP = 0.4                  # the launchers' --sparsity_ratio 0.6
MAX_SPARSITY = 0.7
# case -> (granularity, score method)
CASES = {"zeroth_block": ("block", "MEZO-GradOnly_sum"), "zeroth_layer": ("layer", "MEZO-GradOnly_sum"),
         "first_block": ("block", "GradOnly_sum"), "uniform": (None, "GradOnly_sum")}
T5_BLOCK_KEYS = ("attention_mask", "position_bias", "encoder_attention_mask", "encoder_decoder_position_bias",
                 "layer_head_mask", "cross_attn_layer_head_mask", "encoder_hidden_states")


def pruner_config(case):
    granularity, method = CASES[case]
    return dict(prune_spec=f"2-{KEEP}-1-1", num_samples=N_BATCHES * BATCH_SIZE,
                num_data_first_stage=N_BATCHES * BATCH_SIZE, sparsity_ratio_granularity=granularity,
                max_sparsity_per_layer=MAX_SPARSITY, score_method=method, num_noise=1, noise_eps=1e-3)


def mapping(model, granularity):
    names = prunable_names(model)
    if granularity is None:
        return {}
    return {k: (k if granularity == "layer" else ".".join(k.split(".")[:3])) for k in names}


def state_sha256(state):
    h = hashlib.sha256()
    for k in sorted(state):
        h.update(k.encode())
        h.update(state[k].detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def seed_run():
    np.random.seed(42)
    torch.manual_seed(42)


class _TupleLayer(LlamaDecoderLayer):
    """A decoder layer called the way the reference calls a T5 block."""

    def forward(self, x, **kwargs):
        assert set(kwargs) <= set(T5_BLOCK_KEYS)
        return (super().forward(x),)


class _Adapter(nn.Module):
    """What `T5LayerWandaPruner._prune` touches, around a `LlamaForCausalLM`."""

    def __init__(self, llama):
        super().__init__()
        self.model = llama.model
        self.model.config = llama.config            # `getattr(model, model_prefix).config.use_cache`
        for layer in self.model.layers:
            layer.__class__ = _TupleLayer

    def maybe_autocast(self, dtype=None):
        return contextlib.nullcontext()

    def forward(self, batch):
        x = self.model.embed_tokens(batch["input_ids"])
        for layer in self.model.layers:
            x = layer(x, **{k: None for k in T5_BLOCK_KEYS})[0]
        return x

    def release(self):
        for layer in self.model.layers:
            layer.__class__ = LlamaDecoderLayer
        del self.model.config


def load_reference(ref_root):
    """The LAVIS pruner files by path, the `lavis` package stubbed (as tests/golden/make_golden.py)."""
    def mod(name):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        return m

    for n in ["lavis", "lavis.common", "lavis.datasets", "lavis.models", "lavis.models.blip2_models",
              "lavis.models.t5_models", "lavis.models.clip_models", "lavis.compression",
              "lavis.compression.pruners"]:
        mod(n)

    class _Registry:
        mapping = {}

        @classmethod
        def register_pruner(cls, name):
            def wrap(c):
                cls.mapping[name] = c
                return c
            return wrap

    mod("lavis.common.registry").registry = _Registry
    mod("lavis.datasets.data_utils").prepare_sample = lambda samples, cuda_enabled=True: samples
    mod("lavis.models.blip2_models.blip2_t5").Blip2T5 = object
    mod("lavis.models.t5_models.t5").T5 = object
    mod("lavis.models.clip_models.eva_model").EVA_CLIP = object
    base = os.path.join(ref_root, "LAVIS/lavis/compression/pruners")
    loaded = {}
    for f in ["utils", "base_pruner", "layer_single_base_pruner", "wanda_pruner"]:
        name = f"lavis.compression.pruners.{f}"
        spec = importlib.util.spec_from_file_location(name, os.path.join(base, f + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        loaded[f] = m
    return loaded


def main():
    ref = load_reference(os.environ["ECOFLAP_REFERENCE_CHECKOUT"])
    LayerSparsity = ref["layer_single_base_pruner"].LayerSparsity
    T5LayerWandaPruner = ref["wanda_pruner"].T5LayerWandaPruner
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    out = {}
    try:
        for case, (granularity, method) in CASES.items():
            model = seeded_tiny()
            out[case + "_state_sha256"] = np.array(state_sha256(model.state_dict()))
            loader = batches(vocab=model.config.vocab_size)
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
            pruner = T5LayerWandaPruner(model=adapter, data_loader=with_image, model_prefix="model", **cfg)
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
        torch.set_num_threads(threads)
    np.savez_compressed(os.path.join(HERE, "g23_llama_wanda.npz"), **out)


if __name__ == "__main__":
    main()
