"""The grouped-query toy decoder of `g25_llama_gqa_shape.npz` and `g26_llama_gqa_pruners.npz`, for
their recipes and their tests alike: 4 query heads on 2 key / value heads, everything else the
config of tests/llama_fixture.py; the state is drawn by that module's `fill_state` (same seed, in
`named_parameters()` order), the ids [2, 40] from its seed + 1."""
import numpy as np
import torch

import llama_fixture as LF

CONFIG = dict(LF.CONFIG, heads=4, kv_heads=2)
IDS_SHAPE = (2, 40)
TINY_KEYS = ("hidden_size", "heads", "kv_heads", "head_dim", "intermediate_size", "layers", "vocab_size")


def tiny():
    from ecoflap_amd.shapes import llama as L
    return L.llama_tiny(**{k: CONFIG[k] for k in TINY_KEYS})


def input_ids():
    rng = np.random.default_rng(LF.SEED + 1)
    return torch.from_numpy(rng.integers(0, CONFIG["vocab_size"], size=IDS_SHAPE, dtype=np.int64))
