"""The state and the input ids of `g22_llama_shape.npz`, for its recipe
(tests/golden/make_golden_llama.py) and its test alike: weights are not stored, they are drawn in
`named_parameters()` order from `numpy.random.default_rng(22).standard_normal` — 0.05 x the draw
for matrices, 1 + 0.1 x the draw for norm weights."""
import numpy as np
import torch

SEED = 22
CONFIG = dict(hidden_size=64, heads=2, head_dim=128, intermediate_size=176, layers=2, vocab_size=96,
              rms_norm_eps=1e-6, rope_theta=10000.0)
IDS_SHAPE = (2, 70)


def fill_state(named_parameters):
    """[(name, parameter)] in `named_parameters()` order -> {name: fp32 tensor}."""
    rng = np.random.default_rng(SEED)
    state = {}
    for name, p in named_parameters:
        draw = rng.standard_normal(tuple(p.shape)).astype(np.float32)
        value = 0.05 * draw if p.dim() == 2 else 1.0 + 0.1 * draw
        state[name] = torch.from_numpy(value.astype(np.float32))
    return state


def input_ids():
    rng = np.random.default_rng(SEED + 1)
    return torch.from_numpy(rng.integers(0, CONFIG["vocab_size"], size=IDS_SHAPE, dtype=np.int64))


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32).numpy()
