"""The model and the calibration batches of the LLaMA pruner tests and of `g23_llama_wanda.npz`
(recipe: tests/golden/make_golden_llama_pruner.py): weights are not stored, they are drawn from a
seed as tests/llama_fixture.py draws them."""
import hashlib

import numpy as np
import torch

from llama_fixture import fill_state

N_BATCHES, BATCH_SIZE, SEQLEN, BATCH_SEED = 4, 2, 24, 23


def seeded_tiny(dtype=torch.float32, **shape):
    """`llama_tiny(**shape)` with the seeded state of tests/llama_fixture.py, in `dtype`."""
    from ecoflap_amd.shapes.llama import llama_tiny
    model = llama_tiny(dtype=torch.float32, **shape)
    model.load_state_dict(fill_state(list(model.named_parameters())))
    return (model if dtype == torch.float32 else model.to(dtype)).eval()


def batches(vocab=96, n=N_BATCHES, batch_size=BATCH_SIZE, seqlen=SEQLEN, device=None):
    from ecoflap_amd.shapes.llama import llama_batches
    return llama_batches(n, batch_size, seqlen, vocab, seed=BATCH_SEED, device=device)


def prunable_names(model):
    return [k for k, v in model.named_parameters() if v.dim() == 2 and k.startswith("model.layers.")]


def sha256(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().contiguous().view(torch.uint8).numpy())
                          .tobytes()).hexdigest()
