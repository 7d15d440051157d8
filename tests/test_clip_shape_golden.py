"""CPU: the OpenAI-CLIP shape module IS the reference's model as far as its outputs tell:
rebuilt from `g19_clip_shape.npz`'s seed (the state's sha256 proves the rebuild) it reproduces the
logits and the contrastive loss the reference's own `CLIP` class computed (CoOp/clip/model.py, run
by tests/golden/make_golden_clip.py), bit for bit — toy towers in fp32 and fp16, and ViT-B/16's
true widths (one block per tower) in fp16."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_clip as G  # noqa: E402  (its helpers; the reference is only touched by its main())

from ecoflap_amd.shapes import clip as C  # noqa: E402


@pytest.mark.parametrize("name,mode", [("toy", "fp32"), ("toy", "fp16"), ("b16", "fp16")])
def test_logits_and_loss_equal_the_reference_bit_for_bit(golden_dir, name, mode):
    g = np.load(os.path.join(golden_dir, "g19_clip_shape.npz"))
    assert int(g["seed"]) == G.SEED and int(g["batch"]) == G.BATCH
    build, _, image, context, vocab = G.CASES[name]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                    # (the recipe's setting: one summation order)
    try:
        torch.manual_seed(G.SEED)
        model = build().eval()
        if mode == "fp16":
            C.half_weights(model)
        key = f"{name}_{mode}"
        assert G.state_sha256(model.state_dict()) == str(g[key + "_state_sha256"])
        img, text = G.inputs(image, context, vocab)
        with torch.no_grad():
            per_image, per_text = model(img, text)
            loss = G.contrastive(per_image, per_text)
    finally:
        torch.set_num_threads(threads)
    assert per_image.dtype == (torch.float16 if mode == "fp16" else torch.float32)
    assert np.array_equal(G.bits(per_image), g[key + "_logits_per_image"])
    assert np.array_equal(G.bits(per_text), g[key + "_logits_per_text"])
    assert np.array_equal(G.bits(loss.reshape(1)), g[key + "_loss"])
