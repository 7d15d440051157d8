#!/usr/bin/env python3
"""Generate tests/golden/g19_clip_shape.npz by running the reference's OWN `CLIP` class
(CoOp/clip/model.py, loaded by file path from a checkout of ylsung/ECoFLaP) on states and inputs
drawn from fixed seeds:

    ECOFLAP_REFERENCE_CHECKOUT=/path/to/ECoFLaP python tests/golden/make_golden_clip.py

Nothing of the reference's source is copied: the fixture holds seeds, the sha256 of each initial
state (so that a test can prove it rebuilt the same state), and the bit patterns of the logits
and of the contrastive loss the reference computed.  Cases: toy towers in fp32 and in fp16 as
`convert_weights` leaves them; ViT-B/16 true widths, one block per tower, fp16.

(The reference's CLIP pruner is not run here: the build has no counterpart for it yet.)"""
import hashlib
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from ecoflap_amd.shapes import clip as C  # noqa: E402

CASES = {       # name -> (constructor of the build's module, reference CLIP arguments, image size, context, vocabulary)
    "toy": (lambda: C.clip_toy(1, 1), (16, 32, 1, 64, 16, 6, 64, 32, 2, 1), 32, 6, 64),
    "b16": (lambda: C.clip_slice(1, 1, fp16=False), (512, 224, 1, 768, 16, 77, 49408, 512, 8, 1), 224, 77, 49408),
}
SEED, BATCH = 19, 4


def state_sha256(state):
    h = hashlib.sha256()
    for k in sorted(state):
        h.update(k.encode())
        h.update(state[k].detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def inputs(image, context, vocab):
    g = torch.Generator().manual_seed(SEED + 1)
    img = torch.randn(BATCH, 3, image, image, generator=g)
    text = torch.randint(1, vocab - 1, (BATCH, context), generator=g)
    text[torch.arange(BATCH), torch.randint(1, context, (BATCH,), generator=g)] = vocab - 1    # end of text
    return img, text


def contrastive(per_image, per_text):
    diag = torch.arange(per_image.shape[0])
    return (F.cross_entropy(per_image.float(), diag) + F.cross_entropy(per_text.float(), diag)) / 2


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32).numpy()


def main():
    ref_root = os.environ["ECOFLAP_REFERENCE_CHECKOUT"]
    spec = importlib.util.spec_from_file_location("reference_clip_model",
                                                  os.path.join(ref_root, "CoOp", "clip", "model.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    out = {"seed": np.int64(SEED), "batch": np.int64(BATCH)}
    try:
        for name, (build, ref_args, image, context, vocab) in CASES.items():
            torch.manual_seed(SEED)
            mine = build()
            ref = R.CLIP(*ref_args)
            assert [n for n, _ in ref.named_parameters()] == [n for n, _ in mine.named_parameters()]
            ref.load_state_dict(mine.state_dict())
            ref.eval()
            img, text = inputs(image, context, vocab)
            for mode in (("fp32", "fp16") if name == "toy" else ("fp16",)):
                if mode == "fp16":
                    R.convert_weights(ref)
                with torch.no_grad():
                    per_image, per_text = ref(img, text)
                    loss = contrastive(per_image, per_text)
                key = f"{name}_{mode}"
                out[key + "_state_sha256"] = np.array(state_sha256(ref.state_dict()))
                out[key + "_logits_per_image"] = bits(per_image)
                out[key + "_logits_per_text"] = bits(per_text)
                out[key + "_loss"] = bits(loss.reshape(1))
                print(key, float(loss), out[key + "_state_sha256"])
    finally:
        torch.set_num_threads(threads)
    np.savez(os.path.join(HERE, "g19_clip_shape.npz"), **out)


if __name__ == "__main__":
    main()
