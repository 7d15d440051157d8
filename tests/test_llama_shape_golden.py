"""CPU: the LLaMA shape module IS transformers' `LlamaForCausalLM` as far as its outputs tell:
loaded (strictly: names and shapes are pinned) with the state tests/llama_fixture.py draws, its
torch path reproduces the logits and the loss transformers' own class computed (eager attention,
fp32; tests/golden/make_golden_llama.py), bit for bit."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llama_fixture as LF  # noqa: E402


def test_logits_and_loss_equal_transformers_bit_for_bit(golden_dir):
    from ecoflap_amd.shapes import llama as L
    g = np.load(os.path.join(golden_dir, "g22_llama_shape.npz"))
    assert int(g["seed"]) == LF.SEED
    stored = dict(zip([str(n) for n in g["config_names"]], g["config_values"].tolist()))
    assert stored == {k: float(v) for k, v in LF.CONFIG.items()}
    c = LF.CONFIG
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                    # (the recipe's setting: one summation order)
    try:
        model = L.llama_tiny(hidden_size=c["hidden_size"], heads=c["heads"], head_dim=c["head_dim"],
                             intermediate_size=c["intermediate_size"], layers=c["layers"],
                             vocab_size=c["vocab_size"]).eval()
        assert model.config.rms_norm_eps == c["rms_norm_eps"] and model.config.rope_theta == c["rope_theta"]
        model.load_state_dict(LF.fill_state(model.named_parameters()), strict=True)
        ids = LF.input_ids()
        assert np.array_equal(ids.numpy(), g["input_ids"])
        with torch.no_grad():
            out = model(ids, labels=ids)
    finally:
        torch.set_num_threads(threads)
    assert out.logits.dtype == torch.float32 and tuple(out.logits.shape) == (*LF.IDS_SHAPE, c["vocab_size"])
    assert np.array_equal(LF.bits(out.logits), g["logits"])
    assert np.array_equal(LF.bits(out.loss.reshape(1)), g["loss"])
