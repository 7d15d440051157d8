"""CPU: the LLaMA shape module with grouped-query attention IS transformers' `LlamaForCausalLM` as
far as its outputs tell: 4 query heads on 2 key / value heads, loaded with the state
tests/llama_fixture.py draws, its torch path reproduces the logits and the loss transformers' own
class computed (eager attention, fp32; tests/golden/make_golden_llama_gqa.py) bit for bit, under
transformers' parameter names, shapes and order; `kv_heads == heads` is the model without the
argument; and the true shapes (`llama3_8b`, `llama2_70b`) have the parameters of transformers'
class for the same config, built on the meta device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llama_fixture as LF  # noqa: E402
import llama_gqa_fixture as GF  # noqa: E402


def _shapes(model):
    return [(n, tuple(p.shape)) for n, p in model.named_parameters()]


def test_logits_loss_names_and_shapes_equal_transformers_bit_for_bit(golden_dir):
    g = np.load(os.path.join(golden_dir, "g25_llama_gqa_shape.npz"))
    assert int(g["seed"]) == LF.SEED
    stored = dict(zip([str(n) for n in g["config_names"]], g["config_values"].tolist()))
    assert stored == {k: float(v) for k, v in GF.CONFIG.items()}
    c = GF.CONFIG
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                    # (the recipe's setting: one summation order)
    try:
        model = GF.tiny().eval()
        assert model.config.num_attention_heads == 4 and model.config.num_key_value_heads == 2
        assert model.config.rms_norm_eps == c["rms_norm_eps"] and model.config.rope_theta == c["rope_theta"]
        want = [(str(n), tuple(int(d) for d in s if d)) for n, s in zip(g["parameter_names"], g["parameter_shapes"])]
        assert _shapes(model) == want           # names, shapes and order
        attn = model.model.layers[0].self_attn
        assert tuple(attn.q_proj.weight.shape) == (512, 64) and tuple(attn.k_proj.weight.shape) == (256, 64)
        assert tuple(attn.v_proj.weight.shape) == (256, 64) and tuple(attn.o_proj.weight.shape) == (64, 512)
        model.load_state_dict(LF.fill_state(model.named_parameters()), strict=True)
        ids = GF.input_ids()
        assert np.array_equal(ids.numpy(), g["input_ids"])
        with torch.no_grad():
            out = model(ids, labels=ids)
    finally:
        torch.set_num_threads(threads)
    assert out.logits.dtype == torch.float32 and tuple(out.logits.shape) == (*GF.IDS_SHAPE, c["vocab_size"])
    assert np.array_equal(LF.bits(out.logits), g["logits"])
    assert np.array_equal(LF.bits(out.loss.reshape(1)), g["loss"])


def test_kv_heads_equal_to_heads_is_the_model_without_the_argument():
    from ecoflap_amd.shapes import llama as L
    torch.manual_seed(3)
    plain = L.llama_tiny()
    torch.manual_seed(3)
    same = L.llama_tiny(kv_heads=2)
    assert plain.config.num_key_value_heads == same.config.num_key_value_heads == 2
    assert list(plain.state_dict()) == list(same.state_dict())
    for k, v in plain.state_dict().items():
        assert torch.equal(v, same.state_dict()[k]), k
    assert vars(L.llama_config(64, 2, 176, 2, 96)) == vars(L.llama_config(64, 2, 176, 2, 96, kv_heads=2))
    with pytest.raises(ValueError):
        L.llama_tiny(heads=4, kv_heads=3)


@pytest.mark.parametrize("name,numbers", [
    ("llama3_8b", dict(layers=32, hidden=4096, heads=32, kv=8, mlp=14336, vocab=128256, eps=1e-5, theta=500000.0)),
    ("llama2_70b", dict(layers=80, hidden=8192, heads=64, kv=8, mlp=28672, vocab=32000, eps=1e-5, theta=10000.0)),
    ("mistral_7b", dict(layers=32, hidden=4096, heads=32, kv=8, mlp=14336, vocab=32000, eps=1e-5, theta=10000.0)),
])
def test_the_true_shapes_have_transformers_parameters(name, numbers):
    from transformers import LlamaConfig, LlamaForCausalLM
    from ecoflap_amd.shapes import llama as L
    n = numbers
    with torch.device("meta"):
        mine = getattr(L, name)()
        theirs = LlamaForCausalLM(LlamaConfig(
            hidden_size=n["hidden"], num_attention_heads=n["heads"], num_key_value_heads=n["kv"],
            intermediate_size=n["mlp"], num_hidden_layers=n["layers"], vocab_size=n["vocab"],
            rms_norm_eps=n["eps"], rope_theta=n["theta"], tie_word_embeddings=False, attention_bias=False,
            mlp_bias=False))
    c = mine.config
    assert (c.num_hidden_layers, c.hidden_size, c.num_attention_heads, c.num_key_value_heads, c.head_dim,
            c.intermediate_size, c.vocab_size, c.rms_norm_eps, c.rope_theta) == \
           (n["layers"], n["hidden"], n["heads"], n["kv"], 128, n["mlp"], n["vocab"], n["eps"], n["theta"])
    assert mine.seqlen == 2048 and all(p.dtype == torch.float16 for p in mine.parameters())
    assert _shapes(mine) == _shapes(theirs)
    assert sum(p.numel() for p in mine.parameters()) == sum(p.numel() for p in theirs.parameters())
