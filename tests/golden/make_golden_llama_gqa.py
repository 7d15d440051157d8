#!/usr/bin/env python3
"""Generate tests/golden/g25_llama_gqa_shape.npz by running transformers' OWN `LlamaForCausalLM`
(the installed `transformers`, eager attention, fp32, one thread) with grouped-query attention —
4 query heads on 2 key / value heads — on the state and the ids of tests/llama_gqa_fixture.py:

    python tests/golden/make_golden_llama_gqa.py

The fixture holds the config's numbers, the input ids, the bit patterns of the logits and of the
loss (`labels = input_ids`) and transformers' parameter names and shapes in `named_parameters()`
order; weights are not stored (llama_fixture.fill_state draws them)."""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import llama_fixture as LF  # noqa: E402
import llama_gqa_fixture as GF  # noqa: E402


def main():
    import transformers
    from transformers import LlamaConfig, LlamaForCausalLM

    c = GF.CONFIG
    cfg = LlamaConfig(hidden_size=c["hidden_size"], num_attention_heads=c["heads"],
                      num_key_value_heads=c["kv_heads"], head_dim=c["head_dim"],
                      intermediate_size=c["intermediate_size"], num_hidden_layers=c["layers"],
                      vocab_size=c["vocab_size"], rms_norm_eps=c["rms_norm_eps"],
                      rope_theta=c["rope_theta"], max_position_embeddings=128, tie_word_embeddings=False,
                      attention_bias=False, mlp_bias=False, attn_implementation="eager")
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        ref = LlamaForCausalLM(cfg).eval().float()
        shapes = [(n, tuple(p.shape)) for n, p in ref.named_parameters()]
        ref.load_state_dict(LF.fill_state(ref.named_parameters()), strict=True)
        ids = GF.input_ids()
        with torch.no_grad():
            out = ref(input_ids=ids, labels=ids, use_cache=False)
    finally:
        torch.set_num_threads(threads)
    assert out.logits.dtype == torch.float32 and tuple(out.logits.shape) == (*GF.IDS_SHAPE, c["vocab_size"])
    np.savez(os.path.join(HERE, "g25_llama_gqa_shape.npz"),
             seed=np.int64(LF.SEED), transformers_version=np.array(transformers.__version__),
             config_names=np.array(sorted(c)), config_values=np.array([float(c[k]) for k in sorted(c)]),
             parameter_names=np.array([n for n, _ in shapes], dtype=str),
             parameter_shapes=np.array([list(s) + [0] * (2 - len(s)) for _, s in shapes], dtype=np.int64),
             input_ids=ids.numpy(), logits=LF.bits(out.logits), loss=LF.bits(out.loss.reshape(1)))
    print("transformers", transformers.__version__, "loss", float(out.loss))


if __name__ == "__main__":
    main()
