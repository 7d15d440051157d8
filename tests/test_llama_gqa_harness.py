"""CPU: `--llama_model` of the harness and `--model` of the two LLaMA launchers (LLaMA/main.py:31)
select the grouped-query shapes; the default command line is what it was; and `--shape llama --toy
--llama_model 3-8b` runs both pruners end to end on the oracle backend on a toy decoder with 2 query
heads on 1 key / value head."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launcher(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "LLaMA", "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _flag(flags, name):
    return flags[flags.index(name) + 1]


def test_the_default_command_line_is_unchanged():
    from ecoflap_amd.harness import build_parser
    launch = _launcher("_llama_launch")
    for name in ("ecoflap_zero", "ecoflap_first"):
        mod = _launcher(name)
        for method in ("wanda", "sparsegpt"):
            flags = mod.flags(method)
            assert "--llama_model" not in flags and flags == mod.flags(method, "huggyllama/llama-7b")
            assert _flag(flags, "--llama_prune_spec") == "32-0.4-1-1"
            assert os.path.join("llama_7b", "unstructured") in _flag(flags, "--out_dir")
            assert build_parser().parse_args(flags).llama_model == "7b"
    assert build_parser().parse_args(["--shape", "llama"]).llama_model == "7b"
    assert launch.split_model([]) == ("huggyllama/llama-7b", [])
    assert launch.split_model(["--toy", "--model", "a/b", "--device", "cpu"]) == ("a/b", ["--toy", "--device", "cpu"])


@pytest.mark.parametrize("model,key,layers,folder", [
    ("meta-llama/Meta-Llama-3-8B", "3-8b", 32, "llama3_8b"),
    ("/weights/Llama-2-70b-hf/", "2-70b", 80, "llama2_70b"),
    ("llama-7b", "7b", 32, "llama_7b"),
])
def test_model_maps_by_basename_to_shape_and_layer_count(model, key, layers, folder):
    from ecoflap_amd.harness import build_parser, config_dict
    for name in ("ecoflap_zero", "ecoflap_first"):
        flags = _launcher(name).flags("sparsegpt", model)
        args = build_parser().parse_args(flags)
        assert args.llama_model == key and args.pruning_method == "llama_sparsegpt_pruner"
        assert config_dict(args)["prune_spec"] == f"{layers}-0.4-1-1"
        assert _flag(flags, "--out_dir").endswith(os.path.join(folder, "unstructured", name + "_sparsegpt0.6"))
    with pytest.raises(SystemExit):
        _launcher("ecoflap_zero").flags("wanda", "facebook/opt-6.7b")


def test_an_unknown_llama_model_is_refused():
    from ecoflap_amd.harness import build_parser
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--shape", "llama", "--llama_model", "13b"])


@pytest.mark.parametrize("method", ["wanda", "sparsegpt"])
def test_toy_run_of_a_grouped_query_model(method, tmp_path):
    from oracle_backend import OracleKernels
    import ecoflap_amd.harness as H
    flags = _launcher("ecoflap_zero").flags(method, "meta-llama/Meta-Llama-3-8B")
    assert _flag(flags, "--llama_model") == "3-8b"
    for name, value in (("--llama_prune_spec", "2-0.4-1-1"), ("--num_data", "8"), ("--num_data_first_stage", "4"),
                        ("--out_dir", str(tmp_path))):
        flags[flags.index(name) + 1] = value
    model, table = H.main(flags + ["--toy", "--device", "cpu"], kernels=OracleKernels())
    assert model.config.num_attention_heads == 2 and model.config.num_key_value_heads == 1
    attn = model.model.layers[0].self_attn
    assert tuple(attn.q_proj.weight.shape) == (256, 64) and tuple(attn.k_proj.weight.shape) == (128, 64)
    assert tuple(attn.v_proj.weight.shape) == (128, 64)
    names = [k for k, v in model.named_parameters() if v.dim() == 2 and k.startswith("model.layers.")]
    assert list(table) == names and len(names) == 14
    assert max(table.values()) <= 0.7 + 1e-9 and len(set(table.values())) > 1
    state = dict(model.named_parameters())
    zeros = total = 0
    for n in names:
        w = state[n].data
        if method == "wanda":
            assert bool(((w == 0).sum(1) == int(w.shape[1] * table[n])).all()), n
        else:
            blocks = -(-w.shape[1] // 128)
            assert w.numel() * table[n] - blocks <= int((w == 0).sum()) <= w.numel() * table[n] + 2 * blocks, n
        zeros, total = zeros + int((w == 0).sum()), total + w.numel()
    assert abs(zeros / total - 0.6) < 0.01
    for k in ("model.embed_tokens.weight", "lm_head.weight"):
        assert int((state[k] == 0).sum()) == 0


def test_toy_default_is_the_plain_toy(tmp_path):
    from oracle_backend import OracleKernels
    import ecoflap_amd.harness as H
    flags = _launcher("ecoflap_zero").flags()
    for name, value in (("--llama_prune_spec", "2-0.4-1-1"), ("--num_data", "4"), ("--num_data_first_stage", "2"),
                        ("--out_dir", str(tmp_path))):
        flags[flags.index(name) + 1] = value
    model, _ = H.main(flags + ["--toy", "--device", "cpu"], kernels=OracleKernels())
    assert model.config.num_attention_heads == model.config.num_key_value_heads == 2
