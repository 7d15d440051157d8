"""CPU: `harness --shape llama --toy` with the flag sets of the two LLaMA launchers (the toy's
sizes in place of LLaMA-7B's) on the oracle backend: one table key per prunable matrix, and the
requested overall sparsity within one element per row."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launcher(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "LLaMA", "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _flag(flags, name):
    return flags[flags.index(name) + 1]


def test_launchers_carry_the_shell_scripts_values():
    zero, first = _launcher("ecoflap_zero").flags(), _launcher("ecoflap_first").flags()
    for f in (zero, first):
        assert _flag(f, "--shape") == "llama" and _flag(f, "--pruning_method") == "llama_wanda_pruner"
        assert _flag(f, "--llama_prune_spec") == "32-0.4-1-1"
        assert _flag(f, "--sparsity_ratio_granularity") == "block"
        assert float(_flag(f, "--max_sparsity_per_layer")) == 0.7
        assert _flag(f, "--num_data") == "128" and _flag(f, "--seed") == "0"
        assert "--prunining_dataset_batch_size" not in f          # the harness's default, 1
    assert _flag(zero, "--score_method") == "MEZO-GradOnly_sum" and _flag(zero, "--num_data_first_stage") == "32"
    assert _flag(first, "--score_method") == "GradOnly_sum" and _flag(first, "--num_data_first_stage") == "128"
    assert _flag(zero, "--out_dir").endswith(os.path.join("llama_7b", "unstructured", "ecoflap_zero0.6"))
    assert _flag(first, "--out_dir").endswith(os.path.join("llama_7b", "unstructured", "ecoflap_first0.6"))


def test_parser_defaults_for_llama():
    from ecoflap_amd.harness import build_parser, config_dict
    args = build_parser().parse_args(_launcher("ecoflap_zero").flags())
    assert args.prunining_dataset_batch_size is None            # -> 1 in build_model_and_loader
    cfg = config_dict(args)
    assert cfg["prune_spec"] == "32-0.4-1-1" and cfg["model_prefix"] == "model"
    assert cfg["num_samples"] == 128 and cfg["num_data_first_stage"] == 32


@pytest.mark.parametrize("launcher", ["ecoflap_zero", "ecoflap_first"])
def test_toy_run_of_each_launcher(launcher, tmp_path):
    from oracle_backend import OracleKernels
    import ecoflap_amd.harness as H
    flags = _launcher(launcher).flags()
    for name, value in (("--llama_prune_spec", "2-0.4-1-1"), ("--num_data", "8"), ("--num_data_first_stage", "4"),
                        ("--out_dir", str(tmp_path))):
        flags[flags.index(name) + 1] = value
    model, table = H.main(flags + ["--toy", "--device", "cpu", "--save_pruned_model"], kernels=OracleKernels())
    names = [k for k, v in model.named_parameters() if v.dim() == 2 and k.startswith("model.layers.")]
    assert list(table) == names and len(names) == 14
    assert max(table.values()) <= 0.7 + 1e-9 and len(set(table.values())) > 1
    state = dict(model.named_parameters())
    zeros = total = rows = 0
    for n in names:
        w = state[n].data
        assert bool(((w == 0).sum(1) == int(w.shape[1] * table[n])).all()), n
        zeros, total, rows = zeros + int((w == 0).sum()), total + w.numel(), rows + w.shape[0]
    # the allocator meets 0.6 over the prunable parameters; int() per row loses less than one element
    assert 0.6 * total - rows - 1 <= zeros <= 0.6 * total + 1, (zeros, 0.6 * total, rows)
    for k in ("model.embed_tokens.weight", "lm_head.weight"):
        assert int((state[k] == 0).sum()) == 0
    assert model.seqlen == 128 and model.config.use_cache is False
    assert os.path.exists(tmp_path / "pruned_checkpoint" / (launcher + ".pth"))
    assert os.path.exists(tmp_path / "sparsity_dict" / (launcher + ".yaml"))
