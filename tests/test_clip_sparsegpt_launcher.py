"""CPU: CoOp/scripts/coop/ecoflap_sparsegpt.py holds the two configurations of the reference's
ecoflap_sparsegpt.sh, and the harness runs `clip_sparsegpt_pruner` from its flags end to end."""
import importlib.util
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_clip_pruner as G  # noqa: E402

from oracle_backend import OracleKernels, torch_cpu_normal  # noqa: E402


def _launcher():
    spec = importlib.util.spec_from_file_location(
        "coop_ecoflap_sparsegpt", os.path.join(ROOT, "CoOp", "scripts", "coop", "ecoflap_sparsegpt.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pruner_is_registered_with_the_reference_keywords():
    from ecoflap_amd.registry import registry
    from ecoflap_amd.pruners.clip import CLIPLayerWandaPruner
    cls = registry.get_pruner_class("clip_sparsegpt_pruner")
    assert cls.pruner_name == "clip_sparsegpt_pruner" and issubclass(cls, CLIPLayerWandaPruner)
    # stage 1 is shared with `clip_wanda_pruner`, not copied
    assert cls.get_sparsity is CLIPLayerWandaPruner.get_sparsity and cls.prune is CLIPLayerWandaPruner.prune


def test_launcher_offers_the_reference_configurations():
    L = _launcher()
    import ecoflap_amd.harness as H
    assert list(L.CONFIGS) == ["sparsegpt", "ecoflap"]
    assert [L.CONFIGS[k][0] for k in L.CONFIGS] == ["sparsegpt0.6", "sparsegpt_mezo0.6"]
    a = H.build_parser().parse_args(L.harness_flags("sparsegpt"))
    cfg = H.config_dict(a)
    assert a.shape == "clip" and a.pruning_method == "clip_sparsegpt_pruner" and a.seed == 1
    assert a.job_id == "sparsegpt0.6" and a.out_dir.endswith(os.path.join("ZeroshotCLIP", "sparsegpt0.6_vit_b16_s1"))
    assert cfg["visual_prune_spec"] == cfg["language_prune_spec"] == "1-0.6-1-1"
    assert cfg["sparsity_ratio_granularity"] is None and cfg["num_samples"] == 128
    assert cfg["language_model_prefix"] == "transformer" and cfg["visual_model_prefix"] == "visual.transformer"
    b_args = H.build_parser().parse_args(L.harness_flags("ecoflap"))
    b = H.config_dict(b_args)
    assert b_args.job_id == "sparsegpt_mezo0.6"
    assert b["sparsity_ratio_granularity"] == "block" and b["max_sparsity_per_layer"] == 0.5
    assert b["score_method"] == "MEZO-GradOnly_sum" and b["num_data_first_stage"] == 32


def test_harness_runs_the_ecoflap_configuration(tmp_path, monkeypatch):
    import ecoflap_amd
    import ecoflap_amd.harness as H
    real = ecoflap_amd.load_pruner

    def with_checker(pruner_name, model, loader, cfg_path=None, cfg=None):
        assert pruner_name == "clip_sparsegpt_pruner"
        return real(pruner_name, model, loader, cfg=dict(cfg, kernels=OracleKernels(), z_source=torch_cpu_normal))

    monkeypatch.setattr(ecoflap_amd, "load_pruner", with_checker)
    L = _launcher()
    argv = L.harness_flags("ecoflap", out_root=str(tmp_path)) + [
        "--toy", "--device", "cpu", "--num_data", "16", "--num_data_first_stage", "16",
        "--prunining_dataset_batch_size", "4"]
    out_dir = H.build_parser().parse_args(argv).out_dir
    model, table = H.main(argv)
    assert os.path.exists(os.path.join(out_dir, "pruned_checkpoint", "sparsegpt_mezo0.6.pth"))
    saved = json.load(open(os.path.join(out_dir, "sparsity_dict.json")))
    assert saved == table and len(saved) == 16
    assert max(saved.values()) <= 0.5 + 1e-9
    mats = G.prunable(model)
    kept = sum(p.numel() * (1 - saved[n]) for n, p in mats)
    assert abs(kept / sum(p.numel() for _, p in mats) - 0.6) < 1e-3
    # SparseGPT thresholds per block of 128 columns at int(rows * count * sparsity): every matrix
    # ends within one element per column block of its table entry (an exact zero weight aside)
    for n, p in mats:
        blocks = -(-p.shape[1] // 128)
        zeros = int((p.data == 0).sum())
        assert abs(zeros - p.numel() * saved[n]) <= 2 * blocks + 1, (n, zeros, p.numel() * saved[n])
