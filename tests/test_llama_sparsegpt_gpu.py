"""GPU: `llama_sparsegpt_pruner` end to end on `llama_tiny(hidden 256, two heads of 128, MLP 384, 2
layers, vocabulary 96)` in fp16 at 64 tokens with 8 calibration batches of one sample (512 tokens:
every Hessian is full rank; every matrix has at least two column blocks, so the trailing update
runs): twin sets swept side by side against one by one, the HIP kernels against the oracle's
arithmetic on the same GPU forward, and the structure of the default run."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPE = dict(hidden_size=256, heads=2, head_dim=128, intermediate_size=384, layers=2, vocab_size=96, seqlen=64)
BATCHES, BATCH = 8, 1
KEEP = 0.4          # the launchers' sparsity 0.6


def _setup():
    from llama_pruner_fixture import batches, seeded_tiny
    model = seeded_tiny(dtype=torch.float16, **SHAPE).cuda()
    return model, batches(vocab=96, n=BATCHES, batch_size=BATCH, seqlen=SHAPE["seqlen"], device="cuda")


def run(kernels=None, granularity="block", **extra):
    from ecoflap_amd import load_pruner
    from llama_pruner_fixture import prunable_names
    model, loader = _setup()
    before = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    np.random.seed(42)
    torch.manual_seed(42)
    cfg = dict(prune_spec=f"2-{KEEP}-1-1", num_samples=BATCHES * BATCH, num_data_first_stage=BATCHES * BATCH,
               sparsity_ratio_granularity=granularity, max_sparsity_per_layer=0.7,
               score_method="MEZO-GradOnly_sum")
    cfg.update(extra)
    if kernels is not None:
        cfg["kernels"] = kernels
    pruner = load_pruner("llama_sparsegpt_pruner", model, loader, cfg=cfg)
    model, table = pruner.prune()
    torch.cuda.synchronize()
    with torch.no_grad():
        loss = float(model(loader[0]["input_ids"], labels=loader[0]["input_ids"]).loss)
    after = {n: p.detach().cpu() for n, p in model.named_parameters()}
    return dict(table=table, before=before, after=after, names=prunable_names(model), loss=loss,
                losses=None if pruner.last_loss_table is None else np.array(pruner.last_loss_table),
                stats=dict(pruner.stage_stats))


_RUNS = {}


def default_run(grouped):
    if grouped not in _RUNS:
        _RUNS[grouped] = run(sparsegpt_group_twins=grouped)
        torch.cuda.empty_cache()
    return _RUNS[grouped]


def test_twin_sets_side_by_side_equal_one_by_one_bit_for_bit():
    on, off = default_run(True), default_run(False)
    assert on["table"] == off["table"] and len(on["table"]) == 14 and len(set(on["table"].values())) > 1
    assert np.array_equal(on["losses"], off["losses"])
    bad = [n for n in on["after"] if not torch.equal(on["after"][n].view(torch.int16), off["after"][n].view(torch.int16))]
    assert not bad, f"{len(bad)} parameters differ: {bad[:4]}"
    # q / k / v and gate / up of each of the two blocks
    assert on["stats"]["sparsegpt_group_calls"] == 4
    assert on["stats"]["sparsegpt_group_members"] == [3, 2, 3, 2]
    assert "sparsegpt_group_calls" not in off["stats"] and "sparsegpt_group_members" not in off["stats"]


def test_hip_equals_oracle_on_the_same_forward():
    """Table, stage-1 losses and every parameter bit for bit, with the library on both sides for the
    Hessian update, the factorisations and the trailing product (`whole_matrix_sweep` off: the
    oracle backend has no one-call sweep)."""
    from oracle_backend import OracleKernels
    from ecoflap_amd.pruners.sparsegpt import SparseGPT
    own, mfma = SparseGPT.use_own_cholesky, SparseGPT.use_mfma_hessian
    SparseGPT.use_own_cholesky = False
    SparseGPT.use_mfma_hessian = False
    try:
        a = run(whole_matrix_sweep=False)
        torch.cuda.empty_cache()
        b = run(OracleKernels(), whole_matrix_sweep=False)
    finally:
        SparseGPT.use_own_cholesky, SparseGPT.use_mfma_hessian = own, mfma
    assert a["table"] == b["table"] and len(set(a["table"].values())) > 1
    assert np.array_equal(a["losses"], b["losses"])
    bad = [n for n in a["after"] if not torch.equal(a["after"][n], b["after"][n])]
    assert not bad, f"{len(bad)} parameters differ: {bad[:4]}"
    assert all(float((a["after"][n] == 0).float().mean()) > 0.3 for n in a["names"])


def test_structure_of_the_default_run():
    a = default_run(True)
    assert list(a["table"]) == a["names"] and max(a["table"].values()) <= 0.7 + 1e-9
    for n in a["names"]:
        zeros = float((a["after"][n] == 0).float().mean())
        print(f"{n}: {zeros:.4f} zeros, table {a['table'][n]:.4f}")
        assert abs(zeros - a["table"][n]) < 0.01, (n, zeros, a["table"][n])
    assert np.isfinite(a["loss"])
    # uniform: stage 1 is skipped, nothing is perturbed — what is not prunable is untouched
    u = run(granularity=None)
    assert all(u["table"][n] == 1 - KEEP for n in u["names"]) and u["losses"] is None
    for n in u["names"]:
        assert abs(float((u["after"][n] == 0).float().mean()) - (1 - KEEP)) < 0.01, n
    for n in u["after"]:
        if n not in u["names"]:
            assert torch.equal(u["after"][n], u["before"][n]), n
    assert np.isfinite(u["loss"])
