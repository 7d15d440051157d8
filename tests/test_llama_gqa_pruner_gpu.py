"""GPU: `llama_wanda_pruner` and `llama_sparsegpt_pruner` end to end on a grouped-query decoder —
the shape of tests/test_llama_pruner_gpu.py with 2 query heads on 1 key / value head (hidden 128,
MLP 256, 2 layers, vocabulary 96, fp16, 64 tokens), so `q_proj` has 256 rows and `k_proj` / `v_proj`
128: the HIP kernels against the oracle's arithmetic on the same GPU forward (which runs
`ecoflap_causal_attention_gqa`), the staged, graph-replayed, batched stage 1 against the plain
closure, and SparseGPT's twin sets (q / k / v with unequal rows in ONE grouped call) against one
sweep per matrix."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPE = dict(hidden_size=128, heads=2, kv_heads=1, head_dim=128, intermediate_size=256, layers=2, vocab_size=96,
             seqlen=64)
KEEP = 0.4          # the launchers' sparsity 0.6


def run(pruner_name, kernels=None, n_batches=4, batch=2, **extra):
    from ecoflap_amd import load_pruner
    from ecoflap_amd.shapes import fused
    from llama_pruner_fixture import batches, prunable_names, seeded_tiny, sha256
    model = seeded_tiny(dtype=torch.float16, **SHAPE).cuda()
    attn = model.model.layers[0].self_attn
    assert attn.q_proj.weight.shape[0] == 256 and attn.k_proj.weight.shape[0] == attn.v_proj.weight.shape[0] == 128
    loader = batches(vocab=96, n=n_batches, batch_size=batch, seqlen=SHAPE["seqlen"], device="cuda")
    before = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    np.random.seed(42)
    torch.manual_seed(42)
    cfg = dict(prune_spec=f"2-{KEEP}-1-1", num_samples=n_batches * batch, num_data_first_stage=n_batches * batch,
               sparsity_ratio_granularity="block", max_sparsity_per_layer=0.7, score_method="MEZO-GradOnly_sum")
    cfg.update(extra)
    if kernels is not None:
        cfg["kernels"] = kernels
    pruner = load_pruner(pruner_name, model, loader, cfg=cfg)
    served, real = [0, 0], fused.causal_attention

    def counting(*args, **kwargs):
        y = real(*args, **kwargs)
        if not torch.is_grad_enabled():
            served[0] += 1
            served[1] += y is not None and kwargs.get("kv_heads") == 1
        return y

    fused.causal_attention = counting
    try:
        model, table = pruner.prune()
    finally:
        fused.causal_attention = real
    torch.cuda.synchronize()
    assert served[0] > 0 and served[0] == served[1]     # every no-grad forward took the grouped-query kernel
    after = {n: p.detach().cpu() for n, p in model.named_parameters()}
    names = prunable_names(model)
    return dict(table=table, before=before, after=after, names=names,
                hashes={n: sha256(after[n]) for n in names},
                losses=None if pruner.last_loss_table is None else np.array(pruner.last_loss_table),
                stats=dict(pruner.stage_stats))


def test_wanda_hip_equals_oracle_on_the_same_forward():
    """Table, stage-1 losses and every pruned weight bit for bit; the stage-2 column statistics are
    handed over under rtol 1e-5 (oracle_backend.OracleKernelsK6Synced says why)."""
    from ecoflap_amd import hip
    from oracle_backend import OracleKernelsK6Synced
    a = run("llama_wanda_pruner")
    torch.cuda.empty_cache()
    checker = OracleKernelsK6Synced(hip.HipKernels())
    b = run("llama_wanda_pruner", checker)
    assert list(a["table"]) == a["names"] and len(a["table"]) == 14
    assert a["table"] == b["table"] and len(set(a["table"].values())) > 1
    assert max(a["table"].values()) <= 0.7 + 1e-9
    assert np.array_equal(a["losses"], b["losses"])
    assert checker.k6_calls > 0
    bad = [n for n in a["after"] if not torch.equal(a["after"][n], b["after"][n])]
    assert not bad, f"{len(bad)} parameters differ: {bad[:4]}"
    for n in a["names"]:
        w = a["after"][n]
        want = int(w.shape[1] * a["table"][n])
        zeros = (w == 0).sum(1)
        assert bool((zeros == want).all()), (n, want, zeros.min().item(), zeros.max().item())
    for n in a["after"]:
        if n not in a["names"]:
            assert torch.equal(a["after"][n], a["before"][n]), n


def test_wanda_staged_batched_graph_run_equals_the_plain_closure(monkeypatch):
    plain = run("llama_wanda_pruner", prefix_cache=False)
    torch.cuda.empty_cache()
    monkeypatch.setenv("ECOFLAP_VERIFY_BATCHED", "1")       # every chunk of the batched path checked bit for bit
    staged = run("llama_wanda_pruner", use_graphs=True, eval_batch=16)
    assert staged["table"] == plain["table"]
    assert np.array_equal(staged["losses"], plain["losses"])
    assert staged["hashes"] == plain["hashes"]
    sf = staged["stats"]["stage1"]["suffix_forward"]
    print("suffix_forward:", sf)
    assert sf["graph_replays"] > 0 and sf["stage_calls"] < sf["stage_calls_full"]
    assert "suffix_forward" not in plain["stats"]["stage1"]


def test_sparsegpt_twin_sets_with_unequal_rows_side_by_side_equal_one_by_one():
    on = run("llama_sparsegpt_pruner", n_batches=8, batch=1, sparsegpt_group_twins=True)
    torch.cuda.empty_cache()
    off = run("llama_sparsegpt_pruner", n_batches=8, batch=1, sparsegpt_group_twins=False)
    assert on["table"] == off["table"] and len(on["table"]) == 14 and len(set(on["table"].values())) > 1
    assert np.array_equal(on["losses"], off["losses"])
    bad = [n for n in on["after"] if not torch.equal(on["after"][n].view(torch.int16), off["after"][n].view(torch.int16))]
    assert not bad, f"{len(bad)} parameters differ: {bad[:4]}"
    # q / k / v (256, 128 and 128 rows) and gate / up of each of the two blocks: one grouped call each
    assert on["stats"]["sparsegpt_group_calls"] == 4
    assert on["stats"]["sparsegpt_group_members"] == [3, 2, 3, 2]
    assert "sparsegpt_group_calls" not in off["stats"] and "sparsegpt_group_members" not in off["stats"]
    for n in on["names"]:
        zeros = float((on["after"][n] == 0).float().mean())
        assert abs(zeros - on["table"][n]) < 0.01, (n, zeros, on["table"][n])
