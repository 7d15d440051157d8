"""GPU: the LLaMA decoder's staged forward with the fused loss kernel, and `llama_wanda_pruner` end to
end on `llama_tiny(hidden 128, one head of 128, MLP 256, 2 layers, vocabulary 96)` in fp16 at 64
tokens, 4 calibration batches of 2: the HIP kernels against the oracle's arithmetic on the same GPU
forward, and the staged, graph-replayed, batched stage 1 against the plain closure."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPE = dict(hidden_size=128, heads=1, head_dim=128, intermediate_size=256, layers=2, vocab_size=96, seqlen=64)
BATCHES, BATCH = 4, 2
KEEP = 0.4          # the launchers' sparsity 0.6


def _setup():
    from llama_pruner_fixture import batches, seeded_tiny
    model = seeded_tiny(dtype=torch.float16, **SHAPE).cuda()
    return model, batches(vocab=96, n=BATCHES, batch_size=BATCH, seqlen=SHAPE["seqlen"], device="cuda")


def run(kernels=None, **extra):
    from ecoflap_amd import load_pruner
    from llama_pruner_fixture import prunable_names, sha256
    model, loader = _setup()
    before = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    np.random.seed(42)
    torch.manual_seed(42)
    cfg = dict(prune_spec=f"2-{KEEP}-1-1", num_samples=BATCHES * BATCH, num_data_first_stage=BATCHES * BATCH,
               sparsity_ratio_granularity="block", max_sparsity_per_layer=0.7, score_method="MEZO-GradOnly_sum")
    cfg.update(extra)
    if kernels is not None:
        cfg["kernels"] = kernels
    pruner = load_pruner("llama_wanda_pruner", model, loader, cfg=cfg)
    model, table = pruner.prune()
    torch.cuda.synchronize()
    after = {n: p.detach().cpu() for n, p in model.named_parameters()}
    names = prunable_names(model)
    return dict(table=table, before=before, after=after, names=names,
                hashes={n: sha256(after[n]) for n in names},
                losses=None if pruner.last_loss_table is None else np.array(pruner.last_loss_table),
                stats=dict(pruner.stage_stats))


def test_stages_compose_to_forward_and_the_fused_loss_agrees_with_torch(monkeypatch):
    model, loader = _setup()
    ids = loader[0]["input_ids"]
    with torch.no_grad():
        want = model(ids, labels=ids)
        state = {"input_ids": ids}
        for _, _, fn in model.stage_plan():
            state = fn(state)
        assert torch.equal(state["logits"], want.logits) and torch.equal(state["loss"], want.loss)
        assert want.loss.dtype == torch.float32 and want.loss.dim() == 0
        monkeypatch.setenv("ECOFLAP_NO_FUSED_LOSS", "1")
        chain = model(ids, labels=ids)
        monkeypatch.delenv("ECOFLAP_NO_FUSED_LOSS")
    assert torch.equal(chain.logits, want.logits)
    # both are fp32 evaluations of the fp64 mean L of the same fp16 logits: torch's rows are within
    # E_torch of fp64, the kernel's within 2 E_torch + 4 * 2^-24 (|max| + ln V) (tests/test_lm_loss_gpu.py),
    # and each mean adds at most rows * 2^-24 L
    logits = want.logits.view(-1, 96)
    targets = F.pad(ids, (0, 1), value=-100)[..., 1:].reshape(-1)
    has = targets != -100
    ref = -torch.log_softmax(logits.double(), -1).gather(1, targets.clamp(min=0)[:, None])[:, 0]
    rows32 = F.cross_entropy(logits.float(), targets, ignore_index=-100, reduction="none")
    e_torch = float((rows32.double() - ref)[has].abs().max())
    row_bound = 2 * e_torch + 4 * 2.0 ** -24 * (logits.double().amax(-1).abs() + math.log(96))
    L = float(ref[has].mean())
    bound = e_torch + float(row_bound[has].mean()) + 2 * logits.shape[0] * 2.0 ** -24 * L
    diff = abs(float(want.loss) - float(chain.loss))
    print(f"fused loss {float(want.loss):.7f}, torch chain {float(chain.loss):.7f}, fp64 {L:.9f}: "
          f"|diff| {diff:.3e} <= {bound:.3e}")
    assert diff <= bound
    assert abs(float(want.loss) - L) <= float(row_bound[has].mean()) + logits.shape[0] * 2.0 ** -24 * L


def test_hip_equals_oracle_on_the_same_forward():
    """Table, stage-1 losses and every pruned weight bit for bit; the stage-2 column statistics are
    handed over under rtol 1e-5 (oracle_backend.OracleKernelsK6Synced says why)."""
    from ecoflap_amd import hip
    from oracle_backend import OracleKernelsK6Synced
    a = run()
    torch.cuda.empty_cache()
    checker = OracleKernelsK6Synced(hip.HipKernels())
    b = run(checker)
    assert list(a["table"]) == [f"{n}" for n in a["names"]] and len(a["table"]) == 14
    assert a["table"] == b["table"] and len(set(a["table"].values())) > 1
    assert max(a["table"].values()) <= 0.7 + 1e-9
    assert np.array_equal(a["losses"], b["losses"])
    assert checker.k6_calls > 0
    bad = [n for n in a["after"] if not torch.equal(a["after"][n], b["after"][n])]
    assert not bad, f"{len(bad)} parameters differ: {bad[:4]}"
    # every pruned row has exactly int(cols * s) zeros; what is not prunable is untouched
    for n in a["names"]:
        w = a["after"][n]
        want = int(w.shape[1] * a["table"][n])
        zeros = (w == 0).sum(1)
        assert bool((zeros == want).all()), (n, want, zeros.min().item(), zeros.max().item())
    for n in a["after"]:
        if n not in a["names"]:
            assert torch.equal(a["after"][n], a["before"][n]), n


def test_staged_batched_graph_run_equals_the_plain_closure(monkeypatch):
    plain = run(prefix_cache=False)
    torch.cuda.empty_cache()
    monkeypatch.setenv("ECOFLAP_VERIFY_BATCHED", "1")       # every chunk of the batched path checked bit for bit
    staged = run(use_graphs=True, eval_batch=16)
    assert staged["table"] == plain["table"]
    assert np.array_equal(staged["losses"], plain["losses"])
    assert staged["hashes"] == plain["hashes"]
    sf = staged["stats"]["stage1"]["suffix_forward"]
    print("suffix_forward:", sf)
    assert sf["graph_replays"] > 0 and sf["stage_calls"] < sf["stage_calls_full"]
    assert "suffix_forward" not in plain["stats"]["stage1"]
