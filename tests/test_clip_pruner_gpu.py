"""GPU: `clip_wanda_pruner` end to end at ViT-B/16's true widths (`clip_slice(2, 2)` in fp16, 4
calibration batches of 16), in the launcher's two configurations (CoOp/scripts/coop/
ecoflap_wanda.py: uniform Wanda at keep 0.6; ECoFLaP with `block` granularity, cap 0.5,
MEZO-GradOnly_sum): the HIP kernels against the oracle's arithmetic on the same GPU forward, the
two K1 launch forms, a second run in the same process, and the attention-kernel statistic against
the torch chain."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = {
    "wanda": dict(sparsity_ratio_granularity=None, score_method="obd_avg"),
    "ecoflap": dict(sparsity_ratio_granularity="block", max_sparsity_per_layer=0.5,
                    score_method="MEZO-GradOnly_sum"),
}
BATCHES, BATCH, CLASSES = 4, 16, 100


def _setup():
    from ecoflap_amd.shapes import clip as C
    torch.manual_seed(11)
    model = C.clip_slice(2, 2, fp16=True).eval().cuda()
    g = torch.Generator().manual_seed(12)
    prompts = torch.randint(1, 49000, (CLASSES, 77), generator=g)
    prompts[torch.arange(CLASSES), torch.randint(5, 77, (CLASSES,), generator=g)] = 49407
    loader = [{"img": torch.randn(BATCH, 3, 224, 224, generator=g).cuda(),
               "label": torch.randperm(CLASSES, generator=g)[:BATCH].cuda()} for _ in range(BATCHES)]
    return model, loader, prompts.cuda()


def _prunable(model):
    return [(n, p) for n, p in model.named_parameters() if p.dim() == 2 and ".resblocks" in n]


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def run(config, kernels=None, **extra):
    from ecoflap_amd import load_pruner
    from ecoflap_amd.pruners.losses import clip_contrastive
    model, loader, prompts = _setup()
    np.random.seed(42)
    torch.manual_seed(42)
    cfg = dict(visual_prune_spec="1-0.6-1-1", language_prune_spec="1-0.6-1-1", language_pruning_method="none",
               visual_pruning_method="none", num_samples=BATCHES * BATCH, num_data_first_stage=32,
               **CONFIGS[config])
    cfg.update(extra)
    if kernels is not None:
        cfg["kernels"] = kernels
    pruner = load_pruner("clip_wanda_pruner", model, loader, cfg=cfg)
    pruner.forward_to_cache = clip_contrastive(prompts)
    model, table = pruner.prune()
    torch.cuda.synchronize()
    weights = {n: p.detach().cpu() for n, p in _prunable(model)}
    losses = None if getattr(pruner, "last_loss_table", None) is None else np.array(pruner.last_loss_table)
    return dict(table=table, weights=weights, hashes={n: _sha(w) for n, w in weights.items()},
                losses=losses, stats=dict(pruner.stage_stats))


def _synced_checker():
    from ecoflap_amd import hip
    from oracle_backend import OracleKernelsK6Synced

    class Synced(OracleKernelsK6Synced):
        """...and the fold of the attention kernel's statistic into the running mean
        (`colsq_replay`) both ways too, held to the same rtol, going on with the HIP value."""
        replays = 0

        def colsq_replay(self, scaler_row, sq, batches, nsamples_before=0):
            mine = scaler_row.clone()
            super().colsq_replay(mine, sq, batches, nsamples_before)
            self.hip.colsq_replay(scaler_row, sq, batches, nsamples_before)
            rel = ((scaler_row - mine).abs() / mine.abs().clamp_min(1e-30)).max().item()
            self.replays += 1
            self.k6_max_rel = max(self.k6_max_rel, rel)
            assert rel <= self.rtol, f"colsq_replay: HIP vs oracle differ by {rel:.3e} relative"

    return Synced(hip.HipKernels())


@pytest.mark.parametrize("config", list(CONFIGS))
def test_hip_equals_oracle_on_the_same_forward(config, monkeypatch):
    """Tables, losses, masks and every pruned weight bit for bit.  The float reductions of stage
    2 are handed over under rtol 1e-5 (oracle_backend.OracleKernelsK6Synced says why): every K6
    call, every fold of the attention kernel's statistic, and that statistic itself — in the
    oracle's run each `mha_attention_colsq` is also asked for its output, and the oracle's own
    column sums of that output are held against the kernel's."""
    from ecoflap_amd.shapes import fused
    a = run(config)
    torch.cuda.empty_cache()
    checker = _synced_checker()
    real, checked = fused.mha_attention_colsq, []

    def held(qkv, heads, scale, out=True, seq_first=True):
        y, sq = real(qkv, heads, scale, out=True, seq_first=seq_first)
        mine = torch.empty(sq.shape, dtype=torch.float32)
        checker.o.colsq_raw(mine, y.reshape(-1, y.shape[-1]).cpu().contiguous())
        rel = ((sq.cpu() - mine).abs() / mine).max().item()
        checked.append(rel)
        assert rel <= checker.rtol, rel
        return (y if out else None), sq

    monkeypatch.setattr(fused, "mha_attention_colsq", held)
    b = run(config, checker)
    monkeypatch.setattr(fused, "mha_attention_colsq", real)
    if config == "wanda":
        assert a["table"] is None and b["table"] is None
    else:
        assert a["table"] == b["table"] and len(set(a["table"].values())) > 1
        assert max(a["table"].values()) <= 0.5 + 1e-9
        assert np.array_equal(a["losses"], b["losses"])
    assert checker.k6_calls > 0 and checker.replays == len(checked) == 2 * 2 * BATCHES
    bad = [n for n in a["weights"] if not torch.equal(a["weights"][n], b["weights"][n])]
    assert not bad, f"{len(bad)} of {len(a['weights'])} pruned matrices differ: {bad[:4]}"
    zeros = {n: int((w == 0).sum()) for n, w in a["weights"].items()}
    assert all(z > 0 for z in zeros.values())
    print(f"{config}: {checker.k6_calls} K6 calls + {checker.replays} folds, max |HIP - oracle| / oracle = "
          f"{checker.k6_max_rel:.2e}; attention statistic vs oracle column sums: max rel {max(checked):.2e}")


def test_k1_forms_and_a_second_run_give_the_same_hashes():
    first = run("ecoflap", k1_form="block")
    again = run("ecoflap", k1_form="block")
    units = run("ecoflap", k1_form="units")
    assert first["table"] == again["table"] == units["table"]
    assert np.array_equal(first["losses"], again["losses"]) and np.array_equal(first["losses"], units["losses"])
    assert first["hashes"] == again["hashes"] == units["hashes"]


def test_hooked_passes_go_through_the_kernel_and_the_torch_chain_agrees(monkeypatch):
    """Both towers' hooked passes take `fused.mha_attention_colsq` (the visual tower with the
    output, the text tower without); with ECOFLAP_NO_FUSED_ATTENTION=1 the torch chain is taken,
    and the masks of the two runs agree on >= 99 % of the elements — a floor, not a measurement:
    the two paths differ by fp16 roundings of the attention (forward and statistic)."""
    from ecoflap_amd.shapes import fused
    real, calls = fused.mha_attention_colsq, []

    def spy(qkv, heads, scale, out=True, seq_first=True):
        res = real(qkv, heads, scale, out=out, seq_first=seq_first)
        calls.append((tuple(qkv.shape), heads, out, seq_first, res is not None))
        return res

    monkeypatch.setattr(fused, "mha_attention_colsq", spy)
    a = run("wanda")
    per_tower = 2 * BATCHES                       # blocks x hooked forwards
    assert calls == [((197, BATCH, 2304), 12, True, True, True)] * per_tower + \
        [((77, BATCH, 1536), 8, False, True, True)] * per_tower
    assert a["stats"]["attention_colsq_calls"] == 2 * per_tower
    del calls[:]
    monkeypatch.setenv("ECOFLAP_NO_FUSED_ATTENTION", "1")
    b = run("wanda")
    # the visual tower asks and is refused; the text tower's causal `mha_attention` is refused first,
    # so its store-free pass is never asked for; every out_proj statistic came from the torch chain
    assert [(c[0], c[-1]) for c in calls] == [((197, BATCH, 2304), False)] * per_tower
    assert b["stats"]["attention_colsq_calls"] == 0
    same = sum(int(((a["weights"][n] == 0) == (b["weights"][n] == 0)).sum()) for n in a["weights"])
    total = sum(w.numel() for w in a["weights"].values())
    worst = min((((a["weights"][n] == 0) == (b["weights"][n] == 0)).float().mean().item(), n) for n in a["weights"])
    print(f"masks, kernel statistic vs torch chain: {same / total:.5f} of {total} elements agree "
          f"(worst matrix {worst[1]}: {worst[0]:.5f})")
    assert same / total >= 0.99
