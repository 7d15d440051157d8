"""GPU: `clip_sparsegpt_pruner` end to end at ViT-B/16's true widths (one block per tower, 4
calibration batches of 16: both towers see more tokens than any Hessian has columns), in the two
configurations of CoOp/scripts/coop/ecoflap_sparsegpt.py: the HIP kernels against the oracle's
arithmetic on the same GPU forward, a second run in the same process, the attention calls a hooked
block makes, and the MFMA Hessians of operands taken as they lie against fp64."""
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
    "sparsegpt": dict(sparsity_ratio_granularity=None),
    "ecoflap": dict(sparsity_ratio_granularity="block", max_sparsity_per_layer=0.5,
                    score_method="MEZO-GradOnly_sum"),
}
BATCHES, BATCH, CLASSES = 4, 16, 100
VISUAL, TEXT = (197, BATCH, 2304), (77, BATCH, 1536)


def _setup():
    from ecoflap_amd.shapes import clip as C
    torch.manual_seed(31)
    model = C.clip_slice(1, 1, fp16=True).eval().cuda()
    g = torch.Generator().manual_seed(32)
    prompts = torch.randint(1, 49000, (CLASSES, 77), generator=g)
    prompts[torch.arange(CLASSES), torch.randint(5, 77, (CLASSES,), generator=g)] = 49407
    loader = [{"img": torch.randn(BATCH, 3, 224, 224, generator=g).cuda(),
               "label": torch.randperm(CLASSES, generator=g)[:BATCH].cuda()} for _ in range(BATCHES)]
    return model, loader, prompts.cuda()


def _prunable(model):
    return [(n, p) for n, p in model.named_parameters() if p.dim() == 2 and ".resblocks" in n]


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def run(config, kernels=None, **attrs):
    from ecoflap_amd import load_pruner
    from ecoflap_amd.pruners.losses import clip_contrastive
    model, loader, prompts = _setup()
    np.random.seed(42)
    torch.manual_seed(42)
    cfg = dict(visual_prune_spec="1-0.6-1-1", language_prune_spec="1-0.6-1-1", language_pruning_method="none",
               visual_pruning_method="none", num_samples=BATCHES * BATCH, num_data_first_stage=32,
               **CONFIGS[config])
    if kernels is not None:
        cfg["kernels"] = kernels
    pruner = load_pruner("clip_sparsegpt_pruner", model, loader, cfg=cfg)
    for k, v in attrs.items():
        setattr(pruner, k, v)
    pruner.forward_to_cache = clip_contrastive(prompts)
    model, table = pruner.prune()
    torch.cuda.synchronize()
    weights = {n: p.detach().cpu() for n, p in _prunable(model)}
    losses = None if getattr(pruner, "last_loss_table", None) is None else np.array(pruner.last_loss_table)
    return dict(table=table, weights=weights, hashes={n: _sha(w) for n, w in weights.items()},
                losses=losses, stats=dict(pruner.stage_stats))


@pytest.mark.parametrize("config", list(CONFIGS))
def test_hip_equals_oracle_on_the_same_forward(config, monkeypatch):
    """Table, losses and every pruned weight bit for bit.  Both sides reduce the Hessians by the
    reference's fp32 expression, factor with the library and take the per-step sweep with the
    library GEMM (as the SparseGPT parity tests of the other pruners pin them): what differs is
    who runs stage 1's kernels and the block step."""
    from ecoflap_amd import hip
    from ecoflap_amd.pruners.sparsegpt import SparseGPT
    from oracle_backend import OracleKernelsK6Synced
    monkeypatch.setattr(SparseGPT, "use_mfma_hessian", False)
    monkeypatch.setattr(SparseGPT, "use_own_cholesky", False)
    a = run(config, whole_matrix_sweep=False)
    torch.cuda.empty_cache()
    b = run(config, OracleKernelsK6Synced(hip.HipKernels()), whole_matrix_sweep=False)
    if config == "sparsegpt":
        assert a["table"] is None and b["table"] is None
    else:
        assert a["table"] == b["table"] and len(set(a["table"].values())) > 1
        assert max(a["table"].values()) <= 0.5 + 1e-9
        assert np.array_equal(a["losses"], b["losses"])
    bad = [n for n in a["weights"] if not torch.equal(a["weights"][n], b["weights"][n])]
    assert not bad, f"{len(bad)} of {len(a['weights'])} pruned matrices differ: {bad[:4]}"
    assert all(int((w == 0).sum()) > 0 for w in a["weights"].values())


@pytest.mark.parametrize("config", list(CONFIGS))
def test_default_configuration_is_repeatable_and_meets_its_table(config):
    """MFMA Hessians, own factorisations, the one-call sweep: twice in one process, equal hashes;
    every matrix within 0.01 of the sparsity its table entry (or the uniform ratio) asks for."""
    first = run(config)
    again = run(config)
    assert first["table"] == again["table"]
    assert first["hashes"] == again["hashes"]
    assert len(first["weights"]) == 8
    for n, w in first["weights"].items():
        want = 0.4 if first["table"] is None else first["table"][n]
        got = float((w == 0).float().mean())
        print(f"{config} {n}: sparsity {got:.4f} (table {want:.4f})")
        assert abs(got - want) < 0.01, (n, got, want)


def test_attention_calls_of_the_hooked_passes(monkeypatch):
    """The visual tower's hooked forward issues no attention call of its own for the out-projection's
    operand (it is the block's output); the text tower's issues exactly one more, unmasked, beside the
    causal one.  With ECOFLAP_NO_FUSED_ATTENTION=1 the torch chain is taken and the run completes."""
    from ecoflap_amd.shapes import fused
    real, calls = fused.mha_attention, []

    def spy(qkv, heads, scale, causal=False, seq_first=True):
        res = real(qkv, heads, scale, causal=causal, seq_first=seq_first)
        calls.append((tuple(qkv.shape), bool(causal), res is not None))
        return res

    monkeypatch.setattr(fused, "mha_attention", spy)
    a = run("sparsegpt")
    v, tc, tn = (VISUAL, False, True), (TEXT, True, True), (TEXT, False, True)
    # visual tower: hooked pass, pass after pruning; text tower: its capture runs the visual tower,
    # then the hooked pass (causal forward + the unmasked operand), then the pass after pruning
    assert calls == [v] * BATCHES + [v] * BATCHES + [v] * BATCHES + [tc, tn] * BATCHES + [tc] * BATCHES
    assert a["stats"]["attention_operand_calls"] == 2 * BATCHES
    del calls[:]
    monkeypatch.setenv("ECOFLAP_NO_FUSED_ATTENTION", "1")
    b = run("sparsegpt")
    assert calls and not any(c[-1] for c in calls)            # asked and refused, every time
    assert b["stats"]["attention_operand_calls"] == 0
    for n, w in b["weights"].items():
        assert abs(float((w == 0).float().mean()) - 0.4) < 0.01, n


def test_mfma_hessians_of_operands_as_they_lie_against_fp64(monkeypatch):
    """Every Hessian of the visual and of the text block, reduced by the MFMA SYRK from `[L, N, C]`
    operands as they lie, against (2 / n) X^T X in fp64: within 1e-5 of the Hessian's largest entry
    (DESIGN §2), and the rows really were taken without the permuting copy."""
    from ecoflap_amd.pruners.sparsegpt import SparseGPT
    rows, hessians = {}, []
    real_add, real_factor = SparseGPT.add_rows, SparseGPT.factor_all.__func__

    def add_rows(self, x, tmp):
        assert x.dtype == torch.float16 and x.is_contiguous()
        rows.setdefault(id(self), []).append((x.clone(), int(tmp), x.shape[0]))
        return real_add(self, x, tmp)

    def factor_all(cls, items, percdamp=.01):
        for it in items:
            it.flush()
            hessians.append((id(it), it.H.clone(), it))
        return real_factor(cls, items, percdamp)

    monkeypatch.setattr(SparseGPT, "add_rows", add_rows)
    monkeypatch.setattr(SparseGPT, "factor_all", classmethod(factor_all))
    run("sparsegpt")
    assert len(hessians) == 8
    for key, H, _ in hessians:
        xs = rows[key]
        n = sum(t for _, t, _ in xs)
        assert n == BATCHES * BATCH and all(t == BATCH and r in (BATCH * 197, BATCH * 77) for _, t, r in xs)
        exact = torch.zeros(H.shape, dtype=torch.float64, device="cuda")
        for x, _, _ in xs:
            xd = x.double()
            exact += xd.t() @ xd
        exact *= 2.0 / n
        rel = float((H.double() - exact).abs().max() / exact.abs().max())
        print(f"Hessian {tuple(H.shape)}: max |H - fp64| / max |H| = {rel:.2e}")
        assert rel <= 1e-5
