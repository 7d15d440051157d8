"""Stage 2's grouped block passes (`pruners/wanda.py`, `stage2_group`): batch-1 calibration
samples ride G = 8 to one replayed HIP graph of the block, and the slot guard holds every slot to
the bits that sample gets alone (all slots of a block's first group, the rotating slot
(3 g + 1) mod G of each later group g, against batch-1 replays of the block).

At the true widths (`blip2_width_slice`: ViT-g blocks 1408 / 6144 in fp16, FlanT5-XL blocks
2048 / 5120 in bf16 with the position bias and mask in the caches), where no tensor is small
enough for `verify_all`, each run is compared with the same run at `stage2_group = 1`, bit for bit,
in every Hessian as it reaches `SparseGPT.factor_all`, every Wanda column statistic as it reaches
`wanda_prune_block`, every block's input and the pruned state_dict:

  clean                 grouped == one replay per sample;
  slot 3 shifted        one 16-bit ulp on slot 3 of ViT block 0's fc1 output, only when the block
                        runs G stacked samples: the guard catches it in the first group;
  shift from group 2    the same shift gated by a counter on the device that the captured graph
                        advances: only the rotating slot can reach it.

At the toy size (`verify_all` on) a failed check in block 0's hooked pass turns grouping off for
the rest of the part."""
import copy
import sys

import pytest
import torch

from ecoflap_amd import hip, load_pruner
from ecoflap_amd.pruners import wanda as W
from ecoflap_amd.pruners.sparsegpt import SparseGPT
from ecoflap_amd.shapes import synthetic as S

pytestmark = pytest.mark.gpu

G = 8
VIT = "visual_encoder.blocks"
PARTS = (VIT, "t5_model.encoder.block", "t5_model.decoder.block")
PRUNERS = ("blipt5_sparsegpt_pruner", "blipt5_wanda_pruner")
N_CLEAN = 5 * G + 3                 # whole groups and a ragged tail
N_LATE = (2 + G) * G                # the rotating slot reaches every slot from group 2 on


class SlotShift:
    """Forward hook on a Linear of one ViT block: one 16-bit ulp added to slot `slot`'s rows of
    its output, only when the block runs G stacked samples.  The shift is captured into the
    block's graph behind a counter on the device that the graph advances: replays 0 .. start-1 of
    a grouped pass are left alone, the later ones shifted.  The eager warm-up ahead of each
    capture resets the counter (its output is thrown away).  `passes`: act in the first `passes`
    grouped passes only (a warm-up and a capture each).  `stacked_calls` counts every stacked
    forward the hook sees, acting or not."""

    def __init__(self, start=0, passes=None, slot=3):
        self.start, self.slot, self.passes = start, slot, passes
        self.count = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.stacked_calls = 0
        self.captures = 0

    def __call__(self, module, inp, out):
        if out.shape[0] != G:
            return None
        self.stacked_calls += 1
        if self.passes is not None and self.stacked_calls > 2 * self.passes:
            return None
        if not torch.cuda.is_current_stream_capturing():
            self.count.zero_()
            return None
        self.captures += 1
        self.count.add_(1)
        y = out.clone()
        y[self.slot].view(torch.int16).add_((self.count > self.start).to(torch.int16))
        return y


def _recording(monkeypatch):
    """What reaches the selection, block by block: SparseGPT's Hessians before `factor_all`,
    Wanda's column statistics as handed to `wanda_prune_block`, and every block's input (all
    calibration samples, read from stage 2's loop where it looks up the block's Linears)."""
    rec = {"stat": [], "inputs": []}
    factor_all = SparseGPT.factor_all.__func__
    prune_block = hip.HipKernels.wanda_prune_block
    find_layers = W.find_layers

    def recording_factor_all(cls, items, percdamp=.01):
        rec["stat"].append([w.H.clone() for w in items])
        return factor_all(cls, items, percdamp)

    def recording_prune_block(self, items):
        rec["stat"].append([it[1].clone() for it in items])
        return prune_block(self, items)

    def recording_find_layers(module, *a, **kw):
        f = sys._getframe(1)
        if f.f_code.co_name == "_run" and "inps" in f.f_locals:
            rec["inputs"].append(torch.cat(list(f.f_locals["inps"]), 0))
        return find_layers(module, *a, **kw)

    monkeypatch.setattr(SparseGPT, "factor_all", classmethod(recording_factor_all))
    monkeypatch.setattr(hip.HipKernels, "wanda_prune_block", recording_prune_block)
    monkeypatch.setattr(W, "find_layers", recording_find_layers)
    return rec


def _run(monkeypatch, template, name, n, group, hooks=(), toy=False):
    """One prune of a copy of `template` (uniform sparsity: no stage 1) with `hooks`
    [(module path, hook)] installed -> (record, pruned state_dict, stage_stats, pruner)."""
    model = copy.deepcopy(template)
    handles = [model.get_submodule(path).register_forward_hook(h) for path, h in hooks]
    if toy:
        batches = S.image_text_batches(n, 1, img_size=28, vocab=96, in_len=5, out_len=4, seed=6,
                                       device="cuda")
    else:
        batches = S.image_text_batches(n, 1, img_size=224, vocab=32128, in_len=16, out_len=16,
                                       seed=6, device="cuda")
    cfg = dict(t5_prune_spec="2-0.5-1.0-1.0", vit_prune_spec="2-0.5-1.0-1.0",
               t5_pruning_method="none", vit_pruning_method="none", num_samples=n,
               kernels=hip.HipKernels())
    with monkeypatch.context() as m:
        rec = _recording(m)
        pruner = load_pruner(name, model, batches, cfg=cfg)
        pruner.graph_min_batches = 4
        pruner.stage2_group = group
        model, _ = pruner.prune()
        torch.cuda.synchronize()
    for h in handles:
        h.remove()
    return rec, {k: v.detach().clone() for k, v in model.state_dict().items()}, pruner.stage_stats, pruner


def _assert_same(got, want, what):
    rec_a, sd_a = got[0], got[1]
    rec_b, sd_b = want[0], want[1]
    assert len(rec_a["inputs"]) == len(rec_b["inputs"]) == 6, what
    for bi, (a, b) in enumerate(zip(rec_a["inputs"], rec_b["inputs"])):
        assert torch.equal(a, b), f"{what}: the input of block {bi} (in part order) differs"
    assert len(rec_a["stat"]) == len(rec_b["stat"]) == 6, what
    for bi, (a, b) in enumerate(zip(rec_a["stat"], rec_b["stat"])):
        assert len(a) == len(b), what
        bad = [li for li, (x, y) in enumerate(zip(a, b)) if not torch.equal(x, y)]
        assert not bad, f"{what}: block {bi}'s statistics of Linears {bad} differ"
    bad = [k for k in sd_b if not torch.equal(sd_a[k], sd_b[k])]
    assert not bad, f"{what}: pruned weights differ: {bad[:4]}"


@pytest.fixture(scope="module")
def width_slice():
    from ecoflap_amd.shapes.blip2_t5 import blip2_width_slice
    torch.manual_seed(31)
    return blip2_width_slice().eval().to("cuda")


@pytest.fixture(scope="module")
def ungrouped(width_slice):
    """stage2_group = 1 runs, one per (pruner, calibration samples), shared by the tests below
    (the hooks only act on stacked forwards, so they leave these runs alone)."""
    cache = {}

    def get(monkeypatch, name, n):
        if (name, n) not in cache:
            hook = SlotShift()
            cache[(name, n)] = _run(monkeypatch, width_slice, name, n, 1,
                                    hooks=[(VIT + ".0.mlp.fc1", hook)])
            assert hook.stacked_calls == 0
            assert cache[(name, n)][2].get("stage2_grouped_passes", 0) == 0
        return cache[(name, n)]
    yield get
    cache.clear()


def _grouped_passes_expected(name):
    return 2 if name == "blipt5_sparsegpt_pruner" else 1      # Wanda's hooked pass stays per sample


@pytest.mark.parametrize("name", PRUNERS)
def test_grouped_passes_at_true_width_equal_one_replay_per_sample(monkeypatch, width_slice, ungrouped, name):
    got = _run(monkeypatch, width_slice, name, N_CLEAN, G)
    want = ungrouped(monkeypatch, name, N_CLEAN)
    _, _, stats, pruner = got
    # no tensor of these blocks is small enough for `verify_all` (the smallest compared, a block
    # output, is the size of its input): the guard's rotation is what runs
    min_values = int(getattr(pruner, "stage2_group_min_values", 65536))     # (stage 2's default)
    for x in got[0]["inputs"]:
        assert x.shape[0] == N_CLEAN
        assert 2 * x[0].numel() >= min_values, tuple(x.shape)
    _assert_same(got, want, f"{name} grouped vs one replay per sample")
    per = _grouped_passes_expected(name)
    assert stats["stage2_grouped_passes"] == 6 * per, stats.get("stage2_group_guard")
    n_full = N_CLEAN // G
    for part in PARTS:
        rec = stats["stage2_group_guard"][part]
        assert rec == {"grouped_passes": 2 * per, "slot_checks": 2 * per * (G + n_full - 1),
                       "fell_back": None}, (part, rec)


@pytest.mark.parametrize("name", PRUNERS)
@pytest.mark.parametrize("start", [0, 2], ids=["slot3", "slot3_from_group2"])
def test_slot_dependent_deviation_is_caught(monkeypatch, width_slice, ungrouped, name, start):
    n = N_CLEAN if start == 0 else N_LATE
    hook = SlotShift(start=start)
    got = _run(monkeypatch, width_slice, name, n, G, hooks=[(VIT + ".0.mlp.fc1", hook)])
    assert hook.captures >= 1, "the shift was never captured into a grouped replay"
    _assert_same(got, ungrouped(monkeypatch, name, n), f"{name}, slot 3 shifted from group {start}")
    stats = got[2]
    which = "hooked" if name == "blipt5_sparsegpt_pruner" else "plain"
    assert stats["stage2_group_guard"][VIT]["fell_back"] == f"block 0, {which} pass", stats["stage2_group_guard"]
    assert stats["stage2_group_guard"][VIT]["grouped_passes"] == 0
    per = _grouped_passes_expected(name)
    for part in PARTS[1:]:
        assert stats["stage2_group_guard"][part]["fell_back"] is None, part
        assert stats["stage2_group_guard"][part]["grouped_passes"] == 2 * per, part


def test_failed_check_turns_grouping_off_for_the_part(monkeypatch):
    """Toy size (`verify_all`: every slot of every group is compared): a shift of slot 3 from
    group 2 on, in block 0's hooked pass only.  Block 0 runs again one replay per sample, and no
    later block of the ViT part groups — neither block 0's pass after the prune, whose own check
    would pass, nor block 1."""
    from ecoflap_amd.shapes.blip2_t5 import blip2_toy
    torch.manual_seed(4)
    template = blip2_toy(fp32=False).eval().to("cuda")
    name, n = "blipt5_sparsegpt_pruner", 4 * G + 3
    shift, later = SlotShift(start=2, passes=1), SlotShift(passes=0)
    got = _run(monkeypatch, template, name, n, G, toy=True,
               hooks=[(VIT + ".0.mlp.fc1", shift), (VIT + ".1.mlp.fc1", later)])
    want = _run(monkeypatch, template, name, n, 1, toy=True)
    assert shift.captures == 1
    assert shift.stacked_calls == 2, "block 0's pass after the prune grouped after a failed check"
    assert later.stacked_calls == 0, "block 1 grouped after a failed check in block 0"
    _assert_same(got, want, "toy, slot 3 shifted from group 2 in block 0's hooked pass")
    guard = got[2]["stage2_group_guard"]
    assert guard[VIT]["fell_back"] == "block 0, hooked pass", guard
    assert guard[VIT]["grouped_passes"] == 0
    assert got[2]["stage2_grouped_passes"] == sum(r["grouped_passes"] for r in guard.values())
