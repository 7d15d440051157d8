"""`clip_sparsegpt_pruner`: ECoFLaP / SparseGPT on the two towers of an OpenAI-CLIP model.

Host-side mirror of CoOp/trainers/pruners/sparsegpt_pruner.py:608-806 (`CLIPLayerSparseGPTPruner`)
and of the stage-2 body it borrows through `partial` from `TransformerLayerSparseGPTPruner`
(:428-526).  Registered name, constructor keywords, `prune()` contract, stage 1 and `get_sparsity`
are `clip_wanda_pruner`'s (pruners/clip.py: the reference's two classes differ in `_prune` only), so
this class inherits them and replaces stage 2.

Stage 2 per block: ONE hooked pass over the captured batches completes the four Hessians
(`SparseGPT.add_batch` with the batch count N) before anything is pruned —
  mlp.c_fc, mlp.c_proj   forward hooks, inputs permuted to `[N, L, C]` (:479);
  attn.in_proj_weight    `ln_1(x)` (`hacky_attn.qkv`, :444, :501);
  attn.out_proj.weight   the output of the reference's side attention, which has NO mask in either
                         tower (`hacky_attn.proj`, :14-106, :441-458), while the text tower's own
                         forward stays causal —
then `fasterprune(ratio, prune_n, prune_m, percdamp=0.01, blocksize=128)` per matrix in the
reference's order (:493-514), then one plain pass through the pruned block feeds the next (:519-522).
The two attention operands come from the block (`shapes/clip.py::ResidualAttentionBlock._stat_sink`):
on the GPU in fp16 the out-projection's is the output of `fused.mha_attention(causal=False)` — the
block's own call in the visual tower, one extra call in the text tower — everywhere else the torch
chain `_side_attention`.

Row order.  On the CPU an operand is flattened in the reference's `[N, L]` order: the fp32 Hessian
is bit for bit the reference's.  On the GPU the `[L, N, C]` tensors go to the Hessian update as they
lie — a Hessian is a sum over rows and does not depend on their order beyond rounding — so no
permuting copy is made.

The column sweep of every matrix is ONE host call (`SparseGPT.whole_matrix_sweep`,
`ecoflap_sparsegpt_matrix`) where the backend has it.

`transformer_sparsegpt_pruner` is not registered: like its Wanda sibling the reference class cannot
run on its own.
"""
import time

import torch
import torch.nn as nn

from ..registry import registry
from .base_pruner import print_time
from .clip import CLIPLayerWandaPruner
from .phase_timer import PhaseTimer
from .sparsegpt import SparseGPT
from .wanda import _BlockwiseWanda, find_layers, get_module_recursive


def _in_projection(attn):
    """The packed in-projection of an nn.MultiheadAttention as the `nn.Linear` `SparseGPT` wants
    (the reference's `hacky_attn.qkv`): it shares the Parameter, so the pruned weight needs no
    writing back.  Built on the meta device: no allocation, no draw from torch's generator."""
    lin = nn.Linear(1, 1, bias=False, device="meta")
    lin.in_features, lin.out_features = attn.in_proj_weight.shape[1], attn.in_proj_weight.shape[0]
    lin.weight = attn.in_proj_weight
    return lin


class _HessianSites:
    """What a hooked block reports to (`ResidualAttentionBlock._stat_sink`) under SparseGPT."""

    def __init__(self, wrapped):
        self.wrapped = wrapped
        self.kernel_operands = 0        # out_proj operands that came from the attention kernel

    def takes_statistic(self):
        return False

    def takes_kernel_operand(self):
        return True

    def operand(self, name, x_nlc):
        if name == "attn.out_proj" and x_nlc.is_cuda and not x_nlc.is_contiguous():
            self.kernel_operands += 1
        add_operand(self.wrapped[name], x_nlc.data)


def add_operand(sgpt, x_nlc):
    """`[N, L, C]` operand -> Hessian.  A GPU operand that is a permuted view of a contiguous
    `[L, N, C]` tensor is reduced as it lies (see the module's note on row order)."""
    n = x_nlc.shape[0]
    if x_nlc.is_cuda and x_nlc.dim() == 3 and not x_nlc.is_contiguous():
        lnc = x_nlc.permute(1, 0, 2)
        if lnc.is_contiguous():
            sgpt.add_rows(lnc.reshape(-1, lnc.shape[-1]), n)
            return
    sgpt.add_batch(x_nlc, None)


class _ClipBlockwiseSparseGPT(_BlockwiseWanda):
    """Stage 2 over one tower's `resblocks`."""

    # (name in `wrapped`, sparsity-table leaf) in the order `find_layers` walks the reference's
    # block: mlp.c_fc, mlp.c_proj, then hacky_attn.qkv, hacky_attn.proj (:463, :493-505)
    SITES = (("mlp.c_fc", "mlp.c_fc.weight"), ("mlp.c_proj", "mlp.c_proj.weight"),
             ("attn.in_proj", "attn.in_proj_weight"), ("attn.out_proj", "attn.out_proj.weight"))

    def run_tower(self, model, dataloader, device, module_to_process, n_samples, sparsity_ratio):
        t0 = time.time()
        try:
            return self._run_tower(model, dataloader, device, module_to_process, n_samples, sparsity_ratio)
        finally:
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            self.owner.stage_stats.setdefault("stage2", {})[module_to_process] = time.time() - t0

    def _run_tower(self, model, dataloader, device, module_to_process, n_samples, sparsity_ratio):
        owner = self.owner
        blocks = get_module_recursive(model, module_to_process)
        # the capture runs the WHOLE closure (:413-420): the text tower's runs the already pruned
        # visual tower first; samples are counted by batch["img"]
        with torch.no_grad():
            inps, outs, _ = self.capture(
                model, dataloader, blocks, lambda m, b: owner.forward_to_cache(m, b, device), [],
                n_samples, batch_len=lambda b: b["img"].shape[0])
        n_batches = min(n_samples, len(inps))     # (:433: a sample count against a batch count, as written)
        stats = owner.stage_stats
        for i in range(len(blocks)):
            block = blocks[i]
            subset = find_layers(block)           # mlp.c_fc, mlp.c_proj
            layers = dict(subset)
            layers["attn.in_proj"] = _in_projection(block.attn)
            layers["attn.out_proj"] = block.attn.out_proj
            wrapped = {name: SparseGPT(layers[name], kernels=self.kernels) for name in layers}
            for w_ in wrapped.values():
                w_.whole_matrix_sweep = bool(getattr(owner, "whole_matrix_sweep", True))
                w_.literal_update = True
            handles = [
                subset[name].register_forward_hook(       # permuted for the NLD shape (:479)
                    lambda _m, inp, out, _n=name: add_operand(wrapped[_n], inp[0].permute(1, 0, 2).data))
                for name in subset
            ]
            sites = _HessianSites(wrapped)
            block._stat_sink = sites
            try:
                with PhaseTimer.span("stage2.block_forward_with_hooks (incl. Hessian updates)"):
                    for j in range(n_batches):
                        with torch.no_grad():
                            block(inps[j])
                    for w_ in wrapped.values():
                        w_.flush()                # buffered calibration batches -> H
            finally:
                del block._stat_sink
                for h in handles:
                    h.remove()
            stats["attention_operand_calls"] = stats.get("attention_operand_calls", 0) + sites.kernel_operands
            self._merge_hessians(wrapped)
            with PhaseTimer.span("sparsegpt.factor (all Linears of a block: csrc/cholesky.hip)"):
                SparseGPT.factor_all([wrapped[name] for name, _ in self.SITES], percdamp=0.01)
            for name, leaf in self.SITES:
                assert wrapped[name].nsamples == len(inps) * inps[0].shape[1]      # (:494)
                wrapped[name].fasterprune(sparsity_ratio[f"{module_to_process}.{i}.{leaf}"],
                                          prune_n=owner.prune_n, prune_m=owner.prune_m,
                                          percdamp=0.01, blocksize=128)                # (:507)
                wrapped[name].H = wrapped[name].factor = None      # (`free()` without the cache flush per matrix)
            with PhaseTimer.span("stage2.block_forward_after_prune"):
                for j in range(n_batches):            # the pruned block feeds the next one (:519-522)
                    with torch.no_grad():
                        outs[j] = block(inps[j])
            inps, outs = outs, inps
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
        return model


@registry.register_pruner("clip_sparsegpt_pruner")
class CLIPLayerSparseGPTPruner(CLIPLayerWandaPruner):
    pruner_name = "clip_sparsegpt_pruner"
    whole_matrix_sweep = True       # the column sweep of a matrix in one host call (pruners/sparsegpt.py)

    @print_time
    def _prune(self, model, dataloader, device, model_prefix, module_to_process, n_samples=64,
               sparsity_ratio=0.5):
        return _ClipBlockwiseSparseGPT(self).run_tower(model, dataloader, device, module_to_process,
                                                       n_samples, sparsity_ratio)
