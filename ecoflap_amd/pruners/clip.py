"""`clip_wanda_pruner`: ECoFLaP / Wanda on the two towers of an OpenAI-CLIP model.

Host-side mirror of CoOp/trainers/pruners/wanda_pruner.py:483-681 (`CLIPLayerWandaPruner`) and of
the stage-2 body it borrows through `partial` from `TransformerLayerWandaPruner` (:247-401): same
registered name, constructor keywords, `prune()` contract (`-> (model, table_or_None)`, visual
tower first, weights pruned in place) and sparsity-table keys.  `forward_to_cache(model, batch,
device)` is assigned onto the instance from outside, as CoOp/trainers/zsclip.py:73-93 does
(`pruners/losses.py::clip_contrastive` builds it); batches are `{"img", "label"}`.

What stage 2 reduces per block (all four operands as `[N, L, C]`, `WrappedGPT.add_batch` with the
batch count N):
  mlp.c_fc, mlp.c_proj   forward hooks on the two `nn.Linear`s `find_layers` finds (`attn.out_proj`
                         is a `NonDynamicallyQuantizableLinear` and is not found);
  attn.in_proj_weight    `ln_1(x)`;
  attn.out_proj.weight   the output of the reference's side copy of the attention, which has NO
                         mask in either tower (wanda_pruner.py:300-322): the text tower's out_proj
                         is pruned on the column norms of the unmasked attention while the
                         block's own forward stays causal.
The last two come from the block itself (`shapes/clip.py::ResidualAttentionBlock._stat_sink`); on
the GPU in fp16 the out_proj statistic is the epilogue of the attention kernel
(`ecoflap_mha_attention_colsq`), folded into the running mean by `ecoflap_colsq_replay` — the
roundings of every other site.  Selection is K7's rows mode (:379-383).

`transformer_wanda_pruner` is not registered: the reference class cannot run on its own.
"""
import time

import torch

from ..registry import registry
from .base_pruner import LayerWiseBasePruner, print_time
from .wanda import (WrappedGPT, _BlockwiseWanda, _K6Collector, _StageOneMixin, find_layers,
                    get_module_recursive)


class _ClipLoss:
    """The closure stage 1 calls as `(model, batch, cuda_enabled)`: CoOp's `LayerSparsity` hands the
    model's device, not a flag, as the third argument (layer_single_base_pruner.py:526); adapted
    here, where the pruner knows it.  `stage_of` names the (tower, resblock) a parameter belongs
    to: `k1_form="block"` then perturbs a transformer block's four matrices in one K1 launch."""

    def __init__(self, owner):
        self.owner = owner

    def __call__(self, model, batch, cuda_enabled):
        return self.owner.forward_to_cache(model, batch, next(iter(model.parameters())).device)

    @staticmethod
    def stage_of(name):
        parts = name.split(".")
        if "resblocks" not in parts:
            return None
        return ".".join(parts[:parts.index("resblocks") + 2])


class _InProjection:
    """`WrappedGPT` wants a layer with a `.weight`: the packed in-projection of an
    nn.MultiheadAttention is a bare parameter."""

    def __init__(self, attn):
        self.weight = attn.in_proj_weight


class _AttentionSites:
    """What a hooked block reports to (`ResidualAttentionBlock._stat_sink`)."""

    def __init__(self, wrapped, kernels, collector):
        self.wrapped, self.kernels, self.collector = wrapped, kernels, collector
        self.kernel_statistics = 0      # out_proj statistics that came from the attention kernel

    def takes_statistic(self):
        # (a backend without the replay takes the operand instead)
        return hasattr(self.kernels, "colsq_replay")

    def operand(self, name, x_nlc):
        self.wrapped[name].add_batch(x_nlc.data, None)

    def statistic(self, name, sq, batch):
        w_ = self.wrapped[name]
        self.kernel_statistics += 1
        if self.collector is not None and self.collector.raw:
            # data parallel: the batch's own statistic is kept apart, as every other site's, and
            # replayed in global batch order by `merge()` — the one-process scaler_row bit for bit
            self.collector.add_statistic(w_, sq, int(batch))
            return
        self.kernels.colsq_replay(w_.scaler_row, sq.view(1, -1), [int(batch)], w_.nsamples)
        w_.nsamples += int(batch)


class _ClipBlockwiseWanda(_BlockwiseWanda):
    """Stage 2 over one tower's `resblocks` (an `nn.Sequential` of `[L, N, D]` blocks)."""

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
        # the Catcher on resblocks[0] is driven by the WHOLE closure (:271-282): the text tower's
        # capture runs the already pruned visual tower first; samples are counted by batch["img"]
        with torch.no_grad():
            inps, outs, _ = self.capture(
                model, dataloader, blocks, lambda m, b: owner.forward_to_cache(m, b, device), [],
                n_samples, batch_len=lambda b: b["img"].shape[0])
        n_batches = min(n_samples, len(inps))     # (:294: a sample count against a batch count, as written)
        _, world = self._rank_world()
        for i in range(len(blocks)):
            block = blocks[i]
            subset = find_layers(block)           # mlp.c_fc, mlp.c_proj
            layers = dict(subset)
            layers["attn.in_proj"] = _InProjection(block.attn)
            layers["attn.out_proj"] = block.attn.out_proj
            wrapped = {name: WrappedGPT(layers[name], kernels=self.kernels) for name in layers}
            handles = [
                subset[name].register_forward_hook(       # permuted for the NLD shape (:340)
                    lambda _m, inp, out, _n=name: wrapped[_n].add_batch(inp[0].permute(1, 0, 2).data, out.data))
                for name in subset
            ]
            collector = None
            if hasattr(self.kernels, "colsqnorm_accum_multi"):
                collector = _K6Collector(
                    self.kernels, raw=world > 1 and hasattr(self.kernels, "colsq_replay"),
                    immediate=bool(getattr(owner, "k6_immediate", False)))
                for w_ in wrapped.values():
                    w_.sink = collector
            sites = _AttentionSites(wrapped, self.kernels, collector)
            block._stat_sink = sites
            try:
                for j in range(n_batches):
                    with torch.no_grad():
                        block(inps[j])
                    if collector is not None:
                        collector.flush()
                        collector.end_sample()
            finally:
                del block._stat_sink
                for h in handles:
                    h.remove()
                for w_ in wrapped.values():
                    w_.sink = None
            stats = owner.stage_stats
            stats["attention_colsq_calls"] = stats.get("attention_colsq_calls", 0) + sites.kernel_statistics
            if collector is not None:
                stats["k6_launches"] = stats.get("k6_launches", 0) + collector.launches
            if collector is not None and collector.raw:
                stats["k6_dp_exact_blocks"] = stats.get("k6_dp_exact_blocks", 0) + 1
                collector.merge(self.local_batch_ids[:n_batches], self.global_batches,
                                getattr(owner, "process_group", None))
            else:
                self._merge_statistics(wrapped)
            items = []
            for name, leaf in self.SITES:
                assert wrapped[name].nsamples == len(inps) * inps[0].shape[1]      # (:355)
                weight = layers[name].weight.data
                ratio = sparsity_ratio[f"{module_to_process}.{i}.{leaf}"]
                items.append((weight, wrapped[name].scaler_row, "rows", int(weight.shape[1] * ratio), None))
            self.kernels.wanda_prune_block(items)       # per output row, k smallest by stable order (:379-383)
            for j in range(n_batches):                  # the pruned block feeds the next one (:394-397)
                with torch.no_grad():
                    outs[j] = block(inps[j])
            inps, outs = outs, inps
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
        return model


@registry.register_pruner("clip_wanda_pruner")
class CLIPLayerWandaPruner(_StageOneMixin, LayerWiseBasePruner):
    pruner_name = "clip_wanda_pruner"

    def __init__(self, model, data_loader, language_prune_spec=None, visual_prune_spec=None,
                 language_pruning_method=None, visual_pruning_method=None,
                 language_model_prefix="transformer", visual_model_prefix="visual.transformer", **kwargs):
        kwargs.pop("prune_spec", None)
        kwargs.pop("model_prefix", None)
        super().__init__(model=model, data_loader=data_loader, prune_spec=None, model_prefix="tmp",
                         **kwargs)
        self.language_prune_spec = language_prune_spec
        self.visual_prune_spec = visual_prune_spec
        self.language_model_prefix = language_model_prefix
        self.visual_model_prefix = visual_model_prefix

    def forward_to_cache(self, model, batch, device):
        """Assigned from outside (zsclip.py:93); `losses.clip_contrastive(prompt_tokens)` builds it."""
        raise NotImplementedError("assign pruner.forward_to_cache = clip_contrastive(prompt_tokens)")

    def get_sparsity(self, original_sparsity, sparsity_ratio_granularity=None):
        if self.sparsity_dict is not None:
            return self._load_sparsity_yaml()
        lang, vis = self.language_model_prefix, self.visual_model_prefix
        if sparsity_ratio_granularity is None:
            mapping = {}
        else:
            names = [k for k, v in self.model.named_parameters()
                     if len(v.shape) == 2 and ".resblocks" in k
                     and "relative_attention_bias.weight" not in k
                     and (k.startswith(lang) or k.startswith(vis))]

            def group_of(name):
                # (the language prefix is tested first, as :559 / :578 do)
                is_lang = name.startswith(lang)
                if sparsity_ratio_granularity == "model":
                    return lang if is_lang else vis
                if sparsity_ratio_granularity == "layer":
                    return name
                if sparsity_ratio_granularity == "block":
                    return ".".join(name.split(".")[:3 if is_lang else 4])
                raise NotImplementedError

            if sparsity_ratio_granularity not in ("model", "layer", "block"):
                raise NotImplementedError
            mapping = {k: group_of(k) for k in names}
        return self._layer_sparsity(_ClipLoss(self), original_sparsity, mapping)

    @print_time
    def _prune(self, model, dataloader, device, model_prefix, module_to_process, n_samples=64,
               sparsity_ratio=0.5):
        return _ClipBlockwiseWanda(self).run_tower(model, dataloader, device, module_to_process,
                                                   n_samples, sparsity_ratio)

    @print_time
    def prune(self, importance_scores=None, keep_indices_or_masks=None):
        print("In: ", self.pruner_name)
        dtype_record, requires_grad_record, device = self.model_setup_and_record_attributes(self.model)

        global_sparsity_dict = None
        if self.sparsity_ratio_granularity is not None:
            _, vit_keep_ratio, _, _ = self.convert_spec_to_list(self.visual_prune_spec)
            _, t5_keep_ratio, _, _ = self.convert_spec_to_list(self.language_prune_spec)
            assert vit_keep_ratio == t5_keep_ratio
            global_sparsity_dict = self.get_sparsity(
                1 - vit_keep_ratio, sparsity_ratio_granularity=self.sparsity_ratio_granularity)

        def table_for(spec):
            if global_sparsity_dict is not None:
                return global_sparsity_dict
            _, keep_ratio, _, _ = self.convert_spec_to_list(spec)
            return self.get_sparsity(1 - keep_ratio, sparsity_ratio_granularity=None)

        for spec, prefix in ((self.visual_prune_spec, self.visual_model_prefix),
                             (self.language_prune_spec, self.language_model_prefix)):
            if spec is None:
                continue
            self.model = self._prune(self.model, self.data_loader, device, model_prefix=prefix,
                                     module_to_process=f"{prefix}.resblocks",
                                     n_samples=self.num_samples, sparsity_ratio=table_for(spec))
        self.model_reset(self.model, dtype_record, requires_grad_record, device)
        return self.model, global_sparsity_dict
