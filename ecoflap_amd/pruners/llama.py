"""`llama_wanda_pruner`: ECoFLaP / Wanda on a LLaMA decoder (`shapes/llama.py::LlamaForCausalLM`).

The reference's LLaMA path (`LLaMA/main.py`, `scripts/ecoflap_zero.sh` / `ecoflap_first.sh`) runs
Wanda on `huggyllama/llama-7b` in fp16 at 2048 tokens with a sparsity table from ECoFLaP's stage 1;
the `lib/` that held its loops is not part of the reference tree, so this pruner is put
together from the pieces the T5 pruner is made of, in its shape (`_StageOneMixin`,
`LayerWiseBasePruner`; `prune() -> (model, table_or_None)`):

  prunable   per decoder block the seven Linears `find_layers` finds, in `named_parameters()` order:
             `model.layers.N.self_attn.{q,k,v,o}_proj.weight`, `model.layers.N.mlp.{gate,up,down}_proj.weight`;
             `embed_tokens` and `lm_head` are never pruned;
  stage 1    `LayerSparsity` on `loss_causal_lm` (the labels of a calibration batch are its ids); a
             group of `sparsity_ratio_granularity` "block" is one `model.layers.N`; on the staged
             model the zeroth-order losses come from `PrefixCachedLoss`, whose last stage ends in
             the fused loss kernel (csrc/lm_loss.hip);
  stage 2    `_BlockwiseWanda` over `model.layers` (blocks take and return one tensor), selection per
             output row (the LLaMA loop of Wanda, LAVIS/lavis/compression/pruners/wanda_pruner.py:272-277).
"""
import contextlib

from ..registry import registry
from .base_pruner import LayerWiseBasePruner, print_time
from .losses import loss_causal_lm
from .wanda import _BlockwiseWanda, _StageOneMixin, _t5_block_mapping


@registry.register_pruner("llama_wanda_pruner")
class LlamaLayerWandaPruner(_StageOneMixin, LayerWiseBasePruner):
    pruner_name = "llama_wanda_pruner"

    def __init__(self, model, data_loader, model_prefix="model", **kwargs):
        if kwargs.get("process_group") is not None:
            raise NotImplementedError("llama_wanda_pruner runs in one process")
        super().__init__(model=model, data_loader=data_loader, model_prefix=model_prefix, **kwargs)
        self.loss_func = loss_causal_lm

    def forward_to_cache(self, model, batch):
        return model(batch["input_ids"])

    def prunable_names(self):
        return [k for k, v in self.model.named_parameters()
                if len(v.shape) == 2 and k.startswith(f"{self.model_prefix}.layers.")]

    def get_sparsity(self, original_sparsity, sparsity_ratio_granularity=None):
        if self.sparsity_dict is not None:
            return self._load_sparsity_yaml()
        if sparsity_ratio_granularity is None:
            mapping = {}
        elif sparsity_ratio_granularity == "model":
            mapping = {k: self.model_prefix for k in self.prunable_names()}
        else:       # "model.layers.N" is three components deep
            mapping = _t5_block_mapping(self.prunable_names(), sparsity_ratio_granularity, depth=3)
        return self._layer_sparsity(loss_causal_lm, original_sparsity, mapping)

    @print_time
    def _prune(self, model, dataloader, device, model_prefix, module_to_process="model.layers",
               n_samples=64, sparsity_ratio=0.5):
        cfg = model.config
        use_cache, cfg.use_cache = cfg.use_cache, False
        try:
            _BlockwiseWanda(self).run(
                model, dataloader, module_to_process, n_samples, sparsity_ratio,
                forward_fn=lambda m, b: self.forward_to_cache(m, b), cache_keys=[],
                autocast=contextlib.nullcontext, take_first=False, mode="rows",
                batch_len=lambda b: len(b["input_ids"]))
        finally:
            cfg.use_cache = use_cache
        return model

    @print_time
    def prune(self, importance_scores=None, keep_indices_or_masks=None):
        print("In: ", self.pruner_name)
        dtype_record, requires_grad_record, device = self.model_setup_and_record_attributes(self.model)
        if self.prune_spec is None:
            return self.model, None
        _, keep_ratio, _, _ = self.convert_spec_to_list(self.prune_spec)
        sparsity_dict = self.get_sparsity(1 - keep_ratio,
                                          sparsity_ratio_granularity=self.sparsity_ratio_granularity)
        self.model = self._prune(self.model, self.data_loader, device, model_prefix=self.model_prefix,
                                 module_to_process=f"{self.model_prefix}.layers",
                                 n_samples=self.num_samples, sparsity_ratio=sparsity_dict)
        self.model_reset(self.model, dtype_record, requires_grad_record, device)
        return self.model, sparsity_dict


@registry.register_pruner("llama_sparsegpt_pruner")
class LlamaLayerSparseGPTPruner(LlamaLayerWandaPruner):
    """ECoFLaP / SparseGPT on the same decoder (`LLaMA/main.py:36`, `--prune_method sparsegpt`): stage 1,
    `get_sparsity` and `prune()` are `llama_wanda_pruner`'s; stage 2 is `_BlockwiseWanda`'s SparseGPT
    branch — per block one hooked pass completes the seven Hessians, then every matrix is swept at
    its table entry (the loop of `T5LayerSparseGPTPruner._prune`, sparsegpt_pruner.py:226-420, which
    the CPU run equals bit for bit).  q / k / v and gate / up see the same tensor: their Hessians are
    bit-identical, one factorisation serves each set, and with `sparsegpt_group_twins` each set's
    sweeps run side by side in one host call (`ecoflap_sparsegpt_matrix_group`), every matrix with the
    bits of its own sweep."""
    pruner_name = "llama_sparsegpt_pruner"
    local_method = "sparsegpt"
    whole_matrix_sweep = True       # the column sweep of a matrix in one host call (pruners/sparsegpt.py)
    literal_update = True           # fp32 inputs: `H += x^T x` as the reference rounds it
    # Twin sets swept side by side: on, by the measurement at the 7B shapes (the grouped
    # median is below the one-by-one median by more than the one-by-one form's own max - min at
    # 3 x [4096, 4096] and at 2 x [11008, 4096]); the bits are those of the one-by-one sweeps.
    sparsegpt_group_twins = True

    def __init__(self, model, data_loader, whole_matrix_sweep=None, sparsegpt_group_twins=None, **kwargs):
        super().__init__(model, data_loader, **kwargs)
        if whole_matrix_sweep is not None:
            self.whole_matrix_sweep = bool(whole_matrix_sweep)
        if sparsegpt_group_twins is not None:
            self.sparsegpt_group_twins = bool(sparsegpt_group_twins)
