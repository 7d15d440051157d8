"""CPU: `llama_wanda_pruner` and `llama_sparsegpt_pruner` on the oracle backend on a grouped-query
decoder (4 query heads on 2 key / value heads: `k_proj` / `v_proj` have half the rows of `q_proj`)
against `g26_llama_gqa_pruners.npz` — what the reference's own `LayerSparsity.return_sparsity()`
(stage 1) and `T5LayerWandaPruner._prune` / `T5LayerSparseGPTPruner._prune` (stage 2) gave on the same
seeded model in fp32 (recipe: tests/golden/make_golden_llama_gqa_pruners.py): the table's keys, order
and float64 values, the sha256 of every pruned matrix, the packed zero masks and the final state —
the zeroth-order drift included — bit for bit.  q / k / v still share one factorisation although
their row counts differ: the twins are found by their Hessians."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from llama_pruner_fixture import prunable_names, sha256  # noqa: E402
from make_golden_llama_gqa_pruners import (CASES, calibration, gqa_tiny, packed_masks, pruner_config,  # noqa: E402
                                           stored_masks)
from make_golden_llama_pruner import seed_run, state_sha256  # noqa: E402
import make_golden_llama_sparsegpt as S  # noqa: E402

PRUNER = {"wanda": "llama_wanda_pruner", "sparsegpt": "llama_sparsegpt_pruner"}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "g26_llama_gqa_pruners.npz"))


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_the_fixture_is_no_larger_than_g24(golden_dir):
    assert (os.path.getsize(os.path.join(golden_dir, "g26_llama_gqa_pruners.npz"))
            <= os.path.getsize(os.path.join(golden_dir, "g24_llama_sparsegpt.npz")))


@pytest.mark.parametrize("case", list(CASES))
def test_reference_results_bit_for_bit(golden, case, monkeypatch):
    from ecoflap_amd import load_pruner
    from ecoflap_amd.pruners.sparsegpt import SparseGPT
    from oracle_backend import OracleKernels, torch_cpu_normal
    recipe, name = CASES[case]
    granularity, method = recipe.CASES[name]
    factored = []
    factor_alone = SparseGPT._factor_alone
    monkeypatch.setattr(SparseGPT, "_factor_alone",
                        lambda self, percdamp: (factored.append(self.columns), factor_alone(self, percdamp))[1])
    model = gqa_tiny()
    attn = model.model.layers[0].self_attn
    assert attn.q_proj.weight.shape[0] == 2 * attn.k_proj.weight.shape[0] == 2 * attn.v_proj.weight.shape[0] == 512
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert state_sha256(before) == str(golden[case + "_state_sha256"])
    loader = calibration(case, model.config.vocab_size)
    seed_run()
    cfg = dict(pruner_config(case), kernels=OracleKernels(), z_source=torch_cpu_normal)
    model, table = load_pruner(PRUNER[case.split("_")[0]], model, loader, cfg=cfg).prune()
    names = prunable_names(model)
    assert names == list(golden[case + "_matrix_names"]) and len(names) == 14
    if granularity is None:
        assert len(golden[case + "_table_keys"]) == 0
        assert all(table[n] == 1 - 0.4 for n in names)
    else:
        assert list(table.keys()) == list(golden[case + "_table_keys"]) == names
        got = np.array([table[k] for k in table], dtype=np.float64)
        assert np.array_equal(got, golden[case + "_table_values"]), np.abs(got - golden[case + "_table_values"]).max()
        assert len(set(got.tolist())) > 1
    state = dict(model.named_parameters())
    assert np.array_equal(packed_masks(state, names), stored_masks(golden, case))
    for n, want in zip(names, golden[case + "_matrix_sha256"]):
        assert sha256(state[n].data) == str(want), n
    assert state_sha256(model.state_dict()) == str(golden[case + "_final_state_sha256"])
    if recipe is S:
        # twins: one factorisation for q / k / v (64 columns; 512, 256 and 256 rows), one for o (512
        # columns), one for gate / up (64), one for down (176), per block
        assert factored == [64, 512, 64, 176] * 2, factored
    else:
        assert factored == []
    if not method.startswith("MEZO"):
        for k, v in model.state_dict().items():
            if k in names:
                kept = v != 0
                assert torch.equal(v[kept], before[k][kept]), k
            else:
                assert torch.equal(v, before[k]), k
