"""CPU: `llama_sparsegpt_pruner` on the oracle backend against `g24_llama_sparsegpt.npz` — what the
reference's own `LayerSparsity.return_sparsity()` (stage 1) and `T5LayerSparseGPTPruner._prune` with
its own `SparseGPT` (stage 2) gave on the same seeded `llama_tiny()` in fp32 with 8 calibration
batches of one sample (recipe: tests/golden/make_golden_llama_sparsegpt.py): the table's keys, order
and float64 values, the sha256 of every pruned matrix, the packed zero masks and the final state —
the zeroth-order drift included — bit for bit.  q / k / v and gate / up of a block share one
factorisation: four per block, not seven."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from llama_pruner_fixture import prunable_names, seeded_tiny, sha256  # noqa: E402
from make_golden_llama_sparsegpt import CASES, calibration, pruner_config  # noqa: E402
from make_golden_llama_pruner import seed_run, state_sha256  # noqa: E402


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "g24_llama_sparsegpt.npz"))


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("case", list(CASES))
def test_reference_results_bit_for_bit(golden, case, monkeypatch):
    from ecoflap_amd import load_pruner
    from ecoflap_amd.pruners.sparsegpt import SparseGPT
    from oracle_backend import OracleKernels, torch_cpu_normal
    factored = []
    factor_alone = SparseGPT._factor_alone
    monkeypatch.setattr(SparseGPT, "_factor_alone",
                        lambda self, percdamp: (factored.append(self.columns), factor_alone(self, percdamp))[1])
    model = seeded_tiny()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert state_sha256(before) == str(golden[case + "_state_sha256"])
    loader = calibration(model.config.vocab_size)
    seed_run()
    cfg = dict(pruner_config(case), kernels=OracleKernels(), z_source=torch_cpu_normal)
    pruner = load_pruner("llama_sparsegpt_pruner", model, loader, cfg=cfg)
    assert pruner.local_method == "sparsegpt" and pruner.whole_matrix_sweep is True
    model, table = pruner.prune()
    names = prunable_names(model)
    assert names == list(golden[case + "_matrix_names"]) and len(names) == 14
    if CASES[case][0] is None:
        assert len(golden[case + "_table_keys"]) == 0
        assert all(table[n] == 1 - 0.4 for n in names)
    else:
        assert list(table.keys()) == list(golden[case + "_table_keys"]) == names
        got = np.array([table[k] for k in table], dtype=np.float64)
        assert np.array_equal(got, golden[case + "_table_values"]), np.abs(got - golden[case + "_table_values"]).max()
        assert len(set(got.tolist())) > 1
    state = dict(model.named_parameters())
    for n, want in zip(names, golden[case + "_matrix_sha256"]):
        mask = np.packbits((state[n].data == 0).numpy().reshape(-1))
        assert np.array_equal(mask, golden[f"{case}_mask_{n}"]), n
        assert sha256(state[n].data) == str(want), n
    assert state_sha256(model.state_dict()) == str(golden[case + "_final_state_sha256"])
    # twins: one factorisation for q / k / v (64 columns), one for o (256), one for gate / up (64),
    # one for down (176), per block
    assert factored == [64, 256, 64, 176] * 2, factored
    if not CASES[case][1].startswith("MEZO"):
        for k, v in model.state_dict().items():          # what is not prunable is untouched
            if k not in names:
                assert torch.equal(v, before[k]), k


def test_the_class_defaults_of_sparsegpt_are_left_alone():
    """The pruner sets its choices on its own `SparseGPT` objects, never on the class."""
    from ecoflap_amd import load_pruner
    from ecoflap_amd.pruners.sparsegpt import SparseGPT
    from oracle_backend import OracleKernels, torch_cpu_normal
    model = seeded_tiny()
    seed_run()
    cfg = dict(pruner_config("uniform"), kernels=OracleKernels(), z_source=torch_cpu_normal)
    load_pruner("llama_sparsegpt_pruner", model, calibration(model.config.vocab_size), cfg=cfg).prune()
    assert SparseGPT.whole_matrix_sweep is False and SparseGPT.literal_update is False


def test_data_parallel_is_refused():
    from ecoflap_amd import load_pruner
    model = seeded_tiny()
    with pytest.raises(NotImplementedError):
        load_pruner("llama_sparsegpt_pruner", model, calibration(96),
                    cfg=dict(pruner_config("uniform"), process_group=object()))
