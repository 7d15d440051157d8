"""CPU: `llama_wanda_pruner` on the oracle backend against `g23_llama_wanda.npz` — what the
reference's own `LayerSparsity.return_sparsity()` (stage 1) and `T5LayerWandaPruner._prune`
(stage 2, the rows-mode loop) gave on the same seeded `llama_tiny()` in fp32 (recipe:
tests/golden/make_golden_llama_pruner.py): the table's keys, order and float64 values, the sha256
of every pruned matrix, the packed zero masks and the final state — the zeroth-order drift
included — bit for bit; in the uniform case everything that is not prunable stays untouched."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from llama_pruner_fixture import batches, prunable_names, seeded_tiny, sha256  # noqa: E402
from make_golden_llama_pruner import CASES, pruner_config, seed_run, state_sha256  # noqa: E402


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "g23_llama_wanda.npz"))


@pytest.fixture(autouse=True)
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("case", list(CASES))
def test_reference_results_bit_for_bit(golden, case):
    from ecoflap_amd import load_pruner
    from oracle_backend import OracleKernels, torch_cpu_normal
    model = seeded_tiny()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert state_sha256(before) == str(golden[case + "_state_sha256"])
    loader = batches(vocab=model.config.vocab_size)
    seed_run()
    cfg = dict(pruner_config(case), kernels=OracleKernels(), z_source=torch_cpu_normal)
    model, table = load_pruner("llama_wanda_pruner", model, loader, cfg=cfg).prune()
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
    if not CASES[case][1].startswith("MEZO"):
        # no perturbation: what survives a matrix is its initial value, everything else is untouched
        for k, v in model.state_dict().items():
            if k in names:
                kept = v != 0
                assert torch.equal(v[kept], before[k][kept]), k
            else:
                assert torch.equal(v, before[k]), k


def test_data_parallel_is_refused():
    from ecoflap_amd import load_pruner
    model = seeded_tiny()
    with pytest.raises(NotImplementedError):
        load_pruner("llama_wanda_pruner", model, batches(), cfg=dict(pruner_config("uniform"), process_group=object()))


def test_sparsity_dict_reingest(tmp_path):
    """A table written by one run (`--sparsity_dict`) drives stage 2 of another: same pruned weights."""
    import yaml
    from ecoflap_amd import load_pruner
    from oracle_backend import OracleKernels, torch_cpu_normal
    model = seeded_tiny()
    seed_run()
    cfg = dict(pruner_config("first_block"), kernels=OracleKernels(), z_source=torch_cpu_normal)
    model, table = load_pruner("llama_wanda_pruner", model, batches(), cfg=cfg).prune()
    path = tmp_path / "table.yaml"
    path.write_text(yaml.dump(dict(table)))
    again = seeded_tiny()
    seed_run()
    again, table2 = load_pruner("llama_wanda_pruner", again, batches(),
                                cfg=dict(cfg, kernels=OracleKernels(), sparsity_dict=str(path))).prune()
    assert table2 == table
    for (k, a), (_, b) in zip(model.state_dict().items(), again.state_dict().items()):
        assert torch.equal(a, b), k
