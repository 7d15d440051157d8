"""CPU: `clip_sparsegpt_pruner` IS the reference's `CLIPLayerSparseGPTPruner` as far as its results
tell.  Every case of `g21_clip_sparsegpt.npz` (made by tests/golden/make_golden_clip_sparsegpt.py,
which ran the reference's own class on the build's CLIP modules) goes through `load_pruner` on the
oracle-backed kernels, single-threaded, and must come out bit for bit: the returned table (keys,
order, float64 values; None for the uniform case), every pruned matrix (sha256; the zero masks too
for the toy cases) and the whole final state.  The toy Hessians are rank deficient (16 tokens
against 32 to 256 columns): the damping retry is taken, on both sides by the same LAPACK."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_clip_pruner as G  # noqa: E402  (models, batches, seeds, hashes)
import make_golden_clip_sparsegpt as S  # noqa: E402  (the cases; the reference is only touched by its main())

from oracle_backend import OracleKernels, torch_cpu_normal  # noqa: E402


def run_build(name, granularity, **extra):
    from ecoflap_amd import load_pruner
    model = G.build_model(name)
    initial = {k: v.detach().clone() for k, v in model.state_dict().items()}
    loader, prompts = G.batches(name)
    G.seed_run()
    cfg = dict(G.pruner_config(name, granularity), kernels=OracleKernels(), z_source=torch_cpu_normal)
    cfg.update(extra)
    pruner = load_pruner("clip_sparsegpt_pruner", model, loader, cfg=cfg)
    pruner.forward_to_cache = G.closure(prompts)
    model, table = pruner.prune()
    return model, table, initial, pruner


@pytest.mark.parametrize("name,granularity", S.CASES, ids=[S.case_key(*c) for c in S.CASES])
def test_pruner_equals_the_reference_bit_for_bit(golden_dir, name, granularity):
    g = np.load(os.path.join(golden_dir, "g21_clip_sparsegpt.npz"))
    assert int(g["seed"]) == G.SEED
    key = S.case_key(name, granularity)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                    # (the recipe's setting: one summation order)
    try:
        assert G.state_sha256(G.build_model(name).state_dict()) == str(g[key + "_state_sha256"])
        model, table, initial, _ = run_build(name, granularity)
    finally:
        torch.set_num_threads(threads)
    if granularity is None:
        assert table is None and len(g[key + "_table_keys"]) == 0
    else:
        assert list(table.keys()) == [str(k) for k in g[key + "_table_keys"]]
        assert np.array_equal(np.array([float(v) for v in table.values()], dtype=np.float64),
                              g[key + "_table_values"])
    mats = G.prunable(model)
    assert [n for n, _ in mats] == [str(n) for n in g[key + "_matrix_names"]]
    for (n, p), sha in zip(mats, g[key + "_matrix_sha256"]):
        if name.startswith("toy"):
            assert np.array_equal(np.packbits((p.data == 0).numpy().reshape(-1)), g[f"{key}_mask_{n}"]), n
        assert G.tensor_sha256(p.data) == str(sha), n
    assert G.state_sha256(model.state_dict()) == str(g[key + "_final_state_sha256"])
    if granularity is None:     # no stage 1: what is not a prunable matrix is exactly what it was
        pruned = {n for n, _ in mats}
        for k, v in model.state_dict().items():
            if k not in pruned:
                assert torch.equal(v, initial[k]), k


def test_text_out_proj_hessian_comes_from_the_unmasked_attention(monkeypatch):
    """The quirk of sparsegpt_pruner.py:441-458: out_proj's Hessian comes from a side copy of the
    attention that has no mask, in the text tower too, while the block's forward stays causal."""
    from ecoflap_amd.pruners import clip_sparsegpt as P
    seen = []
    real_operand = P._HessianSites.operand

    def operand(self, name, x):
        seen.append((name, x.detach().clone()))
        return real_operand(self, name, x)

    monkeypatch.setattr(P._HessianSites, "operand", operand)
    blocks_in = []
    model = G.build_model("toy_fp32")
    text0 = model.transformer.resblocks[0]
    weights = (text0.attn.in_proj_weight.detach().clone(), text0.attn.in_proj_bias.detach().clone())
    handle = text0.ln_1.register_forward_hook(lambda _m, _i, out: blocks_in.append(out.detach().clone()))
    from ecoflap_amd import load_pruner
    loader, prompts = G.batches("toy_fp32")
    G.seed_run()
    pruner = load_pruner("clip_sparsegpt_pruner", model, loader,
                         cfg=dict(G.pruner_config("toy_fp32", None), kernels=OracleKernels(),
                                  z_source=torch_cpu_normal))
    pruner.forward_to_cache = G.closure(prompts)
    hooked_first = []
    real_run = P._ClipBlockwiseSparseGPT._run_tower

    def run_tower(self, model_, loader_, device, module_to_process, *a):
        if module_to_process == "transformer.resblocks":
            hooked_first.append((len(seen), len(blocks_in)))
        return real_run(self, model_, loader_, device, module_to_process, *a)

    monkeypatch.setattr(P._ClipBlockwiseSparseGPT, "_run_tower", run_tower)
    pruner.prune()
    handle.remove()
    n_seen, n_in = hooked_first[0]
    # the text tower's first hooked forward of block 0: ln_1's output after the 4 capture forwards
    x = blocks_in[n_in + 4]                                         # [L, N, D]
    operand_ = [s for s in seen[n_seen:] if s[0] == "attn.out_proj"][0][1]
    L, N, D = x.shape
    heads = text0.attn.num_heads
    qkv = F.linear(x.permute(1, 0, 2), *weights).reshape(N, L, 3, heads, D // heads).permute(2, 0, 3, 1, 4)

    def gram(causal):
        o = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], is_causal=causal)
        o = o.transpose(1, 2).reshape(N * L, D).double()
        return o.t() @ o

    got = operand_.reshape(N * L, D).double()
    got = got.t() @ got
    scale = gram(False).abs().max()
    assert (got - gram(False)).abs().max() <= 1e-4 * scale
    assert (got - gram(True)).abs().max() > 1e-2 * gram(True).abs().max()
    assert text0.attn_mask is not None          # (and the block's own forward is still masked)
