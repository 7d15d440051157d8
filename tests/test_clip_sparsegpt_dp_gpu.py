"""GPU: `clip_sparsegpt_pruner` under data parallelism — two ranks sharing cuda:0 over gloo (what
a 1-GPU box can run, as tests/test_clip_pruner_dp_gpu.py): after `_merge_hessians`, once per block,
both ranks hold the same Hessians and end with identical tables and pruned weights.  Equality with
the one-process run is not asserted: the merge re-associates the sums."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import free_port  # noqa: E402

BATCHES, BATCH, CLASSES = 4, 16, 100


def _job():
    from ecoflap_amd import hip, load_pruner
    from ecoflap_amd.pruners.losses import clip_contrastive
    from ecoflap_amd.shapes import clip as C
    torch.manual_seed(21)
    model = C.clip_slice(1, 1, fp16=True).eval().cuda()
    g = torch.Generator().manual_seed(22)
    prompts = torch.randint(1, 49000, (CLASSES, 77), generator=g)
    prompts[torch.arange(CLASSES), torch.randint(5, 77, (CLASSES,), generator=g)] = 49407
    loader = [{"img": torch.randn(BATCH, 3, 224, 224, generator=g).cuda(),
               "label": torch.randperm(CLASSES, generator=g)[:BATCH].cuda()} for _ in range(BATCHES)]
    np.random.seed(42)
    torch.manual_seed(42)
    cfg = dict(visual_prune_spec="1-0.6-1-1", language_prune_spec="1-0.6-1-1", language_pruning_method="none",
               visual_pruning_method="none", num_samples=BATCHES * BATCH, num_data_first_stage=32,
               sparsity_ratio_granularity="block", max_sparsity_per_layer=0.5,
               score_method="MEZO-GradOnly_sum", kernels=hip.HipKernels())
    pruner = load_pruner("clip_sparsegpt_pruner", model, loader, cfg=cfg)
    pruner.forward_to_cache = clip_contrastive(prompts.cuda())
    model, table = pruner.prune()
    torch.cuda.synchronize()
    weights = {n: p.detach().cpu() for n, p in model.named_parameters() if p.dim() == 2 and ".resblocks" in n}
    return {"table": table,
            "hashes": {n: hashlib.sha256(w.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
                       for n, w in weights.items()},
            "sparsity": {n: float((w == 0).float().mean()) for n, w in weights.items()},
            "stats": {k: v for k, v in pruner.stage_stats.items() if isinstance(v, int)}}


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)                       # every rank on the one GPU
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.save(_job(), os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_the_gpu_end_with_identical_hashes(tmp_path):
    mp.spawn(_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(2)]
    assert a["table"] == b["table"] and len(set(a["table"].values())) > 1
    assert a["hashes"] == b["hashes"] and len(a["hashes"]) == 8
    for res in (a, b):
        # a rank hooks its 2 of the 4 batches per tower, the operand still from the attention kernel
        assert res["stats"]["attention_operand_calls"] == 2 * BATCHES // 2
        for n, s in res["sparsity"].items():
            assert abs(s - res["table"][n]) < 0.01, (n, s, res["table"][n])
