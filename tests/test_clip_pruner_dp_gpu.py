"""GPU: `clip_wanda_pruner` under data parallelism with the HIP kernels — two ranks sharing cuda:0
over gloo (what a 1-GPU box can run, as tests/test_dp_one_gpu.py) against the ONE-process run, both
spawned afresh: sparsity table, loss table and every pruned weight bit for bit.  In the ranks the
out_proj statistic still comes from the attention kernel (`ecoflap_mha_attention_colsq`): each
batch's `sq` is that site's row of `_K6Collector`'s raw mode and is replayed in global batch order."""
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

BATCHES, BATCH, CLASSES = 4, 8, 100


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
               visual_pruning_method="none", num_samples=BATCHES * BATCH, num_data_first_stage=BATCHES * BATCH,
               sparsity_ratio_granularity="block", max_sparsity_per_layer=0.5,
               score_method="MEZO-GradOnly_sum", kernels=hip.HipKernels())
    pruner = load_pruner("clip_wanda_pruner", model, loader, cfg=cfg)
    pruner.forward_to_cache = clip_contrastive(prompts.cuda())
    model, table = pruner.prune()
    torch.cuda.synchronize()
    return {"table": table, "losses": np.array(pruner.last_loss_table),
            "weights": {n: p.detach().cpu() for n, p in model.named_parameters()
                        if p.dim() == 2 and ".resblocks" in n},
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


def test_two_ranks_on_the_gpu_reproduce_one_process(tmp_path):
    mp.spawn(_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    ranks = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(2)]
    one = tmp_path / "one_process"
    one.mkdir()
    mp.spawn(_worker, args=(1, free_port(), str(one)), nprocs=1, join=True)
    single = torch.load(one / "r0.pt", weights_only=False)
    # one process: 2 towers x 1 block x 4 hooked forwards through the kernel, folded at once
    assert single["stats"]["attention_colsq_calls"] == 2 * BATCHES and "k6_dp_exact_blocks" not in single["stats"]
    assert len(set(single["table"].values())) > 1
    for res in ranks:
        # a rank: its 2 of the 4 batches per tower, still through the kernel, kept apart and replayed
        assert res["stats"]["attention_colsq_calls"] == 2 * BATCHES // 2
        assert res["stats"]["k6_dp_exact_blocks"] == 2
        assert res["table"] == single["table"]
        assert np.array_equal(res["losses"].view(np.uint32), single["losses"].view(np.uint32))
        bad = [n for n in single["weights"] if not torch.equal(res["weights"][n], single["weights"][n])]
        assert not bad, bad
