"""``sharding.rank_sharded`` through RCCL: an in-process ``nccl`` (= RCCL) group of world
size 1 on cuda:0, as test_gpu_topk_sharded.py drives the top-K retrieval.  The owner's
logits and the counts each cross one all-reduce, the kernel is the real ``rank_inner`` --
and the table itself is never gathered.  Multi-rank correctness of the same code is covered
over gloo (test_rank_host.py)."""
import os
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rccl1(cuda):
    import torch.distributed as dist

    if dist.is_initialized():
        pytest.skip("a process group is already initialised in this process")
    fd, path = tempfile.mkstemp(prefix="msha_rccl1_rank_")
    os.close(fd)
    os.unlink(path)
    store = dist.FileStore(path, 1)
    dist.init_process_group("nccl", store=store, rank=0, world_size=1, device_id=cuda)
    try:
        yield dist
    finally:
        dist.destroy_process_group()
        if os.path.exists(path):
            os.unlink(path)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_rccl_world1_rank_sharded(cuda, rccl1, dt):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import sharding

    n, F, B = 10_007, 128, 130
    g = torch.Generator().manual_seed(51)
    h = (torch.rand(n, F, generator=g) - 0.4).to(dt).to(cuda)
    q = (torch.rand(B, F, generator=g) - 0.4).to(dt).to(cuda)
    target = torch.randint(0, n, (B,), generator=g).to(cuda)
    tab = sharding.ShardedTable(n, F, 1, 0, cuda, dtype=dt)
    assert tab.path() == "rccl"
    tab.set_local(h)
    tab.full.fill_(-7.0)  # a sentinel: a full-table gather would overwrite it
    qpos = torch.tensor([0, 0, 3, 3, 3, 129], device=cuda)
    cols = torch.tensor([5, n - 1, 0, 17, 9_000, 4_242], device=cuda)
    ex = MF.exclude_from_pairs(qpos, cols, B)
    calls = []

    def rank_fn(qq, local, tg, ex_local, off, target_logit):
        assert local.shape[0] == n and off == 0
        calls.append(target_logit is not None)
        return MF.rank_inner(qq, local, tg, exclude=ex_local, col_offset=off,
                             target_logit=target_logit, check=False)

    for exclude in (None, ex):
        got = sharding.rank_sharded(tab, q, target, rank_fn, exclude=exclude)
        want = MF.rank_inner(q, h, target, exclude=exclude)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32))  # bit for bit
    assert calls == [False, True, False, True]  # the owner's logits, then the counts
    assert (got[0] >= 0).all()
    assert (tab.full == -7.0).all()  # the table was never gathered
