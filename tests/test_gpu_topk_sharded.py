"""``sharding.topk_sharded`` through RCCL: an in-process ``nccl`` (= RCCL) group of world
size 1 on cuda:0, as test_gpu_sharded.py drives the pair scorer.  Every rank ranks its
own rows, one all-gather moves the (B, K) lists, the merge runs on the device -- and the
table itself is never gathered.  Multi-rank correctness of the same code is covered over
gloo (test_topk_host.py)."""
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
    fd, path = tempfile.mkstemp(prefix="msha_rccl1_topk_")
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
def test_rccl_world1_topk_sharded(cuda, rccl1, dt):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd import sharding

    n, F, B, K = 10_007, 128, 130, 50
    g = torch.Generator().manual_seed(51)
    h = (torch.rand(n, F, generator=g) - 0.4).to(dt).to(cuda)
    q = (torch.rand(B, F, generator=g) - 0.4).to(dt).to(cuda)
    tab = sharding.ShardedTable(n, F, 1, 0, cuda, dtype=dt)
    assert tab.path() == "rccl"
    tab.set_local(h)
    tab.full.fill_(-7.0)  # a sentinel: a full-table gather would overwrite it
    qpos = torch.tensor([0, 0, 3, 3, 3, 129], device=cuda)
    cols = torch.tensor([5, n - 1, 0, 17, 9_000, 4_242], device=cuda)
    ex = MF.exclude_from_pairs(qpos, cols, B)

    def topk_fn(qq, local, k, ex_local, off):
        assert local.shape[0] == n and off == 0
        return MF.topk_inner(qq, local, k, exclude=ex_local, sigmoid=False, col_offset=off)

    def merge_fn(v, i, k):
        assert v.shape == (B, 1, k)
        return MF.topk_merge(v, i, k, sigmoid=True)

    for exclude in (None, ex):
        got = sharding.topk_sharded(tab, q, K, topk_fn, merge_fn, exclude=exclude)
        want = MF.topk_inner(q, h, K, exclude=exclude, sigmoid=True)
        torch.cuda.synchronize()
        assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])  # bit for bit
    assert not (set(got[1][3].tolist()) & {0, 17, 9_000})
    assert (tab.full == -7.0).all()  # the table was never gathered
    assert int(got[1].max()) < n
