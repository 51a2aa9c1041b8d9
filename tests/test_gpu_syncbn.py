"""GPU: SyncBatchNorm on the kernels of csrc/norm.hip between real ranks (spconv_amd/pytorch/norm.py _SyncBatchNormFn).

A one-GPU box cannot host two RCCL ranks, so two ranks share cuda:0 over gloo (as tests/test_gpu_ddp.py does): the
all-gather of the statistics records and the all-reduce of the backward sums are the real collectives, only the
transport differs.  The process group has a 60 s timeout: a rank that skips a collective is an error, not a wait.

The two ranks are started ONCE (module fixture); each section below leaves its findings, or its traceback, under its
own key and the tests assert on them."""
import copy
import os
import socket
import traceback
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

WORLD = 2


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rel(got, want):
    return float((got.detach().double() - want.detach().double()).abs().max()) / (float(want.detach().double().abs().max()) + 1e-12)


def _section_path_taken(rank, dev):
    """(a) SubMConv3d -> SyncBatchNorm -> ReLU in a SparseSequential, sharded by scene, against the same network with a
    plain BatchNorm1d on the full batch."""
    import spconv_amd.pytorch as spconv
    from spconv_amd import _lib
    from spconv_amd.dist import GradBucket, shard_scenes
    from spconv_amd.pytorch import norm
    shape, bs, per_scene, cin, cout = [16, 32, 32], 2, 1500, 8, 16
    rng = np.random.default_rng(3)
    rows = []
    for b in range(bs):
        lin = rng.choice(int(np.prod(shape)), per_scene, replace=False)
        rows.append(np.concatenate([np.full((per_scene, 1), b), np.stack(np.unravel_index(lin, shape), 1)], 1))
    idx = torch.from_numpy(np.concatenate(rows).astype(np.int32)).to(dev)
    feat = torch.from_numpy(rng.uniform(-1, 1, (idx.shape[0], cin)).astype(np.float32)).to(dev).half()
    gout = torch.from_numpy(rng.standard_normal((idx.shape[0], cout)).astype(np.float32)).to(dev)
    torch.manual_seed(5)
    ref = spconv.SparseSequential(spconv.SubMConv3d(cin, cout, 3, bias=False), torch.nn.BatchNorm1d(cout),
                                  torch.nn.ReLU()).to(dev).half().train()
    with torch.no_grad():
        ref[1].weight.uniform_(0.5, 1.5)
        ref[1].bias.uniform_(-0.5, 0.5)
    net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(copy.deepcopy(ref))
    assert type(net[1]) is torch.nn.SyncBatchNorm and norm.sync_group(net[1]) is not None
    # the full batch, one process, plain BatchNorm1d
    f_ref = feat.clone().requires_grad_(True)
    y_ref = ref(spconv.SparseConvTensor(f_ref, idx, shape, bs)).features
    (y_ref.float() * gout).sum().backward()
    # this rank's scene through the synchronising network
    own = (idx[:, 0] == rank)
    li, lf, lb = shard_scenes(idx, feat, bs, rank, WORLD)
    lf = lf.clone().requires_grad_(True)
    L = _lib.load()
    seen = []
    real = L.spx_batchnorm_local_stats

    def spy(x, n, C, dt, stats_in, n_records, *rest):
        seen.append((bool(stats_in), int(n_records)))
        return real(x, n, C, dt, stats_in, n_records, *rest)

    def torch_path(self, input):
        raise AssertionError("torch.nn.SyncBatchNorm.forward was called: the layer left the HIP path")

    orig_forward = torch.nn.SyncBatchNorm.forward
    L.spx_batchnorm_local_stats = spy
    torch.nn.SyncBatchNorm.forward = torch_path
    try:
        y = net(spconv.SparseConvTensor(lf, li, shape, lb)).features
        (y.float() * gout[own]).sum().backward()
    finally:
        torch.nn.SyncBatchNorm.forward = orig_forward
        L.spx_batchnorm_local_stats = real
    GradBucket(net.parameters(), dtype=torch.float32).all_reduce(average=True)      # what DDP does: the mean over ranks
    res = dict(local_stats_calls=seen,
               y=_rel(y, y_ref[own]), dx=_rel(lf.grad, f_ref.grad[own]),
               params=[_rel(p.grad, q.grad / WORLD) for p, q in zip(net.parameters(), ref.parameters())],
               rm=bool(torch.allclose(net[1].running_mean.float(), ref[1].running_mean.float(), rtol=2e-3, atol=1e-3)),
               rv=bool(torch.allclose(net[1].running_var.float(), ref[1].running_var.float(), rtol=2e-3, atol=1e-3)),
               nbt=int(net[1].num_batches_tracked))
    return res


def _same_on_all_ranks(t):
    parts = [torch.empty_like(t) for _ in range(WORLD)]
    dist.all_gather(parts, t.contiguous())
    return all(torch.equal(parts[0], p) for p in parts[1:])


def _section_empty_and_static(rank, dev):
    """(b) norm.batch_norm directly: a rank without rows; then a rank whose rows are partly padding (n_live)."""
    from spconv_amd.pytorch import norm
    C = 32
    g = torch.Generator().manual_seed(21)
    x0 = (torch.randn(500, C, generator=g) * 1.3 + torch.linspace(-2, 2, C)).to(dev)
    x1 = (torch.randn(250, C, generator=g) * 0.7 + 1.0).to(dev)
    gw = torch.randn(750, C, generator=g).to(dev)           # dL/dy of the static-shape case, by global row
    res = {}
    # -- rank 1 holds no rows
    bn = torch.nn.SyncBatchNorm(C, eps=1e-3, momentum=0.1).to(dev).train()
    ref = torch.nn.BatchNorm1d(C, eps=1e-3, momentum=0.1).to(dev).train()
    x = (x0 if rank == 0 else x0[:0]).clone().requires_grad_(True)
    assert norm.supported(x, bn)
    y = norm.batch_norm(x, bn, relu=True)
    y.sum().backward()                                   # (the backward all-reduce is owed by the empty rank too)
    xr = x0.clone().requires_grad_(True)
    yr = torch.relu(ref(xr))
    yr.sum().backward()
    res["empty"] = dict(shape=tuple(y.shape), same_rm=_same_on_all_ranks(bn.running_mean),
                        same_rv=_same_on_all_ranks(bn.running_var),
                        rm=bool(torch.allclose(bn.running_mean, ref.running_mean, rtol=1e-4, atol=1e-5)),
                        rv=bool(torch.allclose(bn.running_var, ref.running_var, rtol=1e-4, atol=1e-5)),
                        nbt=int(bn.num_batches_tracked),
                        y=_rel(y, yr) if rank == 0 else 0.0, dx=_rel(x.grad, xr.grad) if rank == 0 else 0.0,
                        dw=_rel(bn.weight.grad, ref.weight.grad) if rank == 0 else float(bn.weight.grad.abs().max()))
    # -- rank 1 holds 400 allocated rows, 250 of them live; the padding is filled with 1e4
    bn = torch.nn.SyncBatchNorm(C, eps=1e-3, momentum=0.1).to(dev).train()
    ref = torch.nn.BatchNorm1d(C, eps=1e-3, momentum=0.1).to(dev).train()
    if rank == 0:
        x, n_live, live = x0.clone().requires_grad_(True), None, 500
    else:
        x = torch.full((400, C), 1e4, device=dev)
        x[:250] = x1
        x, n_live, live = x.requires_grad_(True), torch.tensor([250], dtype=torch.int32, device=dev), 250
    mine = slice(0, 500) if rank == 0 else slice(500, 750)
    gy = torch.ones_like(x)                                  # (a gradient arrives on the padding rows too)
    gy[:live] = gw[mine]
    y = norm.batch_norm(x, bn, relu=False, n_live=n_live)
    y.backward(gy)
    xr = torch.cat([x0, x1]).requires_grad_(True)
    yr = ref(xr)
    yr.backward(gw)
    res["static"] = dict(same_rm=_same_on_all_ranks(bn.running_mean), same_rv=_same_on_all_ranks(bn.running_var),
                         rm=bool(torch.allclose(bn.running_mean, ref.running_mean, rtol=1e-4, atol=1e-5)),
                         rv=bool(torch.allclose(bn.running_var, ref.running_var, rtol=1e-4, atol=1e-5)),
                         y=_rel(y[:live], yr[mine]), dx=_rel(x.grad[:live], xr.grad[mine]),
                         padding_zero=bool(not y[live:].any() and not x.grad[live:].any()))
    return res


def _section_no_collective_in_a_graph(rank, dev):
    """(c) StaticTrainingStep refuses a synchronising network at construction."""
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import static
    net = spconv.SparseSequential(spconv.SubMConv3d(8, 16, 3, bias=False), torch.nn.SyncBatchNorm(16),
                                  torch.nn.ReLU()).to(dev).half()
    graphs = []
    real = torch.cuda.CUDAGraph

    class Counted(real):
        def __new__(cls, *a, **k):
            graphs.append(1)
            return super().__new__(cls, *a, **k)

    torch.cuda.CUDAGraph = Counted
    try:
        try:
            static.StaticTrainingStep(net, max_voxels=512, in_channels=8, spatial_shape=[8, 16, 16], batch_size=1,
                                      out_grad=torch.ones((512, 16), dtype=torch.float16, device=dev))
            raised = None
        except RuntimeError as e:
            raised = str(e)
    finally:
        torch.cuda.CUDAGraph = real
    return dict(raised=raised, capturing=bool(torch.cuda.is_current_stream_capturing()), graphs=len(graphs))


def _worker(rank, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=timedelta(seconds=60))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {}
    for name, fn in (("a", _section_path_taken), ("b", _section_empty_and_static),
                     ("c", _section_no_collective_in_a_graph)):
        try:
            res[name] = fn(rank, dev)
        except BaseException:
            res[name] = dict(error=traceback.format_exc())
            break                   # (the other rank's next collective would meet nobody: end here, it times out)
    out[rank] = res
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks(cuda):
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_worker, args=(_free_port(), out), nprocs=WORLD, join=True)
        res = dict(out)
    assert set(res) == set(range(WORLD))
    return res


def _section(ranks, name):
    for rank, res in ranks.items():
        assert name in res, f"rank {rank} never reached section {name}: {res}"
        assert "error" not in res[name], f"rank {rank}:\n{res[name]['error']}"
    return [ranks[r][name] for r in range(WORLD)]


def test_sparse_sequential_takes_the_hip_path_and_the_epilogue_statistics(ranks):
    for r in _section(ranks, "a"):
        print(r)
        # one local_stats call per pass, fed by the convolution's epilogue records: no pass over the rows
        assert len(r["local_stats_calls"]) == 1 and r["local_stats_calls"][0][0] and r["local_stats_calls"][0][1] > 0
        # fp16 rows: 2e-3 of the reference's largest value (tests/test_gpu_norm.py)
        assert r["y"] <= 2e-3 and r["dx"] <= 2e-3, r
        assert max(r["params"]) <= 2e-3, r
        assert r["rm"] and r["rv"] and r["nbt"] == 1


def test_empty_rank_and_static_shape_rank(ranks):
    res = _section(ranks, "b")
    for rank, r in enumerate(res):
        print(r)
        e, s = r["empty"], r["static"]
        assert e["shape"] == ((500, 32) if rank == 0 else (0, 32))
        assert e["same_rm"] and e["same_rv"] and e["rm"] and e["rv"] and e["nbt"] == 1
        assert e["y"] <= 2e-5 and e["dx"] <= 2e-5
        assert e["dw"] <= 1e-4                                 # rank 0: all of the gradient; rank 1: zeros
        assert s["same_rm"] and s["same_rv"] and s["rm"] and s["rv"]
        assert s["y"] <= 2e-5 and s["dx"] <= 2e-5 and s["padding_zero"]


def test_static_training_step_refuses_a_collective(ranks):
    for r in _section(ranks, "c"):
        assert r["raised"] is not None and "collective" in r["raised"], r
        assert not r["capturing"] and r["graphs"] == 0
