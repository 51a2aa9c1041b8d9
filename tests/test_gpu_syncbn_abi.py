"""GPU: the three entry points SyncBatchNorm is built from (include/spconv_amd.h: spx_batchnorm_local_stats,
spx_batchnorm_bwd_sums, spx_batchnorm_bwd_apply) and the n = 0 merge of spx_batchnorm_fwd_stats, in ONE process: the
ranks are row shards of one matrix, the collectives are a stack (all-gather) and a sum (all-reduce) of what the shards
produced.  The reference is a float64 BatchNorm over all rows at once."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-3, 0.1


def _p(t):
    return None if t is None else t.data_ptr()


def _dt(dtype):
    from spconv_amd import _lib
    return {torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16, torch.float32: _lib.DTYPE_F32}[dtype]


def _ws(L, n, C, dev):
    return torch.empty((max(L.spx_batchnorm_ws_bytes(n, C), 16),), dtype=torch.uint8, device=dev)


def _local_stats(L, x, n_live=None, stats_in=None, n_records=0):
    from spconv_amd import _lib
    n, C = x.shape
    rec = torch.full((3, C), float("nan"), dtype=torch.float32, device=x.device)      # (every field must be written)
    ws = _ws(L, n, C, x.device)
    _lib.check(L.spx_batchnorm_local_stats(x.data_ptr(), n, C, _dt(x.dtype), _p(stats_in), n_records, rec.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _p(n_live),
                                           torch.cuda.current_stream().cuda_stream))
    return rec


def _sync_step(xs, dys, w, b, relu, n_lives=None, recs=None):
    """One SyncBatchNorm step of len(xs) simulated ranks: per rank {y, dx, dw, db, mean, invstd, rm, rv, nbt, rec}."""
    from spconv_amd import _lib
    L = _lib.load()
    dev, C, world, dt = xs[0].device, xs[0].shape[1], len(xs), _dt(xs[0].dtype)
    pdt = _dt(w.dtype)
    stream = torch.cuda.current_stream().cuda_stream
    n_lives = n_lives or [None] * world
    if recs is None:
        recs = [_local_stats(L, x, nl) for x, nl in zip(xs, n_lives)]
    gathered = torch.stack(recs, 0)                                  # the all-gather: [world, 3, C]
    merged = gathered.permute(1, 2, 0).contiguous()                 # [3][C][world]
    total = gathered[:, 0, 0].sum(0, keepdim=True)
    out = []
    for x, nl, rec in zip(xs, n_lives, recs):
        n = x.shape[0]
        r = dict(rec=rec, y=torch.full_like(x, float("nan")), mean=torch.empty(C, device=dev),
                 invstd=torch.empty(C, device=dev), rm=torch.zeros(C, device=dev, dtype=w.dtype),
                 rv=torch.ones(C, device=dev, dtype=w.dtype), nbt=torch.zeros((), dtype=torch.int64, device=dev))
        _lib.check(L.spx_batchnorm_fwd_stats(x.data_ptr(), r["y"].data_ptr(), n, C, dt, _p(w), _p(b), _p(r["rm"]),
                                             _p(r["rv"]), _p(r["nbt"]), pdt, MOMENTUM, EPS, int(relu), _p(r["mean"]),
                                             _p(r["invstd"]), merged.data_ptr(), world, _p(nl), stream))
        out.append(r)
    for x, dy, nl, r in zip(xs, dys, n_lives, out):
        n = x.shape[0]
        r["sums"] = torch.full((2, C), float("nan"), device=dev)
        r["dw"], r["db"] = torch.full_like(w, float("nan")), torch.full_like(b, float("nan"))
        ws = _ws(L, n, C, dev)
        _lib.check(L.spx_batchnorm_bwd_sums(x.data_ptr(), dy.data_ptr(), n, C, dt, _p(w), _p(b), pdt, _p(r["mean"]),
                                            _p(r["invstd"]), int(relu), _p(r["sums"]), _p(r["dw"]), _p(r["db"]),
                                            ws.data_ptr(), ws.numel(), _p(nl), stream))
    sums = torch.stack([r["sums"] for r in out]).sum(0)              # the all-reduce
    for x, dy, nl, r in zip(xs, dys, n_lives, out):
        r["dx"] = torch.full_like(x, float("nan"))
        _lib.check(L.spx_batchnorm_bwd_apply(x.data_ptr(), dy.data_ptr(), r["dx"].data_ptr(), x.shape[0], C, dt, _p(w),
                                             _p(b), pdt, _p(r["mean"]), _p(r["invstd"]), int(relu), sums.data_ptr(),
                                             total.data_ptr(), _p(nl), stream))
    torch.cuda.synchronize()
    return out


def _reference(x, dy, w, b, relu):
    """float64 BatchNorm (+ ReLU) over all rows, on the host: y, dx, dw, db, running_mean, running_var, pre-activation."""
    x64 = x.double().cpu().requires_grad_(True)
    w64, b64 = w.double().cpu().requires_grad_(True), b.double().cpu().requires_grad_(True)
    rm, rv = torch.zeros(x.shape[1], dtype=torch.float64), torch.ones(x.shape[1], dtype=torch.float64)
    pre = torch.nn.functional.batch_norm(x64, rm, rv, w64, b64, True, MOMENTUM, EPS)
    y = torch.relu(pre) if relu else pre
    y.backward(dy.double().cpu())
    return y.detach(), x64.grad, w64.grad, b64.grad, rm, rv, pre.detach()


def _inputs(n, C, dtype, dev, relu, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, C, generator=g) * 1.7 + torch.linspace(-3, 3, C)).to(dtype)
    dy = torch.randn(n, C, generator=g).to(dtype)
    w, b = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    if relu:
        # the derivative of the ReLU does not exist at 0: where the float64 pre-activation is within 1e-4 of it (fp32
        # arithmetic in the kernel resolves ~1e-6) the mask is anyone's choice, so no gradient is sent there
        pre = _reference(x, dy, w, b, False)[6]
        dy = torch.where(pre.abs() < 1e-4, torch.zeros((), dtype=dtype), dy)
    return x.to(dev), dy.to(dev), w.to(dev), b.to(dev)


SHARDS = (0, 1, 333, 666)        # an empty rank, a one-row rank (M2 = 0), uneven counts


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dtype,C,tol", [(torch.float16, 8, 2e-3), (torch.float16, 64, 2e-3),
                                         (torch.bfloat16, 8, 1.6e-2), (torch.bfloat16, 64, 1.6e-2),
                                         (torch.float32, 4, 2e-5), (torch.float16, 264, 2e-3)])
def test_row_shards_match_the_whole_matrix(cuda, dtype, C, tol, relu):
    n = sum(SHARDS)
    x, dy, w, b = _inputs(n, C, dtype, cuda, relu, seed=C + int(relu))
    xs, dys = list(torch.split(x, SHARDS)), list(torch.split(dy, SHARDS))
    out = _sync_step([t.contiguous() for t in xs], [t.contiguous() for t in dys], w, b, relu)
    y_ref, dx_ref, dw_ref, db_ref, rm_ref, rv_ref, _ = _reference(x, dy, w, b, relu)
    scale = lambda t: float(t.abs().max()) + 1e-12
    y = torch.cat([r["y"] for r in out]).double().cpu()
    dx = torch.cat([r["dx"] for r in out]).double().cpu()
    dw = torch.stack([r["dw"] for r in out]).double().sum(0).cpu()
    db = torch.stack([r["db"] for r in out]).double().sum(0).cpu()
    errs = dict(y=float((y - y_ref).abs().max()) / scale(y_ref), dx=float((dx - dx_ref).abs().max()) / scale(dx_ref),
                dw=float((dw - dw_ref).abs().max()) / scale(dw_ref), db=float((db - db_ref).abs().max()) / scale(db_ref))
    print(dtype, C, relu, errs)
    assert errs["y"] <= tol and errs["dx"] <= tol, errs
    assert errs["dw"] <= max(tol, 1e-4) and errs["db"] <= max(tol, 1e-4), errs
    for rows, r in zip(SHARDS, out):
        assert torch.equal(r["rec"][0], torch.full((C,), float(rows), device=cuda)), rows      # exact live-row count
        assert torch.isfinite(r["rec"]).all()
        assert torch.allclose(r["rm"].double().cpu(), rm_ref, rtol=1e-4, atol=1e-5)
        assert torch.allclose(r["rv"].double().cpu(), rv_ref, rtol=1e-4, atol=1e-5)
        assert int(r["nbt"]) == 1
        for k in ("mean", "invstd", "rm", "rv"):        # every rank, the empty one included, holds the same bits
            assert torch.equal(r[k], out[-1][k]), (rows, k)
    # the empty rank's local sums and parameter gradients are zeros, its record one of zero rows
    assert not out[0]["sums"].any() and not out[0]["dw"].any() and not out[0]["db"].any() and not out[0]["rec"].any()
    assert not out[1]["rec"][2].any()                   # one row: no spread


def test_half_parameters_and_buffers(cuda):
    """Parameters / running estimates in the 16-bit dtype of a `.half()` model: read and written in place."""
    n, C = sum(SHARDS), 64
    x, dy, w, b = _inputs(n, C, torch.float16, cuda, False, seed=11)
    dy = dy * 0.01                                       # (keeps the fp16 parameter gradients far from overflow)
    w, b = w.half(), b.half()
    out = _sync_step([t.contiguous() for t in torch.split(x, SHARDS)], [t.contiguous() for t in torch.split(dy, SHARDS)],
                     w, b, False)
    y_ref, dx_ref, dw_ref, db_ref, rm_ref, rv_ref, _ = _reference(x, dy, w, b, False)
    y = torch.cat([r["y"] for r in out]).double().cpu()
    dx = torch.cat([r["dx"] for r in out]).double().cpu()
    assert float((y - y_ref).abs().max()) <= 2e-3 * float(y_ref.abs().max())
    assert float((dx - dx_ref).abs().max()) <= 2e-3 * float(dx_ref.abs().max())
    # fp16 holds 11 bits: a stored vector is within 2^-11 of the float64 value, relative to its size
    half = lambda got, want: float((got.double().cpu() - want).abs().max()) <= 2.0 ** -10 * float(want.abs().max()) + 1e-6
    assert out[0]["rm"].dtype == torch.float16 and out[3]["dw"].dtype == torch.float16
    assert half(out[3]["rm"], rm_ref) and half(out[3]["rv"], rv_ref)
    assert torch.equal(out[0]["rm"], out[3]["rm"]) and torch.equal(out[0]["rv"], out[3]["rv"])
    # each rank rounds its own gradient to fp16 before the sum: one rounding per rank
    dw = torch.stack([r["dw"] for r in out]).double().sum(0).cpu()
    db = torch.stack([r["db"] for r in out]).double().sum(0).cpu()
    assert float((dw - dw_ref).abs().max()) <= 4 * 2.0 ** -11 * float(dw_ref.abs().max()) + 1e-4 * float(dw_ref.abs().max())
    assert float((db - db_ref).abs().max()) <= 4 * 2.0 ** -11 * float(db_ref.abs().max()) + 1e-4 * float(db_ref.abs().max())


def test_epilogue_records_are_merged_and_x_is_not_read(cuda):
    """stats_in: the [3][C][records] layout a convolution epilogue leaves, here built by hand from 7 row blocks."""
    from spconv_amd import _lib
    L = _lib.load()
    n, C = 2000, 16
    x, dy, w, b = _inputs(n, C, torch.float16, cuda, False, seed=5)
    blocks = (300, 1, 0, 512, 187, 700, 300)
    assert sum(blocks) == n
    stats_in = torch.zeros((3, C, len(blocks)), dtype=torch.float64)
    for i, rows in enumerate(torch.split(x.double().cpu(), blocks)):
        if rows.shape[0]:
            stats_in[0, :, i] = rows.shape[0]
            stats_in[1, :, i] = rows.mean(0)
            stats_in[2, :, i] = (rows - rows.mean(0)).square().sum(0)
    stats_in = stats_in.float().to(cuda).contiguous()
    poisoned = torch.full_like(x, float("nan"))
    rec_merge = _local_stats(L, poisoned, stats_in=stats_in, n_records=len(blocks))
    rec_pass = _local_stats(L, x)
    torch.cuda.synchronize()
    assert torch.isfinite(rec_merge).all()
    assert torch.equal(rec_merge[0], torch.full((C,), float(n), device=cuda)) and torch.equal(rec_pass[0], rec_merge[0])
    a = _sync_step([x], [dy], w, b, False, recs=[rec_merge])[0]
    c = _sync_step([x], [dy], w, b, False, recs=[rec_pass])[0]
    y_ref = _reference(x, dy, w, b, False)[0]
    tol = 2e-3 * float(y_ref.abs().max())
    assert float((a["y"].double().cpu() - y_ref).abs().max()) <= tol
    assert float((a["y"].double() - c["y"].double()).abs().max()) <= tol


def test_padding_rows_of_a_static_shape_tensor(cuda):
    """n_live: 300 allocated rows with 200 and 0 live; the padding holds 1e4 and must reach nothing."""
    C, alloc, live = 16, 300, (200, 0)
    x, dy, w, b = _inputs(live[0], C, torch.float16, cuda, True, seed=9)
    xs, dys, nls = [], [], []
    for k in live:
        xp = torch.full((alloc, C), 1e4, dtype=torch.float16, device=cuda)
        gp = torch.ones((alloc, C), dtype=torch.float16, device=cuda)
        xp[:k], gp[:k] = x[:k], dy[:k]
        xs.append(xp)
        dys.append(gp)
        nls.append(torch.tensor([k], dtype=torch.int32, device=cuda))
    out = _sync_step(xs, dys, w, b, True, n_lives=nls)
    y_ref, dx_ref, dw_ref, db_ref, rm_ref, rv_ref, _ = _reference(x, dy, w, b, True)
    x64 = x.double().cpu()
    for k, r in zip(live, out):
        assert torch.equal(r["rec"][0], torch.full((C,), float(k), device=cuda))
        assert torch.allclose(r["mean"].double().cpu(), x64.mean(0), rtol=1e-4, atol=1e-5)
        assert torch.allclose(r["invstd"].double().cpu(), (x64.var(0, unbiased=False) + EPS).rsqrt(), rtol=1e-4, atol=1e-5)
        assert torch.allclose(r["rm"].double().cpu(), rm_ref, rtol=1e-4, atol=1e-5)
        assert torch.allclose(r["rv"].double().cpu(), rv_ref, rtol=1e-4, atol=1e-5)
        assert not r["y"][k:].any() and not r["dx"][k:].any()           # exactly zero, not NaN, on the padding rows
    y, dx = out[0]["y"][:live[0]].double().cpu(), out[0]["dx"][:live[0]].double().cpu()
    assert float((y - y_ref).abs().max()) <= 2e-3 * float(y_ref.abs().max())
    assert float((dx - dx_ref).abs().max()) <= 2e-3 * float(dx_ref.abs().max())
    dw = (out[0]["dw"] + out[1]["dw"]).double().cpu()
    assert float((dw - dw_ref).abs().max()) <= 2e-3 * float(dw_ref.abs().max())


def test_row_limit_is_an_error(cuda):
    """A record counts rows in fp32: more than 2^24 rows are refused on the host, nothing is launched or read."""
    from spconv_amd import _lib
    L = _lib.load()
    rec = torch.zeros((3, 8), device=cuda)
    rc = L.spx_batchnorm_local_stats(None, (1 << 24) + 1, 8, _lib.DTYPE_F16, None, 0, rec.data_ptr(), None, 0, None,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"2^24" in L.spx_last_error()
