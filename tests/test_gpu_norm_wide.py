"""BatchNorm1d (+ fused ReLU) beyond 256 channels: csrc/norm.hip runs its row-streaming kernels over column blocks of 256
channels (the last may be narrower).

1. against torch.nn.BatchNorm1d in fp32, protocol and tolerances of test_gpu_norm.test_batchnorm_training_matches_torch
   (each channel's arithmetic is the 256-wide kernel's; neither a channel's statistic nor its error depends on how many
   other channels the row has, so the tolerances carry over);
2. bit identity with the <= 256 kernels on contiguous copies of the column blocks (no tolerance);
3. static-shape tensors: statistics over the live rows, zeros in the padding rows;
4. SparseSequential: Conv(64 -> 512) + BatchNorm1d + ReLU takes the fused path, the convolution's statistics sink stays empty;
5. a captured training step through a 512-wide Conv-BN-ReLU stage."""
import copy

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
KT = 256                                     # channels of a column block (kT of csrc/norm.hip)


def _bn(C, dev, eps=1e-3, momentum=0.01, seed=0):
    torch.manual_seed(seed)
    bn = nn.BatchNorm1d(C, eps=eps, momentum=momentum).to(dev)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-0.3, 0.3)
        bn.running_var.uniform_(0.5, 1.5)
    return bn


# ------------------------------------------------------------------ 1. against torch in fp32
@pytest.mark.parametrize("dtype,tol", [(F32, 2e-5), (F16, 2e-3), (BF16, 1.6e-2)])
@pytest.mark.parametrize("n,C", [(25_000, 512), (7_777, 384), (300, 320), (3_001, 1024), (64, 2048)])
@pytest.mark.parametrize("relu", [False, True])
def test_wide_batchnorm_training_matches_torch(cuda, dtype, tol, n, C, relu):
    from spconv_amd.pytorch import norm
    from test_gpu_norm import _ref
    torch.manual_seed(n + C)
    x = (torch.randn(n, C, device=cuda) * 1.7 + torch.linspace(-3, 3, C, device=cuda)).to(dtype)
    dy = torch.randn(n, C, device=cuda).to(dtype)
    bn = nn.BatchNorm1d(C, eps=1e-3, momentum=0.01).to(cuda)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    ref = copy.deepcopy(bn).float()
    xg = x.clone().requires_grad_(True)
    assert norm.supported(x, bn)
    y = norm.batch_norm(xg, bn, relu=relu)
    y.backward(dy)
    y_ref, dx_ref, dw_ref, db_ref = _ref(ref, x.float(), dy.float(), relu)
    scale = lambda t: float(t.abs().max()) + 1e-12
    errs = {"y": float((y.float() - y_ref).abs().max()) / scale(y_ref),
            "dx": float((xg.grad.float() - dx_ref).abs().max()) / scale(dx_ref),
            "dw": float((bn.weight.grad - dw_ref).abs().max()) / scale(dw_ref),
            "db": float((bn.bias.grad - db_ref).abs().max()) / scale(db_ref)}
    print(f"wide-bn n={n} C={C} {dtype} relu={relu}: {errs}")
    assert errs["y"] <= tol and errs["dx"] <= tol
    assert errs["dw"] <= max(tol, 1e-4) and errs["db"] <= max(tol, 1e-4)
    assert torch.allclose(bn.running_mean, ref.running_mean, rtol=1e-4, atol=1e-5)
    assert torch.allclose(bn.running_var, ref.running_var, rtol=1e-4, atol=1e-5)
    assert int(bn.num_batches_tracked) == 1


# ------------------------------------------------------------------ 2. bit identity with the column slices
def _slice_bn(bn, blk, dev):
    """a BatchNorm1d holding the parameters and running estimates of `bn` on the channels `blk`"""
    sub = nn.BatchNorm1d(blk.stop - blk.start, eps=bn.eps, momentum=bn.momentum).to(dev)
    with torch.no_grad():
        sub.weight.copy_(bn.weight[blk])
        sub.bias.copy_(bn.bias[blk])
        sub.running_mean.copy_(bn.running_mean[blk])
        sub.running_var.copy_(bn.running_var[blk])
    return sub.train(bn.training)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("n,C,dtype", [
    (n, C, dt) for n, C in [(25_000, 512), (7_777, 384), (3_001, 320), (5_003, 264), (300, 1024)]
    for dt in (F16, BF16, F32) if not (C == 264 and dt == F32)])      # (tail blocks: 128, 64, 8 channels -- 8: one 16-bit piece)
def test_wide_batchnorm_is_bit_identical_to_its_column_slices(cuda, n, C, dtype, relu, training):
    from spconv_amd.pytorch import norm
    torch.manual_seed(n * 3 + C)
    x = (torch.randn(n, C, device=cuda) * 1.7 + torch.linspace(-3, 3, C, device=cuda)).to(dtype)
    dy = torch.randn(n, C, device=cuda).to(dtype)
    bn = _bn(C, cuda, seed=C).train(training)
    subs = [(blk, _slice_bn(bn, blk, cuda)) for blk in (slice(c, min(c + KT, C)) for c in range(0, C, KT))]
    assert norm.supported(x, bn)
    xg = x.clone().requires_grad_(True)
    y = norm.batch_norm(xg, bn, relu=relu)
    saved = [t.clone() for t in y.grad_fn.saved_tensors[3:5]]          # mean, 1 / std (fp32)
    y.backward(dy)
    assert len(subs) == (C + KT - 1) // KT and subs[-1][0].stop == C
    for blk, sub in subs:
        xs = x[:, blk].contiguous().requires_grad_(True)
        assert norm.supported(xs, sub)
        ys = norm.batch_norm(xs, sub, relu=relu)
        saved_s = [t.clone() for t in ys.grad_fn.saved_tensors[3:5]]
        ys.backward(dy[:, blk].contiguous())
        at = f"channels {blk.start}:{blk.stop}"
        assert torch.equal(y[:, blk], ys), at
        assert torch.equal(xg.grad[:, blk], xs.grad), at
        assert torch.equal(bn.weight.grad[blk], sub.weight.grad), at
        assert torch.equal(bn.bias.grad[blk], sub.bias.grad), at
        assert torch.equal(bn.running_mean[blk], sub.running_mean), at
        assert torch.equal(bn.running_var[blk], sub.running_var), at
        assert torch.equal(saved[0][blk], saved_s[0]) and torch.equal(saved[1][blk], saved_s[1]), at
        assert int(bn.num_batches_tracked) == int(sub.num_batches_tracked) == (1 if training else 0)
    assert bool(torch.isfinite(y.float()).all()) and float(y.float().abs().max()) > 0
    assert float(xg.grad.float().abs().max()) > 0


# ------------------------------------------------------------------ 3. static-shape tensors
@pytest.mark.parametrize("dtype,tol", [(F32, 2e-5), (F16, 2e-3)])
@pytest.mark.parametrize("n,live,C", [(20_000, 13_337, 512), (5_000, 1, 384), (3_000, 0, 512)])
@pytest.mark.parametrize("relu", [False, True])
def test_wide_batchnorm_over_the_live_rows_of_a_static_tensor(cuda, dtype, tol, n, live, C, relu):
    from spconv_amd.pytorch import norm
    torch.manual_seed(n + live + C)
    x = (torch.randn(n, C, device=cuda) * 1.3 + torch.linspace(-2, 2, C, device=cuda)).to(dtype)
    x[live:] = 1000.0                              # junk in the padding must not reach the statistics
    dy = torch.randn(n, C, device=cuda).to(dtype)
    bn = nn.BatchNorm1d(C, eps=1e-3, momentum=0.1).to(cuda)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    ref = copy.deepcopy(bn)
    n_live = torch.tensor([live], dtype=torch.int32, device=cuda)
    xg = x.clone().requires_grad_(True)
    y = norm.batch_norm(xg, bn, relu=relu, n_live=n_live)
    y.backward(dy)
    assert not bool(y[live:].any()) and not bool(xg.grad[live:].any())
    if live <= 1:
        return                                     # (torch refuses one value per channel; the zeros are the claim)
    xr = x[:live].clone().requires_grad_(True)
    yr = norm.batch_norm(xr, ref, relu=relu)       # the same kernels on the live rows alone
    yr.backward(dy[:live])
    scale = float(yr.float().abs().max())
    assert float((y[:live].float() - yr.float()).abs().max()) <= tol * max(scale, 1.0)
    assert float((xg.grad[:live].float() - xr.grad.float()).abs().max()) <= tol * max(float(xr.grad.float().abs().max()), 1.0)
    for a, b in ((bn.weight.grad, ref.weight.grad), (bn.bias.grad, ref.bias.grad),
                 (bn.running_mean, ref.running_mean), (bn.running_var, ref.running_var)):
        assert float((a.float() - b.float()).abs().max()) <= 1e-3 * max(float(b.float().abs().max()), 1.0)
    # ... and against torch on the live rows in fp32 (the tolerances of case 1)
    r32 = nn.BatchNorm1d(C, eps=1e-3, momentum=0.1).to(cuda)
    with torch.no_grad():
        r32.weight.copy_(ref.weight)
        r32.bias.copy_(ref.bias)
    yt = r32(x[:live].float())
    yt = torch.relu(yt) if relu else yt
    assert float((y[:live].float() - yt).abs().max()) <= tol * float(yt.abs().max())


# ------------------------------------------------------------------ 4. SparseSequential
@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_sparse_sequential_takes_the_fused_path_at_512(cuda, monkeypatch, dtype):
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import norm, ops
    from util import scene
    shape, bs, C, K = [16, 16, 16], 2, 64, 512
    idx = torch.from_numpy(scene(shape, 1500, bs, 4)).to(cuda)
    torch.manual_seed(11)
    seq = spconv.SparseSequential(spconv.SubMConv3d(C, K, 3, bias=False, indice_key="m"), nn.BatchNorm1d(K),
                                  nn.ReLU()).to(cuda, dtype).train()
    one = copy.deepcopy(seq)
    f = (torch.rand((idx.shape[0], C), device=cuda) * 2 - 1).to(dtype)
    calls, sinks = [], []
    orig = norm.batch_norm

    def spy(*a, **k):
        calls.append(k.get("relu"))
        sinks.append(k.get("stats"))
        return orig(*a, **k)
    monkeypatch.setattr(norm, "batch_norm", spy)
    got = seq(spconv.SparseConvTensor(f, idx, shape, bs))
    assert calls == [True]                          # BatchNorm + ReLU: one call of the streaming kernels
    assert all(s is None or s.records is None for s in sinks)      # the wide convolution left no records
    monkeypatch.setattr(norm, "batch_norm", orig)
    with ops.collect_bn_stats() as sink:
        y = one[0](spconv.SparseConvTensor(f, idx, shape, bs))
    assert sink.records is None and sink.count == 0
    assert norm.supported(y.features, one[1])
    z = norm.batch_norm(y.features, one[1], relu=True)
    assert torch.equal(got.features, z)
    assert torch.equal(seq[1].running_mean, one[1].running_mean) and torch.equal(seq[1].running_var, one[1].running_var)
    assert float(got.features.detach().float().abs().max()) > 0 and bool((got.features >= 0).all())
    # ... and it is BatchNorm + ReLU: against torch's layers on the convolution's output
    ref = copy.deepcopy(one[1]).float()
    want = torch.relu(ref(y.features.detach().float()))
    tol = 2e-3 if dtype == F16 else 2e-5            # (the tolerances of case 1)
    assert float((got.features.detach().float() - want).abs().max()) <= tol * float(want.abs().max())


# ------------------------------------------------------------------ 5. captured training
def test_captured_training_step_with_batchnorm_at_512(cuda):
    """test_gpu_wide.test_captured_training_step_with_a_512_wide_stage with the network a backbone has: BatchNorm1d +
    ReLU behind the 512-wide convolutions (norm512 = True).  Same scenes, bounds and criteria."""
    import spconv_amd.pytorch as spconv
    from spconv_amd import _lib
    from spconv_amd.pytorch.static import StaticTrainingStep, strided_layers
    from test_gpu_static import _scene_tensors
    from test_gpu_wide import _generic, _wide_backbone
    L = _lib.load()
    shape, bs, C, dtype = [32, 40, 40], 2, 8, F16
    net = _wide_backbone(spconv, C, cuda, dtype, norm512=True).train()
    assert sum(isinstance(m, nn.BatchNorm1d) and m.num_features == 512 for m in net.modules()) == 2
    eager = copy.deepcopy(net)
    names = list(strided_layers(net))
    g0 = ((torch.rand((1_700, 512), device=cuda) - 0.5) * 0.2).half()
    g = g0.clone()
    scenes = [_scene_tensors(shape, n, bs, C, seed, cuda, dtype) for n, seed in ((4000, 1), (1500, 2), (5500, 3))]
    gen0 = _generic(L, dtype)
    step = StaticTrainingStep(net, 12_000, C, shape, bs, dtype, bounds={names[0]: 13_000, names[1]: 1_700},
                              out_grad=g, input_grad=True, example=scenes[0])
    for f, idx in scenes:
        eager.zero_grad(set_to_none=True)
        fe = f.clone().requires_grad_(True)
        ye = eager(spconv.SparseConvTensor(fe, idx, shape, bs))
        n_out = ye.features.shape[0]
        ye.features.backward(g0[:n_out])
        g.copy_(g0)
        g[n_out:] = 0
        out = step(f, idx)
        assert step.overflowed() == {}
        assert int(out.n_live_dev) == n_out and torch.equal(out.indices[:n_out], ye.indices)
        assert out.features.shape[1] == 512
        assert not bool(out.features[n_out:].any())         # BatchNorm + ReLU zero the padding rows themselves
        err = float((out.features[:n_out].float() - ye.features.detach().float()).abs().max())
        print(f"captured 512-wide BN stage: n_out={n_out} err/max={err / float(ye.features.detach().float().abs().max()):.3e}")
        assert err <= 2e-2 * float(ye.features.detach().float().abs().max()), err
        for (name, pa), pb in zip(net.named_parameters(), eager.parameters()):
            rel = float((pa.grad.float() - pb.grad.float()).norm() / pb.grad.float().norm().clamp_min(1e-12))
            print(f"  {name}: {rel:.3e}")
            assert rel < 3e-2, (name, rel)
        rel = float((step.features.grad[:f.shape[0]].float() - fe.grad.float()).norm() / fe.grad.float().norm())
        print(f"  input gradient: {rel:.3e}")
        assert rel < 3e-2, rel
    assert _generic(L, dtype) == gen0
