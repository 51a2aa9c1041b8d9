"""CPU: refnorm.py (the float64 reference of the normalisation kernels) against torch.nn.functional.batch_norm + autograd
in float64, and the properties of the magnitudes the GPU bound relies on."""
import numpy as np
import pytest
import torch

import refnorm

TOL = 1e-12


def _close(a, b, name):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.abs(a - b).max(initial=0.0) <= TOL * max(1.0, np.abs(b).max(initial=0.0)), (name, np.abs(a - b).max())


def _data(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g, dtype=torch.float64) * 1.7 + torch.linspace(-3, 3, C, dtype=torch.float64)
    dy = torch.randn(n, C, generator=g, dtype=torch.float64)
    w = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    b = torch.rand(C, generator=g, dtype=torch.float64) - 0.5
    rm = torch.randn(C, generator=g, dtype=torch.float64) * 0.5
    rv = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    return x, dy, w, b, rm, rv


@pytest.mark.parametrize("live", [None, 37, 2])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("training", [True, False])
def test_against_torch_float64(training, relu, affine, live):
    n, C, momentum, eps = 50, 12, 0.3, 1e-3
    x, dy, w, b, rm, rv = _data(n, C, 7 + int(relu) + 2 * int(affine))
    L = n if live is None else live
    x[L:], dy[L:] = 1e4, 1.0                      # padding: read by nothing
    out, A = refnorm.batchnorm(x.numpy(), dy.numpy(), w.numpy() if affine else None, b.numpy() if affine else None,
                               live=live, training=training, relu=relu, momentum=momentum, eps=eps,
                               running_mean=rm.numpy(), running_var=rv.numpy())
    xt = x[:L].clone().requires_grad_(True)
    wt, bt = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    rmt, rvt = rm.clone(), rv.clone()
    pre = torch.nn.functional.batch_norm(xt, rmt, rvt, wt if affine else None, bt if affine else None, training,
                                         momentum, eps)
    y = torch.relu(pre) if relu else pre
    y.backward(dy[:L])
    _close(out["pre"][:L], pre.detach().numpy(), "pre")
    _close(out["y"][:L], y.detach().numpy(), "y")
    _close(out["dx"][:L], xt.grad.numpy(), "dx")
    assert not out["y"][L:].any() and not out["dx"][L:].any()
    if training:
        _close(out["mean"], x[:L].mean(0).numpy(), "mean")
        _close(out["var"], x[:L].var(0, unbiased=False).numpy(), "var")
        _close(out["running_mean"], rmt.numpy(), "running_mean")
        _close(out["running_var"], rvt.numpy(), "running_var")
        _close(out["record"][0], np.full(C, float(L)), "rows")
        _close(out["record"][2], out["var"] * L, "M2")
    else:
        _close(out["mean"], rm.numpy(), "mean")
        _close(out["var"], rv.numpy(), "var")
        assert "running_mean" not in out
    _close(out["invstd"], 1.0 / np.sqrt(out["var"] + eps), "invstd")
    if affine:
        _close(out["dweight"], wt.grad.numpy(), "dweight")
        _close(out["dbias"], bt.grad.numpy(), "dbias")
    else:
        # without affine parameters the kernels still leave the two sums; autograd has no leaf for them
        mask = (pre.detach() > 0).double() if relu else torch.ones_like(pre)
        g = (dy[:L] * mask).numpy()
        _close(out["dbias"], g.sum(0), "dbias")
        _close(out["dweight"], (g * (x[:L].numpy() - out["mean"]) * out["invstd"]).sum(0), "dweight")
    _close(out["sums"], np.stack([out["dbias"], out["dweight"]]), "sums")
    # a magnitude bounds its value, and is the spread -- not the second moment -- for the variance
    for k in ("y", "dx", "dweight", "dbias", "sums", "mean", "invstd"):
        assert (A[k] >= np.abs(out[k]) * (1 - 1e-12)).all(), k
    assert np.array_equal(A["var"], out["var"])


def test_degenerate_row_counts():
    x, dy, w, b, rm, rv = (t.numpy() for t in _data(9, 4, 3))
    for live, rows in ((0, 0), (-3, 0), (1, 1), (20, 9)):
        out, A = refnorm.batchnorm(x, dy, w, b, live=live, relu=True, eps=1e-3, running_mean=rm, running_var=rv)
        assert out["record"][0].tolist() == [float(rows)] * 4
        assert all(np.isfinite(v).all() for v in out.values())
        if rows <= 1:
            assert not out["var"].any() and np.allclose(out["invstd"], 1e-3 ** -0.5)
            assert not out["dx"].any() and not out["y"][rows:].any()
            _close(out["running_var"], 0.9 * rv, "running_var")            # one row: the biased variance, 0
        if rows == 0:
            assert not out["mean"].any() and not out["sums"].any()
            _close(out["running_mean"], 0.9 * rm, "running_mean")


def test_records_merge_to_the_statistics_of_all_rows():
    x = _data(40, 6, 5)[0].numpy()
    sizes = [0, 1, 7, 0, 20, 12, 0]
    stats, at = np.zeros((3, 6, len(sizes))), 0
    for i, s in enumerate(sizes):
        stats[:, :, i] = refnorm.record(x[at:at + s])[0]
        at += s
    rows, mean, M2, A_mean = refnorm.merge_records(stats)
    rec, rec_A = refnorm.record(x)
    _close(rows, rec[0], "rows")
    _close(mean, rec[1], "mean")
    _close(M2, rec[2], "M2")
    assert (A_mean <= rec_A[1] * (1 + 1e-12)).all() and (A_mean >= np.abs(mean) * (1 - 1e-12)).all()
    out, _ = refnorm.batchnorm(x, stats=(rows[0], mean, M2, A_mean), running_mean=np.zeros(6), running_var=np.ones(6))
    ref, _ = refnorm.batchnorm(x, running_mean=np.zeros(6), running_var=np.ones(6))
    for k in ("y", "invstd", "running_mean", "running_var"):
        _close(out[k], ref[k], k)


def test_variance_magnitude_is_the_spread():
    """mean 1e3, spread 1: the magnitude of the variance stays ~1, six orders below the second moment"""
    g = np.random.default_rng(0)
    x = 1e3 + g.standard_normal((500, 2))
    out, A = refnorm.batchnorm(x)
    assert (A["var"] < 1.3).all() and (A["var"] > 0.7).all()
    assert (A["mean"] > 999).all()
