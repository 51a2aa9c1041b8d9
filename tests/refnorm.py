"""BatchNorm1d (+ ReLU) over the first `live` rows of an [n, C] matrix, forward and backward, in numpy float64: the plain
restatement csrc/norm.hip is held to (tests/test_gpu_norm_matrix.py), as refconv.py is for the gather-GEMM kernels and
refint8.py for the int8 ones.  Inputs are taken as they are -- the caller rounds them to the kernel's dtype first -- and
nothing here rounds.

Every output comes with its MAGNITUDE A in the sense of util.assert_close_abs_sum: the same formula with every operand
replaced by its absolute value and every subtraction by an addition, i.e. the size of the terms the fp32 arithmetic of the
kernel rounds.  The kernels evaluate xhat = x * invstd + (-mean * invstd) and y = x * sc + (b - mean * sc), sc = w * invstd,
so
    A_xhat = (|x| + |mean|) * invstd                A_y  = (|x| + |mean|) * |sc| + |b|
    A_db   = sum_r |dy'|                            A_dw = sum_r |dy'| * A_xhat          (dy' = dy behind the ReLU mask)
    A_dx   = |w| * invstd * (|dy'| + A_db / rows + A_xhat * A_dw / rows)      (training)     |w| * invstd * |dy'| (eval)
    A_mean = mean_r |x|
The variance is different: M2 = sum_r (x - mean)^2 is a sum of squares, and ITS magnitude is itself -- the spread -- not
mean_r x^2: a kernel that forms E[x^2] - E[x]^2 in fp32 is wrong by u * mean^2, which this magnitude does not forgive
(norm.hip's header: "cancellation is bounded by the spread inside ~400 rows").  invstd = (var + eps)^-1/2 inherits the
relative error of var + eps, whose magnitude is var + eps itself: A_invstd = invstd.

Statistics from elsewhere (records of a convolution epilogue, the other ranks of SyncBatchNorm) enter through `stats`."""
import numpy as np


def _f(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def live_rows(live, n):
    """csrc/norm.hip live_rows: NULL = all rows; clamped to [0, n]"""
    return n if live is None else min(max(int(live), 0), n)


def record(x, live=None):
    """{rows, mean, M2} of the live rows, [3][C], and its magnitude"""
    x = _f(x)
    L = live_rows(live, x.shape[0])
    C = x.shape[1]
    if L == 0:
        return np.zeros((3, C)), np.zeros((3, C))
    xl = x[:L]
    mean = xl.mean(0)
    dev = xl - mean
    M2 = (dev * dev).sum(0)
    return np.stack([np.full(C, float(L)), mean, M2]), np.stack([np.zeros(C), np.abs(xl).mean(0), M2])


def merge_records(stats):
    """Exact merge of [3][C][G] records {rows, mean, M2} (zero-row records carry nothing): rows, mean, M2, A_mean"""
    s = _f(stats)
    cnt, m, M2 = s[0], s[1], s[2]
    rows = cnt.sum(1)
    safe = np.where(rows > 0, rows, 1.0)
    mean = (cnt * m).sum(1) / safe
    tot = M2.sum(1) + (cnt * (m - mean[:, None]) ** 2).sum(1)
    return rows, mean, tot, (cnt * np.abs(m)).sum(1) / safe


def batchnorm(x, dy=None, weight=None, bias=None, live=None, training=True, relu=False, momentum=0.1, eps=1e-5,
              running_mean=None, running_var=None, stats=None):
    """-> (out, A): dicts of the outputs and of their magnitudes, same keys.

    training: batch statistics of the live rows, or `stats` = (rows, mean, M2, A_mean) given from outside (rows a scalar:
    all the rows the statistics were taken over, which is also what the backward pass divides by); biased variance to
    normalise, unbiased for running_var.  Evaluation: running_mean / running_var normalise, dx = w * invstd * dy'.
    Rows from `live` on are padding: y and dx are zero there and nothing reads them.
    Keys: y pre mean var invstd [running_mean running_var record] and with dy: dx dweight dbias sums, plus xhat and dyp
    (the masked gradient) for callers that sum over row ranges of their own."""
    x = _f(x)
    n, C = x.shape
    L = live_rows(live, n)
    xl = x[:L]
    w = np.ones(C) if weight is None else _f(weight)
    b = np.zeros(C) if bias is None else _f(bias)
    out, A = {}, {}
    if training:
        if stats is None:
            rec, rec_A = record(x, L)
            rows, mean, M2, A_mean = float(L), rec[1], rec[2], rec_A[1]
        else:
            rows, mean, M2, A_mean = float(stats[0]), _f(stats[1]), _f(stats[2]), _f(stats[3])
        var = M2 / rows if rows > 0 else np.zeros(C)
        unbiased = M2 / (rows - 1) if rows > 1 else var
        out["record"] = np.stack([np.full(C, rows), mean, M2])
        A["record"] = np.stack([np.zeros(C), A_mean, M2])
        if running_mean is not None:
            out["running_mean"] = (1 - momentum) * _f(running_mean) + momentum * mean
            A["running_mean"] = abs(1 - momentum) * np.abs(_f(running_mean)) + momentum * A_mean
        if running_var is not None:
            out["running_var"] = (1 - momentum) * _f(running_var) + momentum * unbiased
            A["running_var"] = abs(1 - momentum) * np.abs(_f(running_var)) + momentum * unbiased
    else:
        rows, mean, var = float(L), _f(running_mean), _f(running_var)
        A_mean = np.abs(mean)
    invstd = 1.0 / np.sqrt(var + eps)
    out.update(mean=mean, var=var, invstd=invstd)
    A.update(mean=A_mean, var=var, invstd=invstd)
    sc = w * invstd
    pre, A_y = np.zeros((n, C)), np.zeros((n, C))
    pre[:L] = xl * sc + (b - mean * sc)
    A_y[:L] = (np.abs(xl) + np.abs(mean)) * np.abs(sc) + np.abs(b)
    out["pre"], A["pre"] = pre, A_y
    out["y"], A["y"] = (np.maximum(pre, 0.0) if relu else pre), A_y
    if dy is None:
        return out, A
    xhat = (xl - mean) * invstd
    A_xhat = (np.abs(xl) + np.abs(mean)) * invstd
    dyp = _f(dy)[:L] * (pre[:L] > 0) if relu else _f(dy)[:L]
    adyp = np.abs(dyp)
    db, dw = dyp.sum(0), (dyp * xhat).sum(0)
    A_db, A_dw = adyp.sum(0), (adyp * A_xhat).sum(0)
    out.update(dbias=db, dweight=dw, sums=np.stack([db, dw]), xhat=xhat, dyp=dyp)
    A.update(dbias=A_db, dweight=A_dw, sums=np.stack([A_db, A_dw]), xhat=A_xhat, dyp=adyp)
    dx, A_dx = np.zeros((n, C)), np.zeros((n, C))
    if training:
        inv_n = 1.0 / rows if rows > 0 else 0.0
        dx[:L] = w * invstd * (dyp - db * inv_n - xhat * (dw * inv_n))
        A_dx[:L] = np.abs(w) * invstd * (adyp + A_db * inv_n + A_xhat * (A_dw * inv_n))
    else:
        dx[:L] = w * invstd * dyp
        A_dx[:L] = np.abs(w) * invstd * adyp
    out["dx"], A["dx"] = dx, A_dx
    return out, A
