"""fp64 reference of a sparse convolution that builds no rulebook: the pairs come from the coordinates alone.

Each coordinate (batch, *spatial) is encoded as one 64-bit key; the inputs' keys are sorted once and every kernel
offset is a `searchsorted` over them.  Plain torch in float64, on whatever device the inputs live on (the CPU for
small scenes, the GPU for the large ones); nothing of this project's is used.

Conventions (the dense-convolution ones, as torch.nn.functional.conv*d / conv_transpose*d compute them):
  regular    x_in = y_out * s - p + k * d   (outputs: every y that some input reaches, sorted by key)
  transposed y_out = x_in * s - p + k * d   (outputs likewise)
  SubM       x_in = y_out + (k - ksize // 2) * d, outputs = inputs (their own row order; padding is not used)
k runs over the offsets of ksize, last spatial dim fastest; weights are KRSC [K, *ksize, C]."""
from collections import namedtuple

import numpy as np
import torch

RefConv = namedtuple("RefConv", "out_indices out din dW out_abs din_abs dW_abs")


def _as_long(a, device):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a)
    return a.to(device=device, dtype=torch.int64)


def _keys(b, coords, dims):
    """key = ((b * D0 + c0) * D1 + c1) ...: one int64 per coordinate row."""
    key = b.clone()
    for j, dim in enumerate(dims):
        key = key * int(dim) + coords[:, j]
    return key


def _offsets(ksize):
    """[kv, ndim] offsets, last dim fastest (the KRSC weight order)."""
    grids = torch.meshgrid(*[torch.arange(k) for k in ksize], indexing="ij")
    return torch.stack([g.reshape(-1) for g in grids], 1).to(torch.int64)


def out_spatial_shape(spatial_shape, ksize, stride, padding, dilation, subm, transposed=False, out_padding=None):
    if subm:
        return list(spatial_shape)
    out = []
    for i, n in enumerate(spatial_shape):
        if transposed:
            out.append((n - 1) * stride[i] - 2 * padding[i] + ksize[i] + (out_padding[i] if out_padding else 0))
        else:
            out.append((n + 2 * padding[i] - dilation[i] * (ksize[i] - 1) - 1) // stride[i] + 1)
    return out


def pairs(indices, batch_size, spatial_shape, ksize, stride, padding, dilation, subm, transposed=False,
          out_padding=None, device="cpu"):
    """(out_indices [n_out, ndim + 1] int64, pair list [(k, in rows, out rows)] with int64 row tensors)."""
    ndim = len(spatial_shape)
    assert 1 <= ndim <= 4 and len(ksize) == ndim
    idx = _as_long(indices, device)
    n = idx.shape[0]
    b, x = idx[:, 0], idx[:, 1:]
    in_dims = [int(v) for v in spatial_shape]
    out_dims = out_spatial_shape(spatial_shape, ksize, stride, padding, dilation, subm, transposed, out_padding)
    s = torch.tensor(stride, dtype=torch.int64, device=device)
    p = torch.tensor(padding, dtype=torch.int64, device=device)
    d = torch.tensor(dilation, dtype=torch.int64, device=device)
    offs = _offsets(ksize).to(device)
    live = (b >= 0) & (b < batch_size) & ((x >= 0) & (x < torch.tensor(in_dims, device=device))).all(1)
    rows = torch.arange(n, device=device)
    lo_out = torch.zeros(ndim, dtype=torch.int64, device=device)
    hi_out = torch.tensor(out_dims, dtype=torch.int64, device=device)
    cand = []                                   # per offset: (input rows, output coordinates)
    if subm:
        if n == 0:
            return idx, cand
        centre = torch.tensor([k // 2 for k in ksize], dtype=torch.int64, device=device)
        key_in = torch.where(live, _keys(b, x, in_dims), torch.full_like(b, -1))    # (dead rows: key -1, never hit)
        order = torch.argsort(key_in, stable=True)          # (repeated coordinates: the smallest row wins)
        sorted_keys = key_in[order]
        for k in range(offs.shape[0]):
            xin = x + (offs[k] - centre) * d               # the input each output reads through offset k
            ok = live & ((xin >= 0) & (xin < hi_out)).all(1)
            key = _keys(b, xin.clamp(min=0), in_dims)
            pos = torch.searchsorted(sorted_keys, key).clamp(max=max(n - 1, 0))
            hit = ok & (sorted_keys[pos] == key)
            cand.append((k, order[pos[hit]], rows[hit]))
        return idx, cand
    per_k = []
    for k in range(offs.shape[0]):
        if transposed:
            y = x * s - p + offs[k] * d
            ok = live.clone()
        else:
            num = x + p - offs[k] * d
            ok = live & (torch.remainder(num, s) == 0).all(1)
            y = torch.div(num, s, rounding_mode="floor")
        ok &= ((y >= lo_out) & (y < hi_out)).all(1)
        per_k.append((k, rows[ok], _keys(b[ok], y[ok], out_dims)))
    all_keys = torch.cat([t[2] for t in per_k]) if per_k else torch.zeros(0, dtype=torch.int64, device=device)
    out_keys = torch.unique(all_keys, sorted=True)
    for k, r, key in per_k:
        cand.append((k, r, torch.searchsorted(out_keys, key)))
    # decode the sorted keys back to coordinates
    rest = out_keys.clone()
    cols = []
    for dim in reversed(out_dims):
        cols.append(torch.remainder(rest, dim))
        rest = torch.div(rest, dim, rounding_mode="floor")
    out_idx = torch.stack([rest] + cols[::-1], 1) if out_keys.numel() else torch.zeros((0, ndim + 1), dtype=torch.int64,
                                                                                       device=device)
    return out_idx, cand


def _apply(cand, n_in, n_out, f, w, dout):
    """out, din, dW in float64 from the pair list (f [n_in, C], w [K, kv, C], dout [n_out, K] or None)."""
    K, kv, C = w.shape
    out = torch.zeros((n_out, K), dtype=torch.float64, device=f.device)
    din = dw = None
    if dout is not None:
        din = torch.zeros((n_in, C), dtype=torch.float64, device=f.device)
        dw = torch.zeros((K, kv, C), dtype=torch.float64, device=f.device)
    for k, i, o in cand:
        if i.numel() == 0:
            continue
        wk = w[:, k, :]
        out.index_add_(0, o, f[i] @ wk.t())
        if dout is not None:
            g = dout[o]
            din.index_add_(0, i, g @ wk)
            dw[:, k, :] += g.t() @ f[i]
    return out, din, dw


def ref_conv(indices, batch_size, spatial_shape, feats, weight, dout, ksize, stride, padding, dilation, subm,
             transposed=False, out_padding=None):
    """RefConv(out_indices, out, din, dW, out_abs, din_abs, dW_abs): the convolution and its two gradients in float64,
    and the same three on |feats|, |weight|, |dout| (the `A` of util.assert_close_abs_sum).  dout may be None (then
    din, dW and their magnitudes are None).  Runs on feats' device."""
    out_idx, cand = pairs(indices, batch_size, spatial_shape, ksize, stride, padding, dilation, subm, transposed,
                          out_padding, feats.device)
    return conv_from_pairs(out_idx, cand, feats, weight, dout)


def conv_from_pairs(out_idx, cand, feats, weight, dout):
    """ref_conv over pairs() already enumerated (several operand sets over one scene)."""
    dev = feats.device
    f = feats.to(torch.float64)
    K, C = weight.shape[0], weight.shape[-1]
    w = weight.to(device=dev, dtype=torch.float64).reshape(K, -1, C)
    g = None if dout is None else dout.to(device=dev, dtype=torch.float64)
    n_in, n_out = f.shape[0], out_idx.shape[0]
    out, din, dw = _apply(cand, n_in, n_out, f, w, g)
    oa, da, wa = _apply(cand, n_in, n_out, f.abs(), w.abs(), None if g is None else g.abs())
    shape = tuple(weight.shape)
    return RefConv(out_idx, out, din, None if dw is None else dw.reshape(shape), oa, da,
                   None if wa is None else wa.reshape(shape))
