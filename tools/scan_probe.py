#!/usr/bin/env python
"""What do the selective scan and the causal convolution over serialised rows cost?  `functional.selective_scan` /
`causal_conv1d_rows` (csrc/scan.hip) against the composite a user writes today: pad the serialised rows to the
channel-first [B, Dm, L] layout (one read-back of the offsets), the torch restatement of `selective_scan_ref` (a Python
loop of L steps, float32) or `F.conv1d`, and un-pad -- alternating in one process.  HIP events, 5 warm-up calls, median of
the repeats.  4 scenes of voxels on [41, 1600, 1408] along a Hilbert curve, f16, G = 1, Dm in {128, 512}:

  full   4 x 100 000 voxels: the native calls, the convolution composite and a bidirectional SerializedMamba(Dm / 2)
         training step; the scan composite's loop is not usable at L = 100 000
  small  4 x 2 048 voxels: the native calls AND both composites -- the size at which the scan composite is timed

For the scan the achieved bytes/s and exp/s come from shape-derived counts (`scan_counts`) and are set against the
machine's peaks (8 TB/s; one exp per lane every fourth cycle: 256 CUs x 16 x 2.4 GHz).

    python tools/scan_probe.py [--out profiles/scan_probe.json] [--repeats 20]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import spconv_amd.pytorch as spconv  # noqa: E402
from serialize_probe import timed  # noqa: E402
from spconv_amd.pytorch import functional as Fsp  # noqa: E402

GRID, BATCH, N, W = [41, 1600, 1408], 4, 16, 4
PEAK_BYTES, PEAK_EXP = 8.0e12, 256 * 16 * 2.4e9


def level(dev, per_scene):
    g = torch.Generator().manual_seed(per_scene)
    cells = torch.stack([torch.randint(0, hi, (BATCH * per_scene,), generator=g) for hi in [BATCH] + GRID], dim=1)
    cells = torch.unique(cells, dim=0).int().to(dev).contiguous()
    x = spconv.SparseConvTensor(torch.zeros((cells.shape[0], 1), device=dev), cells, GRID, BATCH)
    return Fsp.serialize(x, orders=("hilbert",))


def pad(rows, order, off):
    """rows [n, C] -> [B, C, L] along the order (off: the offsets on the host)"""
    srt = rows[order.long()]
    return torch.nn.utils.rnn.pad_sequence([srt[off[b]:off[b + 1]] for b in range(BATCH)], batch_first=True).transpose(1, 2)


def unpad(padded, order, off, n):
    srt = torch.cat([padded[b, :, :off[b + 1] - off[b]].t() for b in range(BATCH)])
    return torch.zeros((n, padded.shape[1]), dtype=padded.dtype, device=padded.device).index_copy(0, order.long(), srt)


def scan_composite(u, delta, A, B, C, D, z, bias, ser):
    off, order, n = ser.offsets.tolist(), ser.order[0], u.shape[0]              # (the read-back)
    up, dp, zp = (pad(t, order, off).float() for t in (u, delta, z))
    Bp, Cp = (pad(t[:, 0], order, off).float() for t in (B, C))
    dp = torch.nn.functional.softplus(dp + bias[None, :, None])
    dA = torch.exp(torch.einsum("bdl,dn->bdln", dp, A))
    dBu = torch.einsum("bdl,bnl,bdl->bdln", dp, Bp, up)
    h, ys = torch.zeros((BATCH, u.shape[1], N), device=u.device), []
    for i in range(up.shape[2]):
        h = dA[:, :, i] * h + dBu[:, :, i]
        ys.append(torch.einsum("bdn,bn->bd", h, Cp[:, :, i]))
    y = (torch.stack(ys, dim=2) + up * D[None, :, None]) * torch.nn.functional.silu(zp)
    return unpad(y.to(u.dtype), order, off, n)


def conv_composite(x, w, b, ser):
    off, order = ser.offsets.tolist(), ser.order[0]
    xp = pad(x, order, off)
    y = torch.nn.functional.conv1d(xp, w[:, None].to(x.dtype), b.to(x.dtype), padding=W - 1, groups=x.shape[1])[..., :xp.shape[2]]
    return unpad(torch.nn.functional.silu(y), order, off, x.shape[0])


def scan_counts(n, Dm, G, eb=2):
    """(forward, backward) x (bytes, exps) from the shapes: row tensors once per walk that reads or writes them, B / C
    once per 64-channel workgroup (forward walks) or per group (backward walk); 16 exps per row, channel and walk"""
    bc = n * G * N * eb
    fwd_bytes = n * Dm * eb * (2 + 3 + 1) + bc * (Dm // G // 64) * 3
    bwd_bytes = n * Dm * eb * (3 + 4 + 3) + bc * (Dm // G // 64) + bc * 4
    return (fwd_bytes, 2 * n * Dm * N), (bwd_bytes, 3 * n * Dm * N)


def probe(dev, repeats):
    res = {"dtype": "f16", "G": 1, "W": W}
    for Dm in (128, 512):
        for tag, per_scene in (("full", 100_000), ("small", 2048)):
            ser = level(dev, per_scene)
            seq, n = Fsp.scan_sequences(ser), int(ser.order.shape[1])
            torch.manual_seed(Dm)
            half = lambda *s: torch.randn(s, device=dev).half().requires_grad_(True)
            u, z, B, C = half(n, Dm), half(n, Dm), half(n, 1, N), half(n, 1, N)
            delta = (torch.rand((n, Dm), device=dev) * 4 - 6).half().requires_grad_(True)
            A = -torch.arange(1, N + 1, device=dev).float().repeat(Dm, 1).requires_grad_(True)
            D, bias = (torch.randn(Dm, device=dev).requires_grad_(True) for _ in range(2))
            w, b = (torch.randn(s, device=dev).requires_grad_(True) for s in ((Dm, W), (Dm,)))
            g = torch.randn((n, Dm), device=dev).half()
            forms = {"scan_native": (lambda: Fsp.selective_scan(u, delta, A, B, C, D, z, bias, True, seq=seq), True),
                     "conv_native": (lambda: Fsp.causal_conv1d_rows(u, w, b, seq=seq, activation="silu"), True),
                     "conv_composite": (lambda: conv_composite(u, w, b, ser), True),
                     "scan_composite": (lambda: scan_composite(u, delta, A, B, C, D, z, bias, ser), tag == "small")}
            entry = {"rows": n}
            with torch.no_grad():
                entry["conv_max_abs_diff"] = float((forms["conv_native"][0]().float() - conv_composite(u, w, b, ser).float()).abs().max())
                if tag == "small":
                    entry["scan_max_abs_diff"] = float((forms["scan_native"][0]().float()
                                                        - forms["scan_composite"][0]().float()).abs().max())
            leaves = (u, delta, A, B, C, D, z, bias, w, b)
            for name, (fn, run) in forms.items():
                if not run:
                    entry[name] = "not measured: a Python loop of 100 000 steps"
                    continue

                def fwd(fn=fn):
                    with torch.no_grad():
                        fn()

                def both(fn=fn):
                    for t in leaves:
                        t.grad = None
                    fn().backward(g)
                few = repeats if "native" in name or "conv" in name else 3
                entry[name] = {"fwd": timed(fwd, few, warmup=2), "fwd_bwd": timed(both, few, warmup=2)}
            (fb, fe), (bb, be) = scan_counts(n, Dm, 1)
            tf = entry["scan_native"]["fwd"]["median_us"] * 1e-6
            tb = entry["scan_native"]["fwd_bwd"]["median_us"] * 1e-6 - tf
            for what, t, nbytes, nexp in (("scan_fwd", tf, fb, fe), ("scan_bwd", tb, bb, be)):
                rates = {"bytes_per_s": nbytes / t, "exp_per_s": nexp / t}
                rates.update(of_peak_bytes=round(rates["bytes_per_s"] / PEAK_BYTES, 3),
                             of_peak_exp=round(rates["exp_per_s"] / PEAK_EXP, 3))
                rates["nearer_bound"] = "exp issue" if rates["of_peak_exp"] > rates["of_peak_bytes"] else "bytes"
                entry[what] = rates
            if tag == "full":
                layer = spconv.SerializedMamba(Dm // 2, bidirectional=True).to(dev).half()
                feats = torch.randn((n, Dm // 2), device=dev).half()
                opt = torch.optim.SGD(layer.parameters(), lr=1e-3)

                def train():
                    opt.zero_grad(set_to_none=True)
                    layer(feats, seq).float().square().mean().backward()
                    opt.step()
                entry["mamba_train_step_native"] = timed(train, repeats, warmup=2)
                entry["mamba_train_step_composite"] = "not measured"
            res[f"Dm{Dm}_{tag}"] = entry
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_probe.json"))
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scan_probe needs the GPU: nothing is measured without one")
    res = {"repeats": args.repeats, "probe": probe(torch.device("cuda:0"), args.repeats)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
