#!/usr/bin/env python
"""SyncBatchNorm (+ ReLU): the launches one rank issues per layer on the kernels of csrc/norm.hip against the aten
sequence torch.nn.SyncBatchNorm issues.  One process, no process group: the collective between the two halves of each
direction is the same on both sides and is not timed; the gathered statistics of a two-rank group are a fixed tensor.

  forward   ours   spx_batchnorm_local_stats (pass over the rows + record merge) -> spx_batchnorm_fwd_stats (merge of
                   the ranks' records + running estimates + apply with the ReLU fused)
            torch  batch_norm_stats -> batch_norm_gather_stats_with_counts -> batch_norm_elemt -> relu
  backward  ours   spx_batchnorm_bwd_sums -> spx_batchnorm_bwd_apply (ReLU mask fused)
            torch  batch_norm_backward_reduce -> batch_norm_backward_elemt (no ReLU backward: one launch in torch's favour)

fp16 at 400k x 16, 200k x 32, 100k x 64, 50k x 128, 20k x 512.  Device events around hipGraph replays after a warm-up;
every replay walks S sets of {x, y, dy, dx} (> 256 MiB together) so that no call finds its rows in the Infinity Cache;
the two variants alternate inside every round.  Each figure is the median of R rounds with its min .. max spread.

    python tools/bench_syncbn.py [--rounds 9] [--out profiles/syncbn_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from spconv_amd import _lib                                   # noqa: E402

SHAPES = ((400_000, 16), (200_000, 32), (100_000, 64), (50_000, 128), (20_000, 512))
EPS, MOMENTUM, WORLD = 1e-3, 0.1, 2


def graph_us(fn, span, reps):
    """device time per call of fn(0) .. fn(span - 1) captured into one graph, over `reps` replays"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(span):
            fn(i)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(span):
            fn(i)
    g.replay()
    torch.cuda.synchronize()

    def timed():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / (reps * span)
    return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "syncbn_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_syncbn needs the GPU")
    L = _lib.load()
    dev = torch.device("cuda:0")
    F16, F32 = _lib.DTYPE_F16, _lib.DTYPE_F32
    res = {"rounds": args.rounds, "dtype": "f16", "world": WORLD, "cases": {}}
    for n, C in SHAPES:
        mb = n * C * 2 / 1e6
        S = max(4, int(300e6 // (4 * n * C * 2)) + 1)                # sets of four matrices, > 256 MiB together
        x = [(torch.randn((n, C), device=dev) * 1.5 + 0.3).half() for _ in range(S)]
        dy = [torch.randn((n, C), device=dev).half() for _ in range(S)]
        y = [torch.empty_like(t) for t in x]
        dx = [torch.empty_like(t) for t in x]
        w, b = torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) - 0.5
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        ws = torch.empty((L.spx_batchnorm_ws_bytes(n, C),), dtype=torch.uint8, device=dev)
        record = torch.empty((3, C), device=dev)
        mean, invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
        sums = torch.empty((2, C), device=dev)
        dw, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        stream = lambda: torch.cuda.current_stream().cuda_stream
        # what the all-gather would deliver: this rank's record and a second rank's (the same rows)
        _lib.check(L.spx_batchnorm_local_stats(x[0].data_ptr(), n, C, F16, None, 0, record.data_ptr(), ws.data_ptr(),
                                               ws.numel(), None, stream()))
        gathered = torch.stack([record, record], 0)
        merged = gathered.permute(1, 2, 0).contiguous()
        total = gathered[:, 0, 0].sum(0, keepdim=True)
        _lib.check(L.spx_batchnorm_fwd_stats(x[0].data_ptr(), y[0].data_ptr(), n, C, F16, w.data_ptr(), b.data_ptr(),
                                             rm.data_ptr(), rv.data_ptr(), None, F32, MOMENTUM, EPS, 1, mean.data_ptr(),
                                             invstd.data_ptr(), merged.data_ptr(), WORLD, None, stream()))
        t_mean, t_invstd = torch.batch_norm_stats(x[0], EPS)
        mean_all, invstd_all = torch.stack([t_mean, t_mean]), torch.stack([t_invstd, t_invstd])
        counts = torch.full((WORLD,), float(n), device=dev)
        count_i32 = counts.to(torch.int32)
        sum_dy, sum_dy_xmu, _, _ = torch.batch_norm_backward_reduce(dy[0], x[0], t_mean, t_invstd, w, True, True, True)

        def ours_fwd(i):
            k = i % S
            _lib.check(L.spx_batchnorm_local_stats(x[k].data_ptr(), n, C, F16, None, 0, record.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), None, stream()))
            _lib.check(L.spx_batchnorm_fwd_stats(x[k].data_ptr(), y[k].data_ptr(), n, C, F16, w.data_ptr(), b.data_ptr(),
                                                 rm.data_ptr(), rv.data_ptr(), None, F32, MOMENTUM, EPS, 1,
                                                 mean.data_ptr(), invstd.data_ptr(), merged.data_ptr(), WORLD, None,
                                                 stream()))

        def torch_fwd(i):
            k = i % S
            m, s = torch.batch_norm_stats(x[k], EPS)
            gm, gs = torch.batch_norm_gather_stats_with_counts(x[k], mean_all, invstd_all, rm, rv, MOMENTUM, EPS, counts)
            return torch.relu(torch.batch_norm_elemt(x[k], w, b, gm, gs, EPS)), m, s

        def ours_bwd(i):
            k = i % S
            _lib.check(L.spx_batchnorm_bwd_sums(x[k].data_ptr(), dy[k].data_ptr(), n, C, F16, w.data_ptr(), b.data_ptr(),
                                                F32, mean.data_ptr(), invstd.data_ptr(), 1, sums.data_ptr(),
                                                dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), None, stream()))
            _lib.check(L.spx_batchnorm_bwd_apply(x[k].data_ptr(), dy[k].data_ptr(), dx[k].data_ptr(), n, C, F16,
                                                 w.data_ptr(), b.data_ptr(), F32, mean.data_ptr(), invstd.data_ptr(), 1,
                                                 sums.data_ptr(), total.data_ptr(), None, stream()))

        def torch_bwd(i):
            k = i % S
            a, c, gw, gb = torch.batch_norm_backward_reduce(dy[k], x[k], t_mean, t_invstd, w, True, True, True)
            return torch.batch_norm_backward_elemt(dy[k], x[k], t_mean, t_invstd, w, sum_dy, sum_dy_xmu, count_i32), gw, gb

        reps = max(3, 200 // S)
        case = {"tensor_MB": round(mb, 1), "sets_rotated": S}
        for direction, ours, theirs in (("fwd", ours_fwd, torch_fwd), ("bwd", ours_bwd, torch_bwd)):
            timers = {"hip": graph_us(ours, S, reps), "aten": graph_us(theirs, S, reps)}
            samples = {v: [] for v in timers}
            for _ in range(args.rounds):
                for v, tm in timers.items():            # alternating
                    samples[v].append(tm())
            out = {v: {"us": round(statistics.median(s), 2), "min": round(min(s), 2), "max": round(max(s), 2),
                       "spread_pct": round(100 * (max(s) - min(s)) / statistics.median(s), 1)} for v, s in samples.items()}
            out["hip_over_aten"] = round(out["hip"]["us"] / out["aten"]["us"], 3)
            case[direction] = out
            print(f"[bench_syncbn] {n} x {C} {direction}: {out}", file=sys.stderr, flush=True)
        res["cases"][f"{n}x{C}"] = case
        del x, y, dy, dx
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
