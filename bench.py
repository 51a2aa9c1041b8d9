#!/usr/bin/env python
"""Benchmark of the hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--config 2|2b|3|4|5] [--full] [--dump-outputs DIR]

A plain run sets up, runs W warm-up steps, times exactly K steps, and prints one JSON line (`value`,
`ms_per_step` = milliseconds per timed step, ...).  `--full` adds the side figures described below
(rooflines, kernel groups, eager and alternative-schedule loops, CPU baselines, the `also` block of
the other configurations).  `--dump-outputs DIR` writes what the last timed step computed (configs
2 / 2b) as DIR/<name>.npy in float32; the inputs are seeded, so two builds can be compared array by array.

With N > 1 and no WORLD_SIZE in the environment the script re-launches itself under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1`, one rank
per GPU (RCCL); under an existing launcher it reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*.

Configurations (BASELINE.json `configs`; SURVEY.md section 8d gives the concrete inputs):

  2   (default, the headline) one 3x3x3 SubMConv3d, C = 64 -> 64, fp16, 100 000 uniform-random
      voxels in 1600x1280x40; step = forward + backward (dgrad + wgrad), rulebook reused through
      `indice_key` (docs/USAGE.md:104-105) and timed separately (`rulebook_ms`).
  2b  the same layer on the coordinates of the reference's real-LiDAR fixture
      (test/data/test_spconv.pkl -> tests/golden/lidar_scene.npz: 125 562 voxels, 6.28 pairs/voxel).
  3   SparseConv3d k3 s2 p1 chain 16 -> 32 -> 64 -> 128, fp16, forward + backward, fresh rulebooks
      every step (a new scene per step, as in training) on the 2b coordinates.
  4   SECOND-style VoxelNet backbone (BatchNorm + ReLU), fp16, 4 LiDAR-density scenes of 100 k
      voxels per GPU (batch 32 over 8 GPUs), forward + backward + one flat-bucket RCCL all-reduce.
  5   int8 SubMConv3d 3x3x3 C = 128 -> 128, 200 000 voxels, per-channel scale + bias + ReLU,
      inference forward only.

Memory level.  A step's working set at config 2 (~88 MB) fits the 256 MiB Infinity Cache, so
replaying ONE scene measures an L3-resident loop, not HBM.  The timed loop therefore ROTATES
over `--scenes` distinct scenes (default 8: ~700 MB, every tensor of a scene has been evicted
by the time it is touched again) -- `value`, `ms_per_step` and `roofline` (= `roofline_cold`)
are from that loop; the single-scene (Infinity-Cache-resident) numbers are reported next to
them as `warm` / `roofline_warm`.  Inputs are resident in HBM before the timed region.

One JSON line is printed by rank 0.  `roofline.achieved` = algorithmic bytes of
the slowest kernel group / its device time, measured live with HIP events on the launch stream;
`roofline.traffic` is the PMC figure of the committed rocprofv3 passes (profiles/traffic.json,
builder-run; null when the configuration has none on file).  `cpu_baseline` times the CPU
oracle (a restatement of the reference's ConvAlgo.Native CPU path, oracle/) on a bounded sample
at N = 1.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SHAPE = [40, 1280, 1600]       # z, y, x (KITTI-shape, SURVEY.md section 8d cfg 2)
# hipGraph captures in this script run in THREAD-LOCAL error mode: at N > 1 the process group is up while rank 0
# still captures kernel-group timing graphs, and RCCL's watchdog thread polls its work events (hipEventQuery) at any
# time -- under the default global mode that poll fails with "operation not permitted when stream is capturing" and
# takes the process down (seen with BENCH_SOLO_DIST=1 on the real backend; gloo has no such thread)
CAPTURE_MODE = "thread_local"
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 achievable
METRIC = "active-voxels/sec fwd+bwd, 3x3x3 SubMConv3d C=64, ~100k voxels/scene"


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--config", choices=["2", "2b", "3", "4", "4i", "5"], default="2")
    ap.add_argument("--voxels", type=int, default=None, help="voxels per scene (config default if unset)")
    ap.add_argument("--channels", type=int, default=None)
    ap.add_argument("--scene", choices=["uniform", "lidar", "fixture"], default=None,
                    help="coordinate source (config default if unset)")
    ap.add_argument("--dtype", choices=["f16", "bf16", "f32"], default="f16")
    ap.add_argument("--scenes", type=int, default=8,
                    help="distinct scenes the timed loop rotates over (cold = HBM-resident working set); "
                         "1 = replay one scene (Infinity-Cache-resident)")
    ap.add_argument("--cold", action="store_true", help="alias of the default (--scenes >= 4 enforced)")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of hipGraph replay")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-also", action="store_true",
                    help="config 2 at N = 1 only: skip the compact block of the other configurations")
    ap.add_argument("--sort", choices=["auto", "on", "off"], default="auto",
                    help="row order of the rulebook tables: auto = the layer modules' default (density-aware rows "
                         "layout built on the device inside the rulebook build), on = the reference's explicit mask "
                         "sort (SPCONV_DO_SORT=1), off = input order (SPCONV_DO_SORT=0)")
    ap.add_argument("--prewarm", type=int, default=0,
                    help="untimed steps run BEFORE the contract's W warm-up steps (clock ramp, allocator and cache "
                         "state).  0 = none: `value` is W warm-up steps + K timed steps and nothing else; the "
                         "pre-warmed figure of round 4 is the side field `round4_protocol`")
    ap.add_argument("--key-order", action="store_true",
                    help="configs 3 / 4 / 4i: the scenes' voxels are handed over in ascending coordinate-key order (what "
                         "spconv_amd.pytorch.utils.sort_voxels_by_coordinate gives a data loader) and the captured pass "
                         "declares it (key_ordered_input=True): level 1 builds its rulebook from a rank map, not a hash table")
    ap.add_argument("--graph-steps", type=int, default=8,
                    help="steps captured per hipGraph (a replay boundary costs ~5 us): 8 at EVERY N, so that the first "
                         "step of a scaling curve measures the gradient exchange, not a change of graph shape")
    ap.add_argument("--full", action="store_true",
                    help="also the side figures: CPU baselines (all configurations) and, at configs 2 / 2b, the "
                         "per-kernel-group times and rooflines, the eager step, the rulebook build, the round-4, "
                         "steady-state, cache-warm and one-step-per-replay loops and (config 2, N = 1) the compact "
                         "block of the other configurations.  Off: the run times the headline loop and nothing else")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="configs 2 / 2b: after the timed steps write what the last timed step computed (the layer's "
                         "output features, the input-feature and weight gradients) as DIR/<name>.npy, float32, at most "
                         "64 MB in all (a fixed, seeded sample of rows beyond that)")
    args = ap.parse_args(argv)
    if args.cold:
        args.scenes = max(args.scenes, 4)
    if args.dump_outputs and args.config not in ("2", "2b"):
        ap.error("--dump-outputs is implemented for configs 2 and 2b")
    return args


# ------------------------------------------------------------------ multi-rank launch
def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_command(gpus: int, argv) -> list:
    """The torch.distributed.run command `bench.py --gpus N` re-executes itself under."""
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
            "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__), *argv]


def maybe_spawn(args, argv) -> None:
    """--gpus N without a launcher's environment: become the launcher (one rank per GPU)."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    cmd = launch_command(args.gpus, argv)
    if os.environ.get("BENCH_DRY_LAUNCH") == "1":          # tests: show the command, do not run it
        print(json.dumps({"launch": cmd}))
        raise SystemExit(0)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC (RCCL across processes)
    import subprocess                                      # a child process, not exec: the launcher stays the parent
    raise SystemExit(subprocess.call(cmd, env=env))


# ------------------------------------------------------------------ helpers
def algorithmic_bytes(n_in, n_out, C, K, kv, s, out_s=None):
    """Compulsory bytes per call: features/outputs touched once, whole
    rulebook read once, weights once."""
    out_s = s if out_s is None else out_s
    fwd = s * n_in * C + out_s * n_out * K + 4 * kv * n_out + s * kv * C * K
    dgrad = s * n_out * K + s * n_in * C + 4 * kv * n_in + s * kv * C * K
    wgrad = s * n_in * C + s * n_out * K + 4 * kv * n_out + 4 * kv * C * K
    return {"fwd": fwd, "dgrad": dgrad, "wgrad": wgrad, "bwd": dgrad + wgrad}


def event_time_ms(fn, iters=80, warm=10, span=0):
    """Average device time of fn(i) between HIP events recorded on the current (launch) stream.
    span > 0: the calls fn(0) .. fn(span - 1) are captured into ONE hipGraph and the replays are
    timed, so that host enqueue time (ctypes + torch.empty, which exceeds the kernel time of a
    100 k-voxel scene) cannot leak into a kernel group's figure; falls back to eager launches."""
    g = None
    if span > 0:
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for i in range(span):
                    fn(i)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
                for i in range(span):
                    fn(i)
        except Exception as e:
            print(f"[bench] group capture failed ({type(e).__name__}: {e}); timing eager launches", file=sys.stderr)
            g = None
            torch.cuda.synchronize()
    if g is not None:
        reps = max(3, iters // span)
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / (reps * span)
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def pmc_traffic(key, group):
    """HBM bytes per launch of a kernel group from the committed rocprofv3 PMC passes
    (FETCH_SIZE x 2 [gfx950 wide-read correction, MI355X_MICROARCH.md] + WRITE_SIZE, separate
    --pmc runs of THIS command; tools/pmc_traffic.py wrote profiles/traffic.json)."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            v = json.load(f)[key][group]["hbm_bytes_per_launch"]
        return int(v) if v else None
    except (OSError, KeyError, ValueError, TypeError):
        return None


# every (workload key, kernel group) bench.py asks profiles/traffic.json for (tests/test_host.py checks that the
# committed file answers all of them: BENCH_r04 carried `traffic: null` because the file had been overwritten by a
# per-key fragment)
TRAFFIC_KEYS = (("uniform-f16-c64-n100000", "fwd"), ("uniform-f16-c64-n100000", "bwd"),
                ("fixture-f16-c64-n100000", "fwd"), ("fixture-f16-c64-n100000", "bwd"),
                ("uniform-i8-c128-n200000", "fwd"))


def roofline_obj(group, ab, ms, kernel, traffic=None, extra=None):
    achieved = ab / (ms * 1e-3) / 1e9
    r = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
         "traffic_over_algorithmic": round(traffic / ab, 3) if traffic else None,
         "traffic_source": "profiles/traffic.json (builder-run rocprofv3 --pmc passes)" if traffic else None,
         "group": group, "kernel": kernel, "algorithmic_bytes": int(ab), "ms": round(ms, 5)}
    if extra:
        r.update(extra)
    return r


DUMP_BYTES = 60_000_000        # data bytes of --dump-outputs (64 MB in all with the .npy headers, with room to spare)


def dump_outputs(path, arrays, budget=DUMP_BYTES):
    """Writes every tensor of `arrays` (name -> tensor) as <path>/<name>.npy in float32.  When the float32 total exceeds
    `budget`, every array keeps the same fraction of its rows (dim 0), a fixed sample (numpy seed 0, ascending row order),
    so that two builds given the same arguments write the same rows.  Returns name -> {shape, rows_sampled}."""
    arrs = {k: v.detach().float().cpu().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float32)
            for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrs.values())
    os.makedirs(path, exist_ok=True)
    info = {}
    for name, a in arrs.items():
        rows = None
        if total > budget and a.ndim >= 1 and a.shape[0] > 1:
            keep = max(1, a.shape[0] * budget // total)
            rows = np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))
            a = a[rows]
        np.save(os.path.join(path, f"{name}.npy"), np.ascontiguousarray(a, dtype=np.float32))
        info[name] = {"shape": list(a.shape), "rows_sampled": None if rows is None else int(rows.shape[0])}
    return info


class Dist:
    """Rank bookkeeping; the process group comes up lazily (after graph capture)."""

    def __init__(self):
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        # BENCH_DIST_BACKEND=gloo BENCH_ONE_DEVICE=1: dry run of the N > 1 control flow on one GPU
        self.backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")
        if os.environ.get("BENCH_ONE_DEVICE", "0") == "1":
            self.local_rank = 0
        # BENCH_SOLO_DIST=1: the distributed code path (process group brought up after graph capture, gradient
        # bucket all-reduced on the side stream, barriers) with a world of ONE rank -- the only way to run the real
        # RCCL backend through that path on a one-GPU box
        self.multi = self.world > 1 or os.environ.get("BENCH_SOLO_DIST", "0") == "1"
        if self.multi and self.world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(_free_port()))
        self.up = False
        self.dev = None

    def init(self):
        if self.multi and not self.up:
            import torch.distributed as dist
            if self.backend == "nccl":
                dist.init_process_group("nccl", rank=self.rank, world_size=self.world, device_id=self.dev)
            else:
                dist.init_process_group(self.backend, rank=self.rank, world_size=self.world)
            self.up = True

    def barrier(self):
        if self.multi:
            import torch.distributed as dist
            dist.barrier()

    def reduce_max_sum(self, elapsed, n):
        if not self.multi:
            return elapsed, n, 1
        import torch.distributed as dist
        t = torch.tensor([elapsed], device=self.dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        tot = torch.tensor([float(n), 1.0], device=self.dev, dtype=torch.float64)
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        seen = int(tot[1].item())
        if seen != self.world:       # a rank that did not take part would silently inflate the per-GPU figure
            raise RuntimeError(f"bench: {seen} ranks answered the reduction, WORLD_SIZE is {self.world}")
        return float(t.item()), int(tot[0].item()), seen

    def finish(self):
        if self.up:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()


def timed_region(D: Dist, run_steps, warmup, steps):
    """W untimed steps, then exactly K steps between barrier + synchronize on both sides."""
    run_steps(warmup)
    torch.cuda.synchronize()
    D.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_steps(steps)
    torch.cuda.synchronize()
    D.barrier()
    return time.perf_counter() - t0


def fixture_coords():
    """tests/golden/lidar_scene.npz: the reference fixture's voxel coordinates (delta-encoded)."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "lidar_scene.npz"))
    shape = [int(v) for v in d["shape"]]
    lin = np.cumsum(d["delta"].astype(np.int64))
    return lin, shape


def fixture_scene(seed):
    """Scene `seed` of the fixture family: seed 0 = the fixture itself (shuffled row order, as
    tests/golden loads it); other seeds mirror / shift it in y, x so that rotated scenes are
    distinct tensors with the same neighbourhood statistics."""
    lin, shape = fixture_coords()
    z, y, x = np.unravel_index(lin, shape)
    if seed & 1:
        y = shape[1] - 1 - y
    if seed & 2:
        x = shape[2] - 1 - x
    if seed & 4:
        y, x = x.copy(), y.copy()
    lin = np.ravel_multi_index((z, y, x), shape)
    if os.environ.get("BENCH_FIXTURE_ORDER", "shuffled") == "raster":
        lin = np.sort(lin)            # A/B: rows in raster order (what the row order alone is worth)
    else:
        np.random.default_rng(seed).shuffle(lin)
    coords = np.stack(np.unravel_index(lin, shape), axis=-1).astype(np.int32)
    idx = np.concatenate([np.zeros((coords.shape[0], 1), dtype=np.int32), coords], axis=1)
    return np.ascontiguousarray(idx), shape


def make_scene(kind, voxels, seed, batch=1, shape=None):
    from spconv_amd.utils import synthetic
    if kind == "fixture":
        assert batch == 1
        return fixture_scene(seed)
    shape = shape or SHAPE
    gen = synthetic.uniform_scene if kind == "uniform" else synthetic.lidar_like_scene
    return gen(shape, voxels, batch, seed=seed * 131), shape


# ------------------------------------------------------------------ CPU baselines
def key_sorted(idx_np, shape):
    """Rows of a scene in ascending coordinate-key order (batch-major, last axis fastest)."""
    key = idx_np[:, 0].astype(np.int64)
    for d, s in enumerate(shape):
        key = key * int(s) + idx_np[:, 1 + d]
    return np.ascontiguousarray(idx_np[np.argsort(key, kind="stable")])


def cpu_baseline_layer(idx, shape, C, K, seed):
    """The oracle (port of the reference CPU path) on this host: rulebook once, then fwd+bwd.

    Two variants: faithful-pip = serial gather / scatter-add (the published
    CPU wheel has no OpenMP) + torch.mm on the thread pool; faithful-omp = rows gathered / scattered
    in parallel as a source build with -fopenmp would.  Thread settings: 16, and os.cpu_count() as
    BASELINE.md asks -- on a many-core host the small per-offset GEMMs oversubscribe badly there,
    so that setting gets one pass only when it is slow.  `value` is the FASTEST of all runs."""
    import oracle
    n = idx.shape[0]
    rng = np.random.default_rng(seed)
    f = torch.from_numpy(rng.uniform(-1, 1, (n, C)).astype(np.float32))
    w = torch.from_numpy(rng.uniform(-1, 1, (K, 3, 3, 3, C)).astype(np.float32))
    dout = torch.from_numpy(rng.uniform(-0.2, 0.2, (n, K)).astype(np.float32))
    cores = os.cpu_count() or 1
    t0 = time.perf_counter()
    _, pair, num, _ = oracle.get_indice_pairs(idx, 1, shape, [3] * 3, [1] * 3, [1] * 3, [1] * 3, subm=True)
    t_rule = time.perf_counter() - t0

    def one_pass(omp):
        t0 = time.perf_counter()
        oracle.indice_conv(f, w, pair, num, n, subm=True, omp=omp)
        oracle.indice_conv_backward(f, w, dout, pair, num, subm=True, omp=omp)
        return time.perf_counter() - t0

    results = {}
    slow_at_all_cores = False
    for variant, omp in (("faithful-pip", False), ("faithful-omp", True)):
        for threads in sorted({min(16, cores), cores}):
            if threads == cores and cores > 16 and slow_at_all_cores:
                continue                                    # already shown to oversubscribe: skip
            torch.set_num_threads(threads)
            oracle.set_omp_threads(threads)
            first = one_pass(omp)                           # warm-up, also sizes the budget
            times = []
            if first > 3.0:                                 # seconds per step: one pass is the sample
                times = [first]
                slow_at_all_cores = slow_at_all_cores or threads == cores
            else:
                budget = time.perf_counter() + 5.0
                while len(times) < 10 and (time.perf_counter() < budget or not times):
                    times.append(one_pass(omp))
            results[f"{variant}@{threads}"] = statistics.median(times)
    # The same step on the reference's OWN code where it compiles here: rulebook = SparseConvIndicesCPU (indices.py:1639-1708),
    # row gather / scatter-add = GatherCPU (gather.py:30-86), both rendered from /root/reference by oracle/refbuild and
    # compiled into oracle/_ref; torch.mm in between, as the reference's cppcore.py:232-348 callbacks do.  Serial gather /
    # scatter (the published CPU wheel has no OpenMP, README.md:133) + MKL threads.
    reference = None
    try:
        from oracle import ref as oref
        if oref.available():
            t0 = time.perf_counter()
            _, rpair, rnum, _ = oref.get_indice_pairs(idx, 1, shape, [3] * 3, [1] * 3, [1] * 3, [1] * 3, subm=True)
            t_rrule = time.perf_counter() - t0
            same = bool(np.array_equal(rpair, pair) and np.array_equal(rnum, num))
            threads = min(16, cores)
            torch.set_num_threads(threads)
            oracle.use_reference_gather(True)
            try:
                def ref_pass():
                    t0 = time.perf_counter()
                    oracle.indice_conv(f, w, rpair, rnum, n, subm=True, omp=False)
                    oracle.indice_conv_backward(f, w, dout, rpair, rnum, subm=True, omp=False)
                    return time.perf_counter() - t0
                first = ref_pass()
                rtimes = [first] if first > 3.0 else []
                budget = time.perf_counter() + 5.0
                while not rtimes or (first <= 3.0 and len(rtimes) < 10 and time.perf_counter() < budget):
                    rtimes.append(ref_pass())
            finally:
                oracle.use_reference_gather(False)
            rmed = statistics.median(rtimes)
            reference = {"value": n / rmed, "unit": "voxels/s", "cores": threads, "kind": "reference-rendered",
                         "ms_per_step": rmed * 1e3, "rulebook_ms": t_rrule * 1e3,
                         "rulebook_equals_port": same,
                         "sample": f"{len(rtimes)} fwd+bwd passes of the same {n}-voxel scene: rulebook by the reference's "
                                   f"SparseConvIndicesCPU ({t_rrule * 1e3:.1f} ms, single thread), rows moved by its GatherCPU "
                                   f"(serial), torch.mm on {threads} threads; compiled from /root/reference by "
                                   f"oracle/refbuild (oracle/_ref/libspconv_ref.so)"}
    except Exception as e:                                   # the checker library is optional on a box without it
        reference = {"error": f"{type(e).__name__}: {e}"[:200], "kind": "reference-rendered"}
    best = min(results, key=results.get)
    med = results[best]
    others = ", ".join(f"{k}: {v * 1e3:.0f} ms/step" for k, v in results.items())
    return {"value": n / med, "unit": "voxels/s", "cores": int(best.split("@")[1]), "kind": "port",
            "reference_rendered": reference,
            "sample": f"fwd+bwd passes (1 warm-up, <= 10 timed, ~5 s budget per setting) of one "
                      f"{n}-voxel scene of this workload, fp32, per-offset gather -> torch.mm -> scatter-add "
                      f"(BASELINE.md) on a {cores}-thread host; fastest = {best}; all settings: {others}; "
                      f"rulebook built once: {t_rule * 1e3:.1f} ms (single thread, std::unordered_map)",
            "variant": best.split("@")[0], "ms_per_step": med * 1e3, "rulebook_ms": t_rule * 1e3}


def cpu_baseline_int8(idx, shape, C, K):
    """numpy restatement of the reference's int8 forward + quantised epilogue
    (test/test_all_algo.py:222-288) on the same scene: per-offset gather -> matmul -> scatter-add,
    BLAS threads as numpy finds them."""
    import oracle
    n = idx.shape[0]
    rng = np.random.default_rng(5)
    f = rng.integers(-127, 128, (n, C), dtype=np.int8)
    w = rng.integers(-127, 128, (K, 3, 3, 3, C), dtype=np.int8)
    scale = (rng.uniform(0.5, 1.5, K) * 1e-2).astype(np.float32)
    bias = rng.uniform(-1, 1, K).astype(np.float32)
    t0 = time.perf_counter()
    _, pair, num, _ = oracle.get_indice_pairs(idx, 1, shape, [3] * 3, [1] * 3, [1] * 3, [1] * 3, subm=True)
    t_rule = time.perf_counter() - t0
    times = []
    budget = time.perf_counter() + 15.0
    while len(times) < 5 and (time.perf_counter() < budget or not times):
        t0 = time.perf_counter()
        oracle.int8_conv_ref(f, w, pair, num, n, True, scale, bias, relu=True)
        times.append(time.perf_counter() - t0)
    dt = statistics.median(times)
    return {"value": n / dt, "unit": "voxels/s", "cores": os.cpu_count() or 1, "kind": "port",
            "sample": f"{len(times)} int8 forward passes (per-offset gather -> matmul -> scatter-add + quantised "
                      f"epilogue, numpy) over the same {n}-voxel scene, median {dt * 1e3:.0f} ms; rulebook "
                      f"{t_rule * 1e3:.0f} ms (single thread)",
            "ms_per_step": dt * 1e3}


def cpu_baseline_net(layers, seed=0, budget_s=25.0):
    """Oracle pass over the sparse conv layers of a network step (rulebook + forward + backward
    per layer on the layer's recorded coordinates, fp32, random features), conv layers only."""
    import oracle
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    oracle.set_omp_threads(min(16, os.cpu_count() or 1))
    rng = np.random.default_rng(seed)
    t_total, done, vox = 0.0, 0, 0
    for L in layers:
        idx = L["idx"]
        t0 = time.perf_counter()
        out_inds, pair, num, _ = oracle.get_indice_pairs(idx, L["bs"], L["shape"], L["ksize"], L["stride"],
                                                         L["padding"], L["dilation"], None, L["subm"], False)
        n_out = out_inds.shape[0]
        f = torch.from_numpy(rng.uniform(-1, 1, (idx.shape[0], L["C"])).astype(np.float32))
        w = torch.from_numpy(rng.uniform(-1, 1, (L["K"], *L["ksize"], L["C"])).astype(np.float32))
        d = torch.from_numpy(rng.uniform(-1, 1, (n_out, L["K"])).astype(np.float32))
        oracle.indice_conv(f, w, pair, num, n_out, subm=L["subm"], omp=True)
        oracle.indice_conv_backward(f, w, d, pair, num, subm=L["subm"], omp=True)
        t_total += time.perf_counter() - t0
        done += 1
        if t_total > budget_s:
            break
    return t_total, done


# ------------------------------------------------------------------ config 2 / 2b
def run_layer(args, D: Dist):
    import spconv_amd.pytorch as spconv
    from spconv_amd.dist import GradBucket
    from spconv_amd.pytorch import ops
    dev, world, rank = D.dev, D.world, D.rank
    dtype = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[args.dtype]
    kind = args.scene or ("fixture" if args.config == "2b" else "uniform")
    voxels = args.voxels or 100_000
    C = K = args.channels or 64
    S = max(1, args.scenes)
    torch.manual_seed(0)
    import spconv_amd.pytorch.conv as conv_mod
    if args.sort != "auto":              # A/B runs only: what SPCONV_DO_SORT=1 / 0 would select
        conv_mod.MODULE_DO_SORT = {"on": True, "off": False}[args.sort]
    net = spconv.SubMConv3d(C, K, 3, bias=False, indice_key="bench").to(dev, dtype)
    net.train()

    class Scene:
        pass

    scenes, rule_ms = [], []
    for si in range(S):
        sc = Scene()
        sc.idx_np, sc.shape = make_scene(kind, voxels, seed=rank * S + si)
        if getattr(args, "key_order", False):      # rows in ascending coordinate key (utils.sort_voxels_by_coordinate)
            sc.idx_np = key_sorted(sc.idx_np, sc.shape)
        sc.n = sc.idx_np.shape[0]
        sc.indices = torch.from_numpy(sc.idx_np).to(dev)
        g = torch.Generator(device="cpu").manual_seed(1234 + rank * S + si)
        sc.feats = (torch.rand((sc.n, C), generator=g) * 2 - 1).to(dev, dtype).requires_grad_(True)
        sc.dout = ((torch.rand((sc.n, K), generator=g) * 2 - 1) * 0.2).to(dev, dtype)

        # the rulebook is the one the MODULE builds: net(x) with a default environment (density-aware rows layout
        # made on the device inside the build), cached under the layer's indice_key and reused by every later step
        # exactly as a second SubM layer of a backbone stage reuses it (docs/USAGE.md:104-105)
        with torch.no_grad():
            y0 = net(spconv.SparseConvTensor(sc.feats.detach(), sc.indices, sc.shape, 1))
        sc.rb = y0.indice_dict["bench"].rulebook
        sc.x = spconv.SparseConvTensor(sc.feats, sc.indices, sc.shape, 1, indice_dict=y0.indice_dict)
        del y0

        def build(sc=sc):            # what the module's first call runs (conv.py: ops.build_rulebook)
            return ops.build_rulebook(sc.indices, 1, sc.shape, [3] * 3, [1] * 3, [1] * 3, [1] * 3, [0] * 3,
                                      True, do_sort=conv_mod.MODULE_DO_SORT)[0]
        torch.cuda.synchronize()
        if si == 0 and args.full:        # rulebook build: timed separately (wall, incl. enqueue)
            for _ in range(5):
                t0 = time.perf_counter()
                build()
                torch.cuda.synchronize()
                rule_ms.append((time.perf_counter() - t0) * 1e3)
            t_rule_dev = event_time_ms(lambda i: build(), iters=10, warm=2)
        ops._plan_of(sc.rb)
        num = sc.rb.num_per_loc.cpu().numpy()
        sc.P = int(sc.n + 2 * num[:13].sum())                      # pairs incl. centre
        scenes.append(sc)
    n = scenes[0].n
    bucket = GradBucket(net.parameters()) if D.multi else None   # fp16 gradient, reduced in place

    def compute(sc, keep=None):
        """One step; `keep` (a dict) receives what the step hands its caller: output features, dX, dW."""
        net.weight.grad = None
        sc.feats.grad = None
        y = net(sc.x)
        y.features.backward(sc.dout)
        if keep is not None:
            keep.update(out_features=y.features.detach(), grad_features=sc.feats.grad, grad_weight=net.weight.grad)

    # what the last step of each captured graph hands its caller (tensors of the graph's pool, rewritten by every
    # replay), and what the last step run so far handed it: --dump-outputs writes the latter after the timed steps
    outs_of, last_out = {}, [None]
    launch = "eager"
    fwd_dispatched = {}   # forward launches per kernel family inside the timed graph's capture
    graphs = None         # one step per replay, one graph per scene
    graph_grads = []      # the gradient tensor each per-scene graph writes
    graph_u = None        # U steps per replay over consecutive scenes (N = 1 only)
    graph_w = None        # U steps per replay, all on scene 0 (the Infinity-Cache-resident loop)
    U = max(1, args.graph_steps)
    graph_b = None        # N > 1: a second U-step graph with its own gradient buffers (the two alternate)
    dws_a, dws_b = [], [] # the dW tensor each captured step of graph_u / graph_b writes
    rem_graphs = {}       # r -> (graph of r < U steps, its dW tensors): the tail of a run whose length is no multiple of U
    if not args.no_graph:
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for sc in scenes:
                    for _ in range(2):
                        compute(sc)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graphs = []
            for sc in scenes:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
                    compute(sc, outs_of.setdefault(id(g), {}))
                graphs.append(g)
                graph_grads.append(net.weight.grad)   # each graph writes dW into its own pool buffer
            if U > 1:
                graph_u = torch.cuda.CUDAGraph()
                lc0 = {k: _lib_count(k) for k in ("igemm_ws", "igemm_v4")}
                with torch.cuda.graph(graph_u, capture_error_mode=CAPTURE_MODE):
                    for u in range(U):
                        compute(scenes[u % S], outs_of.setdefault(id(graph_u), {}) if u == U - 1 else None)
                        dws_a.append(net.weight.grad)
                # which forward kernel the TIMED graph holds (the library's own record of what it dispatched while
                # the graph was captured -- not the class state seen afterwards: round-5 ADVICE)
                fwd_dispatched.update({k: _lib_count(k) - v for k, v in lc0.items()})
                if D.multi:
                    graph_b = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph_b, capture_error_mode=CAPTURE_MODE):
                        for u in range(U):
                            compute(scenes[u % S], outs_of.setdefault(id(graph_b), {}) if u == U - 1 else None)
                            dws_b.append(net.weight.grad)
                else:
                    graph_w = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph_w, capture_error_mode=CAPTURE_MODE):
                        for u in range(U):
                            compute(scenes[0])
                # the steps of a run that do not fill a U-step replay (K mod U, W mod U) get a graph of their own
                # length: a 20-step run is 2 x 8 + 1 x 4 steps = three launches, not 2 + four single-step replays
                for r in sorted({args.prewarm % U, args.warmup % U, args.steps % U} - {0}):
                    g = torch.cuda.CUDAGraph()
                    dws = []
                    with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
                        for u in range(r):
                            compute(scenes[u % S], outs_of.setdefault(id(g), {}) if u == r - 1 else None)
                            dws.append(net.weight.grad)
                    rem_graphs[r] = (g, dws)
            launch = "hipgraph"
        except Exception as e:  # capture unsupported -> eager launches, same work
            print(f"[bench] graph capture failed ({type(e).__name__}: {e}); using eager launches",
                  file=sys.stderr)
            graphs = graph_u = graph_w = graph_b = None
            graph_grads, rem_graphs = [], {}
            outs_of.clear()
            torch.cuda.synchronize()
    if graph_u is None:
        U = 1
    # the process group comes up AFTER the capture, so that no RCCL helper thread can touch the
    # device while the stream is capturing
    D.init()
    counter = [0]

    def step(warm=False):
        i = 0 if warm else counter[0] % S
        counter[0] += 1
        if graphs is not None:
            graphs[i].replay()
            net.weight.grad = graph_grads[i]                       # the dW this replay produced
            last_out[0] = outs_of[id(graphs[i])]
        else:
            last_out[0] = {}
            compute(scenes[i], last_out[0])
        if bucket is not None:
            bucket.all_reduce(average=True)                        # one RCCL call per step

    # N > 1: the gradient exchange leaves the critical path.  The U dW tensors of a replay are packed into one
    # flat bucket and all-reduced (average) on a SIDE stream while the next replay -- the other graph, with its
    # own gradient buffers -- runs; a graph is replayed again only after its bucket's all-reduce has finished.
    # One RCCL call of U x 221 KB per U steps instead of a blocking small-message call behind every step.
    overlap = None
    if D.multi and graph_b is not None:
        import torch.distributed as dist
        side_ar = torch.cuda.Stream()
        numel = net.weight.numel()

        class _Half:
            pass
        def _half(g, dws):
            h = _Half()
            h.graph, h.dws = g, dws
            h.flat = torch.zeros((len(dws), numel), dtype=dws[0].dtype, device=dev)
            h.done, h.reduced = torch.cuda.Event(), torch.cuda.Event()
            h.pending = False
            return h
        halves = [_half(graph_u, dws_a), _half(graph_b, dws_b)]
        rem_halves = {r: _half(g, dws) for r, (g, dws) in rem_graphs.items()}
        overlap = {"halves": halves, "next": 0, "rem": rem_halves}

        def replay_overlapped(h=None):
            if h is None:
                h = overlap["halves"][overlap["next"]]
                overlap["next"] ^= 1
            main = torch.cuda.current_stream()
            if h.pending:
                main.wait_event(h.reduced)           # its previous bucket has been reduced: buffers are free
            h.graph.replay()
            last_out[0] = outs_of[id(h.graph)]
            h.done.record(main)
            with torch.cuda.stream(side_ar):
                side_ar.wait_event(h.done)
                for row, d in zip(h.flat.unbind(0), h.dws):      # small device-to-device copies into the bucket
                    row.copy_(d.reshape(-1))
                if D.backend == "nccl":
                    dist.all_reduce(h.flat, op=dist.ReduceOp.AVG)
                else:
                    dist.all_reduce(h.flat, op=dist.ReduceOp.SUM)
                    h.flat.div_(world)
                h.reduced.record(side_ar)
            h.pending = True

        def drain_overlapped():
            for h in overlap["halves"] + list(overlap["rem"].values()):
                if h.pending:
                    torch.cuda.current_stream().wait_event(h.reduced)
                    h.pending = False

    def run_steps(k, warm=False):
        """Exactly k steps: whole U-step replays, then the tail (its own graph when one was captured for
        that length, single steps otherwise)."""
        gu = graph_w if warm else graph_u
        if overlap is not None and not warm:
            for _ in range(k // U):
                replay_overlapped()
            k = k % U
            if k in overlap["rem"]:
                replay_overlapped(overlap["rem"][k])
                k = 0
            drain_overlapped()
        elif gu is not None:
            for _ in range(k // U):
                gu.replay()
            if k >= U and not warm:
                last_out[0] = outs_of[id(gu)]
            k = k % U
            if not warm and k in rem_graphs:
                rem_graphs[k][0].replay()
                last_out[0] = outs_of[id(rem_graphs[k][0])]
                k = 0
        for _ in range(k):
            step(warm)

    run_steps(args.prewarm)              # untimed, stated in config.prewarm_steps; the contract's W + K follow
    elapsed = timed_region(D, run_steps, args.warmup, args.steps)
    dumped = None
    if args.dump_outputs and rank == 0:  # before anything below replays the graphs again
        dumped = dump_outputs(args.dump_outputs, last_out[0])
    # The timed region above is what the contract asks for; its wall clock holds a FIXED cost of ~30-40 us (first
    # graph launch until the first kernel runs + the wake-up of the final synchronize: fitted over K = 20 / 40 / 80 /
    # 160, profiles/r04_experiments.md), i.e. 7 % of a 20-step region and 0.1 % of a 2000-step one.  The same loop over a
    # few hundred steps is reported next to it (not `value`).
    # Round 4 quoted `value` from ONE graph of exactly K steps behind 400 untimed pre-warm steps (3.94 G voxels/s in the
    # driver's line).  That shaped the measurement around a 20-step run and put a protocol kink between N = 1 and N = 2
    # (ADVICE / VERDICT r4), so `value` is back on the plain schedule; the same figure is kept here for comparison.
    round4 = None
    if args.full and not D.multi and graph_u is not None and 1 <= args.steps <= 40 and args.steps != U:
        try:
            gk = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gk, capture_error_mode=CAPTURE_MODE):
                for u in range(args.steps):
                    compute(scenes[u % S])
            run_steps(400)
            for _ in range(max(1, args.warmup // args.steps)):
                gk.replay()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            gk.replay()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t1
            round4 = {"steps_per_replay": args.steps, "prewarm_steps": 400, "ms_per_step": round(dt / args.steps * 1e3, 5),
                      "value": round(sum(sc.n for sc in scenes) / S * args.steps / dt, 1),
                      "note": "round 4's schedule (one K-step graph behind 400 untimed steps), NOT `value`"}
            del gk
        except Exception as e:                                        # a side figure must not cost the headline
            round4 = {"error": f"{type(e).__name__}: {e}"[:200]}
    steady = None
    if args.full and not D.multi and args.steps < 400:
        k_steady = U * max(1, 400 // U)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run_steps(k_steady)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t1
        steady = {"steps": k_steady, "ms_per_step": round(dt / k_steady * 1e3, 5),
                  "value": round(sum(sc.n for sc in scenes) / S * k_steady / dt, 1),
                  "note": "same loop, same graphs, more steps: the fixed cost of a timed region amortised"}
    warm_ms = None
    if args.full and not D.multi and S > 1:   # the same K steps on ONE scene (Infinity-Cache-resident)
        run_steps(min(args.warmup, 50), warm=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run_steps(args.steps, warm=True)
        torch.cuda.synchronize()
        warm_ms = (time.perf_counter() - t1) / args.steps * 1e3
    single_replay_ms = None
    if args.full and graph_u is not None and not D.multi:   # the rotating K steps, one step per replay, for reference
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        single_replay_ms = (time.perf_counter() - t1) / args.steps * 1e3
    # BENCH_CHECK_EXCHANGE=1 (tests): the overlapped exchange, checked numerically -- after one more replay of a graph,
    # row u of its reduced bucket must equal the mean over the ranks of step u's dW (every rank has its own scenes)
    exchange_check = None
    if overlap is not None and os.environ.get("BENCH_CHECK_EXCHANGE") == "1":
        import torch.distributed as dist
        worst = 0.0
        for h in overlap["halves"] + list(overlap["rem"].values()):
            replay_overlapped(h)
            drain_overlapped()
            torch.cuda.synchronize()
            for u, dw in enumerate(h.dws):
                mine = dw.detach().float().reshape(-1).contiguous()
                everyone = [torch.empty_like(mine) for _ in range(world)]
                dist.all_gather(everyone, mine)
                want = torch.stack(everyone).mean(0)
                scale = float(want.abs().max()) or 1.0
                worst = max(worst, float((h.flat[u].float() - want).abs().max()) / scale)
        distinct = float((torch.stack(everyone)[0] - torch.stack(everyone)[-1]).abs().max()) > 0
        exchange_check = {"max_rel_err": worst, "ranks_have_distinct_gradients": bool(distinct),
                          "buckets_checked": len(overlap["halves"]) + len(overlap["rem"])}
    n_mean = sum(sc.n for sc in scenes) / S
    elapsed, n_total, ranks_seen = D.reduce_max_sum(elapsed, n_mean)
    ms_per_step = elapsed / args.steps * 1e3
    value = n_total * args.steps / elapsed
    if rank != 0:
        return None

    s = scenes[0].feats.element_size()
    P = sum(sc.P for sc in scenes) / S
    dt = args.dtype
    layout_info = None
    if scenes[0].rb.layout is not None:
        head = scenes[0].rb.layout[:4].cpu().tolist()
        layout_info = {"class": "regrouped" if head[0] else "identity", "rows_with_a_neighbour": head[1]}
    cfg_name = "configs[1]" if args.config == "2" and kind == "uniform" else f"config {args.config}"
    result = {
        "metric": METRIC, "value": value, "unit": "voxels/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": f"SubMConv3d 3x3x3 C={C}->{K} {dt}, {int(n_mean)} {kind} voxels/scene in "
                               f"{scenes[0].shape[2]}x{scenes[0].shape[1]}x{scenes[0].shape[0]} (BASELINE {cfg_name}), "
                               f"{S} distinct scenes per GPU visited round-robin, rulebook reused via indice_key",
                   "voxels_per_gpu": int(n_mean), "pairs_per_voxel": round(P / n_mean, 4), "launch": launch,
                   "steps_per_replay": U if launch == "hipgraph" else None, "scenes_rotated": S,
                   "rulebook_source": "net(x): the module's own build, default environment" if args.sort == "auto"
                                      else f"net(x) with SPCONV_DO_SORT={'1' if args.sort == 'on' else '0'}",
                   "rows_layout": layout_info, "mask_sort": scenes[0].rb.argsort_fwd is not None,
                   "forward_launches_in_timed_graph": fwd_dispatched or None,
                   "prewarm_steps": args.prewarm, "gradient_exchange_check": exchange_check,
                   "parallelism": f"dp{world}",
                   "ranks_seen": ranks_seen,
                   "dist_backend": D.backend if D.multi else None,
                   "gradient_exchange": None if not D.multi else (
                       f"one flat-bucket all-reduce (average) of the {U} dW of a replay ({U} x {net.weight.numel() * s} B) "
                       f"on a side stream, overlapped with the next replay (two graphs with their own gradient "
                       f"buffers alternate)" if overlap is not None else "blocking all-reduce of dW after every step")},
    }
    if dumped is not None:
        result["dumped_outputs"] = {"dir": os.path.abspath(args.dump_outputs), "arrays": dumped,
                                    "step": "the last timed step (rank 0): output features, dX, dW"}
    if not args.full:
        return result

    # ---- per-kernel-group device time (HIP events on the launch stream), cold and warm -------
    w = net.weight.detach()
    plan = [ops._plan_of(sc.rb) for sc in scenes]

    def groups_for(pick):
        def fwd(i):
            sc = scenes[pick(i)]
            pair, mask, order, to = ops.tables_of(sc.rb, "fwd", K)
            ops.igemm_fwd(sc.feats.detach(), w, pair, mask, order, sc.n, 13, tile_order=to)

        def bwd(i):
            sc = scenes[pick(i)]
            pair, mask, order, to = ops.tables_of(sc.rb, "fwd", C)
            ops.igemm_bwd(sc.feats.detach(), sc.dout, w, pair, mask, order, sc.rb.pair_native,
                          sc.rb.num_per_loc, True, plan[pick(i)], tile_order=to)

        def dgrad(i):
            sc = scenes[pick(i)]
            pair, mask, order, to = ops.tables_of(sc.rb, "fwd", C)
            ops.igemm_dgrad(sc.dout, w, pair, mask, order, sc.n, True, tile_order=to)

        def wgrad(i):
            sc = scenes[pick(i)]
            ops.igemm_wgrad(sc.feats.detach(), sc.dout, w.shape, sc.rb.pair_native, sc.rb.num_per_loc, True,
                            plan[pick(i)])
        sp = 0 if args.no_graph else max(S, 8)
        return {"fwd": event_time_ms(fwd, span=sp), "bwd": event_time_ms(bwd, span=sp),
                "dgrad": event_time_ms(dgrad, span=sp), "wgrad": event_time_ms(wgrad, span=sp)}
    t_cold = groups_for(lambda i: i % S)
    t_warm = groups_for(lambda i: 0) if S > 1 else t_cold
    # eager launches of the same step.  Fresh leaf tensors: the benchmark's own leaves were first used on the
    # capture side stream, and autograd ties a leaf's AccumulateGrad node to that stream -- every eager backward
    # on the main stream would then pay cross-stream event traffic (166 us per step instead of ~75) that a
    # training loop, which stays on one stream, never sees.
    import copy
    net_e = copy.deepcopy(net)
    eager = []
    for sc in scenes:
        fe = sc.feats.detach().clone().requires_grad_(True)
        xe = spconv.SparseConvTensor(fe, sc.indices, sc.shape, 1)
        xe.indice_dict["bench"] = sc.x.indice_dict["bench"]
        eager.append((fe, xe, sc.dout))

    def compute_eager(i):
        fe, xe, do = eager[i % S]
        net_e.weight.grad = None
        fe.grad = None
        net_e(xe).features.backward(do)
    # host-paced (three launches per step enqueued from Python).  Round 5 pinned the bimodal figure of rounds 3-4 (76 vs
    # 150-200 us on the same tree) to the autograd engine's DEVICE THREAD: backward runs on a worker thread the calling
    # thread wakes every step, and when the scheduler parks that thread on a far / sleeping core the hand-over doubles the
    # step.  With the engine single-threaded (torch.autograd.set_multithreading_enabled(False): backward on the calling
    # thread) six of six processes ran 76-77 us; pinning the process to two cores does the same
    # (profiles/r05_experiments.md section 8).  Both figures: the recipe's, and the default engine's (median of three).
    # Round 6: importing spconv_amd.pytorch puts the engine on the calling thread in a process that drives ONE GPU
    # (spconv_amd/pytorch/__init__.py: AUTOGRAD_ENGINE) -- the "default engine" runs below are what a drop-in user gets
    # after the import; torch's own multi-threaded engine is measured explicitly beside it.
    with torch.autograd.set_multithreading_enabled(False):
        eager_runs_st = [event_time_ms(compute_eager, iters=200, warm=30) for _ in range(3)]
    eager_runs = [event_time_ms(compute_eager, iters=200, warm=30) for _ in range(3)]
    with torch.autograd.set_multithreading_enabled(True):
        eager_runs_mt = [event_time_ms(compute_eager, iters=200, warm=30) for _ in range(2)]
    t_eager = sorted(eager_runs_st)[1]
    del net_e, eager
    t_sort_dev = None
    if scenes[0].rb.argsort_fwd is not None:      # mask sort + tile-order table copies: once per rulebook
        t_sort_dev = round(event_time_ms(lambda i: ops.sort_rulebook(scenes[0].rb), iters=10, warm=2), 4)
    t_layout_dev = None
    if scenes[0].rb.layout is not None:           # the rows layout alone (count -> scan -> scatter), part of every build
        t_layout_dev = round(event_time_ms(lambda i: ops.rows_layout(scenes[0].rb), iters=10, warm=2), 4)
    ab = algorithmic_bytes(n_mean, n_mean, C, K, 27, s)
    # stricter count for the fused backward launch: dout is read once for both gradients
    # (dout + feat + din + pair table + Native lists of P pairs + W + dW)
    strict = {"fwd": ab["fwd"], "bwd": s * n_mean * K + 2 * s * n_mean * C + 4 * 27 * n_mean + 8 * P
              + 2 * s * 27 * C * K}
    ops.poll_class(scenes[0].rb)
    dense_fwd = bool(getattr(scenes[0].rb.layout, "_spx_dense", False)) and C == 64 and K == 64
    if fwd_dispatched:
        dense_fwd = fwd_dispatched.get("igemm_ws", 0) > 0 and fwd_dispatched.get("igemm_v4", 0) == 0
    kname = {"fwd": (f"igemm_ws_kernel<16,9,2,{dt},fwd> (weight-stationary, dense class)" if dense_fwd
                     else f"igemm_v4_kernel<{K},2,{dt},fwd>"),
             "bwd": f"igemm_bwd_kernel<{C},2,{dt}> + wgrad_reduce2_kernel"}
    tkey = f"{kind}-{dt}-c{C}-n{voxels}"

    def roof(t, label):
        dom = max(("fwd", "bwd"), key=lambda k: t[k])
        return roofline_obj(dom, ab[dom], t[dom], kname[dom], pmc_traffic(tkey, dom),
                            {"memory_level": label, "shared_input_bytes": int(strict[dom]),
                             "shared_input_frac": round(strict[dom] / (t[dom] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)})
    cold_label = (f"HBM: loop rotates over {S} scenes, ~{S * (4 * s * n_mean * C + 12 * 27 * n_mean) / 1e6:.0f} MB "
                  f"working set > 256 MiB Infinity Cache") if S >= 4 else \
        f"{S} scene(s) replayed: working set fits the 256 MiB Infinity Cache (NOT an HBM measurement)"
    r_cold = roof(t_cold, cold_label)
    r_warm = roof(t_warm, "Infinity Cache: one scene replayed (~88 MB working set stays in the 256 MiB L3)")

    def ktable(t):
        return {k: {"ms": round(v, 5), "algorithmic_MB": round(ab[k] / 1e6, 3),
                    "GBps": round(ab[k] / (v * 1e-3) / 1e9, 1)} for k, v in t.items()}
    total_bytes = ab["fwd"] + ab["bwd"]
    result.update({
        "roofline": r_cold, "roofline_cold": r_cold, "roofline_warm": r_warm,
        "kernels": ktable(t_cold), "kernels_warm": ktable(t_warm),
        "kernels_note": "each group is timed alone (its own hipGraph, rotating over the scenes); in a step the "
                        "backward of scene i finds the rows and tables its forward has just read in the caches, "
                        "so ms_per_step can be below fwd + bwd",
        "warm": None if warm_ms is None else {"ms_per_step": round(warm_ms, 5),
                                              "value": round(n / (warm_ms * 1e-3), 1),
                                              "note": "one scene replayed: Infinity-Cache-resident working set"},
        "steady_state": steady,
        "round4_protocol": round4,
        "step_GBps_algorithmic": round(total_bytes / (ms_per_step * 1e-3) / 1e9, 1),
        "eager_device_ms_per_step": round(t_eager, 5),
        "eager_device_ms_per_step_note": "autograd engine single-threaded (torch.autograd.set_multithreading_enabled(False)): "
                                         "median of three windows; default engine beside it",
        "eager_device_ms_per_step_runs": [round(v, 5) for v in eager_runs_st],
        "eager_device_ms_per_step_default_engine_runs": [round(v, 5) for v in eager_runs],
        "eager_autograd_engine_after_import": spconv.AUTOGRAD_ENGINE,
        "eager_device_ms_per_step_torch_multithreaded_engine_runs": [round(v, 5) for v in eager_runs_mt],
        "ms_per_step_one_step_per_replay": None if single_replay_ms is None else round(single_replay_ms, 5),
        "rulebook_ms": round(statistics.median(rule_ms), 4),
        "rulebook_device_ms": round(t_rule_dev, 4),
        "rows_layout_device_ms": t_layout_dev,
        "mask_sort_device_ms": t_sort_dev,
    })
    if world == 1 and args.full and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline_layer(scenes[0].idx_np, scenes[0].shape, C, K, seed=1)
    return result


# ------------------------------------------------------------------ config 5 (int8 inference)
def run_int8(args, D: Dist):
    from spconv_amd.pytorch import ops
    dev = D.dev
    voxels = args.voxels or 200_000
    C = K = args.channels or 128
    S = max(1, args.scenes)
    rng = np.random.default_rng(5)
    w = torch.from_numpy(rng.integers(-127, 128, (K, 3, 3, 3, C), dtype=np.int8)).to(dev)
    scale = torch.from_numpy((rng.uniform(0.5, 1.5, K) * 1e-2).astype(np.float32)).to(dev)
    bias = torch.from_numpy(rng.uniform(-1, 1, K).astype(np.float32)).to(dev)
    scenes = []
    for si in range(S):
        idx_np, shape = make_scene(args.scene or "uniform", voxels, seed=D.rank * S + si)
        ind = torch.from_numpy(idx_np).to(dev)
        rb = ops.build_rulebook(ind, 1, shape, [3] * 3, [1] * 3, [1] * 3, [1] * 3, [0] * 3, True,
                                need_native=False, do_sort={"auto": "layout", "on": True, "off": False}[args.sort])[0]
        ops.sparse_neighbourhoods(rb)     # host view of the class (one read per rulebook, outside the timed loop):
                                          # the int8 launch picks its tile height by it
        f = torch.from_numpy(rng.integers(-127, 128, (idx_np.shape[0], C), dtype=np.int8)).to(dev)
        scenes.append((idx_np, shape, rb, f))
    n = scenes[0][0].shape[0]

    def fwd(i):
        _, _, rb, f = scenes[i % S]
        pair, mask, order, to = ops.tables_of(rb, "fwd", K)
        return ops.igemm_fwd_int8(f, w, pair, mask, order, n, 13, scale, bias, None, 0.0,
                                  torch.int8, ops.Activation.ReLU, 0.0, tile_order=to,
                                  sparse_hint=rb.sparse_class is True, hint_rows=getattr(rb, "heavy_rows", 0))
    graphs = None
    if not args.no_graph:
        try:
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for i in range(S):
                    fwd(i)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
                for i in range(S):
                    fwd(i)
            graphs = g
        except Exception as e:
            print(f"[bench] graph capture failed ({e}); eager", file=sys.stderr)
            graphs = None
    D.init()
    cnt = [0]

    def run_steps(k):
        if graphs is not None:
            for _ in range(k // S):
                graphs.replay()
            k %= S
        for _ in range(k):
            fwd(cnt[0])
            cnt[0] += 1
    elapsed = timed_region(D, run_steps, args.warmup, args.steps)
    elapsed, n_total, ranks_seen = D.reduce_max_sum(elapsed, n)
    if D.rank != 0:
        return None
    t_cold = event_time_ms(fwd, span=0 if args.no_graph else max(S, 8))
    t_warm = event_time_ms(lambda i: fwd(0), span=0 if args.no_graph else 8)
    ab = algorithmic_bytes(n, n, C, K, 27, 1)["fwd"]
    r = roofline_obj("fwd", ab, t_cold, f"igemm_i8_sparse_kernel<{K}> (appendix tiles + streaming main tiles; v_mfma_i32_16x16x64_i8)"
                     if K in (64, 128) and C <= 128 else f"igemm_v4_kernel<{K},1,int8,fwd> (v_mfma_i32_16x16x64_i8)",
                     pmc_traffic(f"uniform-i8-c{C}-n{voxels}", "fwd"),
                     {"memory_level": f"HBM: {S} scenes rotated" if S >= 4 else "Infinity Cache (single scene)"})
    res = {"metric": "active-voxels/sec forward, int8 3x3x3 SubMConv3d C=128 (BASELINE config 5)",
           "value": n_total * args.steps / elapsed, "unit": "voxels/s", "n_gpus": D.world, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "i8", "data": "synthetic",
           "config": {"workload": f"int8 SubMConv3d 3x3x3 C={C}->{K}, {n} uniform voxels/scene, per-channel scale + "
                                  f"bias + ReLU, int8 out, inference forward only (BASELINE config 5)",
                      "scenes_rotated": S, "launch": "hipgraph" if graphs is not None else "eager",
                      "mask_sort": scenes[0][2].argsort_fwd is not None,
                      "parallelism": f"dp{D.world}", "ranks_seen": ranks_seen},
           "roofline": r, "roofline_cold": r,
           "roofline_warm": roofline_obj("fwd", ab, t_warm, r["kernel"], None, {"memory_level": "Infinity Cache"})}
    if D.world == 1 and args.full and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline_int8(scenes[0][0], scenes[0][1], C, K)
    return res


# ------------------------------------------------------------------ configs 3 and 4 (whole networks)
def run_net(args, D: Dist):
    import spconv_amd.pytorch as spconv
    from spconv_amd.dist import GradBucket
    from spconv_amd.utils import nets
    dev, world, rank = D.dev, D.world, D.rank
    S = max(1, min(args.scenes, 4))
    voxels = args.voxels or 100_000
    torch.manual_seed(0)
    if args.config == "3":
        net = nets.downsample_chain().to(dev).half().train()
        cin, bs = 16, 1
        kind = args.scene or "fixture"
        batches = [make_scene(kind, voxels, seed=rank * S + si) for si in range(S)]
        name = "SparseConv3d k3 s2 p1 chain 16->32->64->128"
    else:
        net = nets.second_backbone(4).to(dev).half().train()
        cin, bs = 4, 4
        kind = args.scene or "lidar"
        batches = [make_scene(kind, voxels, seed=rank * S + si, batch=bs, shape=nets.SECOND_SHAPE)
                   for si in range(S)]
        name = "SECOND-style VoxelBackBone8x (12 sparse convs + BatchNorm1d + ReLU)"
    key_order = bool(getattr(args, "key_order", False))
    if key_order:
        batches = [(key_sorted(idx_np, shape), shape) for idx_np, shape in batches]
    data = []
    for idx_np, shape in batches:
        ind = torch.from_numpy(idx_np).to(dev)
        f = torch.randn(idx_np.shape[0], cin, device=dev).half()
        data.append((ind, f, shape))
    bucket = GradBucket(net.parameters()) if D.multi else None
    D.init()
    cnt = [0]
    last = {}

    def step():
        ind, f, shape = data[cnt[0] % S]
        cnt[0] += 1
        net.zero_grad(set_to_none=True)
        x = spconv.SparseConvTensor(f.clone().requires_grad_(args.config == "3"), ind, shape, bs)
        y = net(x)
        g = last.get(y.features.shape)
        if g is None:
            g = last[y.features.shape] = (torch.rand(y.features.shape, device=dev) - 0.5).half() * 0.2
        y.features.backward(g)
        if bucket is not None:
            bucket.all_reduce(average=True)
        return y

    def run_steps(k):
        for _ in range(k):
            step()
    warm, steps = args.warmup, args.steps
    elapsed = timed_region(D, run_steps, warm, steps)
    eager_st_ms = None
    if not D.multi:          # the eager step with the autograd engine on the calling thread (run_layer: the recipe)
        with torch.autograd.set_multithreading_enabled(False):
            eager_st_ms = timed_region(D, run_steps, min(warm, 5), steps) / steps * 1e3
    eager_ms, static_info = None, None
    if not args.no_graph and not D.multi:
        # the same step with static shapes, captured (rulebooks included); `value` is from this loop when it
        # ran clean, the eager loop's time rides along
        try:
            t_static, static_info = static_training_steps(net, data, bs, cin, data[0][2], steps, warm, D,
                                                          input_grad=args.config == "3", key_ordered=key_order)
            # accepted when the gradients agree with the eager step as well as the eager step agrees with
            # itself under a permutation of the input rows (bit-identical for networks without BatchNorm)
            if (not static_info["overflowed"] and static_info["dw_rel_diff_vs_eager"]
                    <= max(2e-3, 1.5 * static_info["dw_rel_diff_noise_floor"])):
                eager_ms, elapsed = elapsed / steps * 1e3, t_static
            else:
                static_info["rejected"] = True
        except Exception as e:
            static_info = {"error": f"{type(e).__name__}: {e}"[:300]}
            torch.cuda.synchronize()
    n_mean = sum(b[0].shape[0] for b in batches) / S
    elapsed, n_total, ranks_seen = D.reduce_max_sum(elapsed, n_mean)
    if rank != 0:
        return None
    # algorithmic bytes of every conv layer of one step (fwd + dgrad + wgrad, SURVEY.md 8d formulas)
    recs = []

    def hook(mod, a, out):
        x = a[0]
        recs.append(dict(idx=x.indices.cpu().numpy(), bs=x.batch_size, shape=list(x.spatial_shape),
                         ksize=list(mod.kernel_size), stride=list(mod.stride), padding=list(mod.padding),
                         dilation=list(mod.dilation), subm=mod.subm, C=mod.in_channels, K=mod.out_channels,
                         n_in=x.features.shape[0], n_out=out.features.shape[0]))
    hs = [m.register_forward_hook(hook) for m in nets.conv_layers(net)]
    cnt[0] = 0
    bucket = None        # rank 0 only from here on: no collective in this bookkeeping step
    step()
    for h in hs:
        h.remove()
    total = 0
    for r in recs:
        kv = int(np.prod(r["ksize"]))
        ab = algorithmic_bytes(r["n_in"], r["n_out"], max(r["C"], 8), r["K"], kv, 2)
        total += ab["fwd"] + ab["wgrad"] + (ab["dgrad"] if r is not recs[0] or args.config == "3" else 0)
    ms = elapsed / steps * 1e3
    res = {"metric": f"active-voxels/sec fwd+bwd through {name} (BASELINE config {args.config})",
           "value": n_total * steps / elapsed, "unit": "voxels/s", "n_gpus": world, "steps": steps, "warmup": warm,
           "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f16",
           "data": "synthetic",
           "config": {"workload": f"{name}, fp16, {bs} {kind} scene(s) of ~{voxels} voxels per GPU per step "
                                  f"({int(n_mean)} input voxels), fresh rulebooks every step, forward + backward"
                                  + (" + flat-bucket RCCL gradient all-reduce" if D.multi else ""),
                      "input_voxels_per_gpu": int(n_mean), "layer_voxels": [[r["n_in"], r["n_out"]] for r in recs],
                      "scenes_rotated": S,
                      "launch": "eager" if eager_ms is None else "hipGraph replay of the whole step (static shapes: "
                                "rulebook builds + forward + backward captured once, one graph for every scene)",
                      "static_shapes": static_info, "parallelism": f"dp{world}", "ranks_seen": ranks_seen,
                      "conv_output_order": __import__("spconv_amd.constants", fromlist=["x"]).CONV_OUTPUT_ORDER,
                      "input_row_order": "ascending coordinate key, declared (key_ordered_input)" if key_order
                                         else "generator order (shuffled in space)" +
                                         ("; sorted by coordinate key at the head of the captured step (entry_sort: "
                                          "spx_key_argsort inside the graph and the timed region)"
                                          if (static_info or {}).get("entry_sort") and eager_ms is not None else ""),
                      "dist_backend": D.backend if D.multi else None},
           "roofline": roofline_obj("step", total, ms, "whole step: rulebook builders + igemm_v4 / igemm_bwd / "
                                    "wgrad_reduce2 of every layer (+ the bn_* BatchNorm+ReLU kernels at config 4)", None,
                                    {"memory_level": "HBM (activations of a step exceed the Infinity Cache)",
                                     "note": "algorithmic bytes = conv layers only (SURVEY.md 8d formulas per layer); "
                                             "the time also holds rulebook builds, normalisation layers and host "
                                             "enqueue gaps, so this is the end-to-end fraction, not a kernel's"})}
    res["roofline_cold"] = res["roofline"]
    if eager_ms is not None:
        res["eager_ms_per_step"] = eager_ms
    if eager_st_ms is not None:
        res["eager_ms_per_step_single_thread_autograd"] = eager_st_ms
    if world == 1 and args.full and not args.no_cpu_baseline:
        t, done = cpu_baseline_net(recs)
        frac_layers = done / len(recs)
        res["cpu_baseline"] = {"value": n_mean / t * frac_layers if done < len(recs) else n_mean / t,
                               "unit": "voxels/s", "cores": min(16, os.cpu_count() or 1), "kind": "port",
                               "sample": f"oracle rulebook + forward + backward of the first {done} of {len(recs)} "
                                         f"sparse conv layers of ONE step (conv layers only, no BatchNorm), fp32, "
                                         f"faithful-omp at {min(16, os.cpu_count() or 1)} threads: {t:.1f} s"
                                         + ("" if done == len(recs) else
                                            "; value extrapolated by layer count (bounded sample)")}
    return res


def static_training_steps(net, data, bs, cin, shape, steps, warm, D: Dist, input_grad=True, key_ordered=False):
    """The training step of a network (BASELINE configs 3 and 4) with static shapes: input padded with dead
    rows, every strided layer's output bounded at 1.1 x the largest count over the scenes, rulebook builds +
    forward + backward of the whole step in ONE captured graph that serves every scene
    (spx_conv_rulebook_static: nothing is read back; BatchNorm statistics over the live rows through the
    device-side row count every tensor carries).  Returns (seconds for `steps` steps, info dict); the
    gradients of scene 0 are compared with the eager, unbounded step before anything is timed."""
    import copy
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch.static import StaticTrainingStep, strided_layers
    dev = D.dev
    S = len(data)
    net_e = copy.deepcopy(net)                       # eager, unbounded reference
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, a, out, k=k: seen.__setitem__(k, max(seen.get(k, 0), out.features.shape[0])))
             for k, m in strided_layers(net_e).items()]
    with torch.no_grad():
        for ind, f, _ in data:
            net_e(spconv.SparseConvTensor(f, ind, shape, bs))
    for h in hooks:
        h.remove()
    bounds = {k: int(v * 1.1) + 1 for k, v in seen.items()}
    n_max = int(max(d[0].shape[0] for d in data) * 1.05) + 1
    layers = strided_layers(net)
    k_last = list(layers.values())[-1].out_channels
    gstat = ((torch.rand((bounds[list(layers)[-1]], k_last), device=dev) - 0.5) * 0.2).half()
    runner = StaticTrainingStep(net, n_max, cin, shape, bs, torch.float16, bounds=bounds, out_grad=gstat,
                                input_grad=input_grad, device=dev, example=(data[0][1], data[0][0]),
                                capture_error_mode=CAPTURE_MODE, key_ordered_input=key_ordered)
    fbuf, g = runner.features, runner.graph

    def load(si):
        runner.load(data[si][1], data[si][0])
    # parity of the captured step against the eager, unbounded one (scene 0)
    load(0)
    g.replay()
    y_static = runner.out.features.detach()
    ind, f, _ = data[0]
    fe = f.clone().requires_grad_(input_grad)
    ye = net_e(spconv.SparseConvTensor(fe, ind, shape, bs))
    ye.features.backward(gstat[:ye.features.shape[0]])
    torch.cuda.synchronize()
    worst, per_param = 0.0, []
    for (name, pa), pb in zip(net.named_parameters(), net_e.parameters()):
        d = float((pa.grad.float() - pb.grad.float()).norm() / pb.grad.float().norm().clamp_min(1e-20))
        per_param.append((round(d, 6), name))
        worst = max(worst, d)
    ye_f = ye.features.detach().float()
    out_diff = float((y_static[:ye_f.shape[0]].detach().float() - ye_f).norm() / ye_f.norm().clamp_min(1e-20))
    # noise floor of that comparison: the eager step on the SAME scene with its rows permuted -- mathematically
    # the same gradients, another summation order (with BatchNorm layers and a zero-mean synthetic output
    # gradient the sums are small against their terms, so fp16 rounding flips show up at the percent level)
    perm = torch.randperm(ind.shape[0], device=dev)
    net_p = copy.deepcopy(net_e)
    net_p.zero_grad(set_to_none=True)
    yp = net_p(spconv.SparseConvTensor(f[perm].clone().requires_grad_(input_grad), ind[perm].contiguous(), shape, bs))

    def lin(ix, sh):
        k = ix[:, 0].long()
        for d, extent in enumerate(sh):
            k = k * int(extent) + ix[:, 1 + d].long()
        return k
    ke, kp = lin(ye.indices, ye.spatial_shape), lin(yp.indices, yp.spatial_shape)
    order = torch.argsort(kp)[torch.argsort(torch.argsort(ke))]
    gp = torch.empty_like(gstat[:ye.features.shape[0]])
    gp[order] = gstat[:ye.features.shape[0]]
    yp.features.backward(gp)
    floor = 0.0
    for pa, pb in zip(net_p.parameters(), net_e.parameters()):
        floor = max(floor, float((pa.grad.float() - pb.grad.float()).norm() / pb.grad.float().norm().clamp_min(1e-20)))
    del net_p, yp
    din = None
    if input_grad:
        din = float((fbuf.grad[:ind.shape[0]].float() - fe.grad.float()).norm() / fe.grad.float().norm().clamp_min(1e-20))
    cnt = [0]

    def run_steps(k):
        for _ in range(k):
            load(cnt[0] % S)
            cnt[0] += 1
            g.replay()
    elapsed = timed_region(D, run_steps, warm, steps)
    over = runner.overflowed()
    runner.release_bounds()
    return elapsed, {"bounds": bounds, "padded_input_rows": n_max, "entry_sort": bool(runner.entry_sort and not key_ordered),
                     "input_order_violation": runner.input_order_violation(), "dw_rel_diff_vs_eager": worst, "dw_rel_diff_noise_floor": floor, "out_rel_diff_vs_eager": out_diff,
                     "dw_rel_diff_worst_params": sorted(per_param, reverse=True)[:4],
                     "din_rel_diff_vs_eager": din, "overflowed": over}


def run_infer(args, D: Dist):
    """Configuration 4 as INFERENCE (eval mode, no autograd), two ways on the same scenes: the eager
    forward pass (one device -> host read of the output count per strided layer, ~90 launches enqueued
    from Python) and the static-shape form (spconv_amd/pytorch/static.py: input padded with dead rows,
    every strided layer bounded, rulebook builds and gather-GEMMs of the whole pass in ONE captured
    graph; a step = copy the scene into the static buffers + replay).  Live rows of both are compared
    bit for bit on every scene before anything is timed."""
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch.static import StaticInference, strided_layers
    from spconv_amd.utils import nets
    dev, world, rank = D.dev, D.world, D.rank
    S = max(1, min(args.scenes, 4))
    voxels = args.voxels or 100_000
    torch.manual_seed(0)
    net = nets.second_backbone(4).to(dev).half().eval()
    bs, kind = 4, args.scene or "lidar"
    data = []
    for si in range(S):
        idx_np, shape = make_scene(kind, voxels, seed=rank * S + si, batch=bs, shape=nets.SECOND_SHAPE)
        if getattr(args, "key_order", False):
            idx_np = key_sorted(idx_np, shape)
        data.append((torch.from_numpy(idx_np).to(dev), torch.randn(idx_np.shape[0], 4, device=dev).half(), shape))
    shape = data[0][2]
    D.init()
    # bounds: the largest output count of each strided layer over the scenes + 10 %
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, a, out, k=k: seen.__setitem__(k, max(seen.get(k, 0), out.features.shape[0])))
             for k, m in strided_layers(net).items()]
    # algorithmic bytes of every conv layer's forward (SURVEY.md 8d formula per layer), summed over the scenes
    ab = [0]
    hooks += [m.register_forward_hook(lambda mod, a, out: ab.__setitem__(0, ab[0] + algorithmic_bytes(
        a[0].features.shape[0], out.features.shape[0], max(mod.in_channels, 8), mod.out_channels,
        int(np.prod(mod.kernel_size)), 2)["fwd"])) for m in nets.conv_layers(net)]
    want = []
    with torch.no_grad():
        for ind, f, _ in data:
            y = net(spconv.SparseConvTensor(f, ind, shape, bs))
            want.append((y.indices.clone(), y.features.clone()))
    for h in hooks:
        h.remove()
    cnt = [0]

    def eager_steps(k):
        with torch.no_grad():
            for _ in range(k):
                ind, f, _ = data[cnt[0] % S]
                cnt[0] += 1
                net(spconv.SparseConvTensor(f, ind, shape, bs))
    warm, steps = args.warmup, args.steps
    t_eager = timed_region(D, eager_steps, warm, steps)
    bounds = {k: int(v * 1.1) + 1 for k, v in seen.items()}
    n_max = max(d[0].shape[0] for d in data)
    runner = StaticInference(net, int(n_max * 1.05) + 1, 4, shape, bs, torch.float16, bounds=bounds,
                             capture_error_mode=CAPTURE_MODE, key_ordered_input=bool(getattr(args, "key_order", False)))
    identical = True
    for (ind, f, _), (wi, wf) in zip(data, want):
        got = runner(f, ind)
        n_live = wi.shape[0]
        identical &= bool(torch.equal(got.indices[:n_live], wi) and torch.equal(got.features[:n_live], wf)
                          and bool((got.indices[n_live:, 0] < 0).all()))
    identical &= runner.overflowed() == {}

    def graph_steps(k):
        for _ in range(k):
            ind, f, _ = data[cnt[0] % S]
            cnt[0] += 1
            runner(f, ind)
    elapsed = timed_region(D, graph_steps, warm, steps)
    for m in strided_layers(net).values():
        m.static_num_out = 0
    # deployment form: BatchNorm folded into the convolution weights, ReLU in the kernel's epilogue
    # (quantization/utils.py fold_sequential_eval: 12 layers instead of 36), captured the same way; checked
    # against ITS eager pass (folding rescales fp16 weights, so it is not bit-identical to the unfolded net)
    from spconv_amd.pytorch.quantization.utils import fold_sequential_eval
    folded_ms, folded_ok = None, None
    try:
        fnet = fold_sequential_eval(net)
        with torch.no_grad():
            fwant = [fnet(spconv.SparseConvTensor(f, ind, shape, bs)) for ind, f, _ in data]
            fwant = [(y.indices.clone(), y.features.clone()) for y in fwant]
        frunner = StaticInference(fnet, int(n_max * 1.05) + 1, 4, shape, bs, torch.float16,
                                  bounds={k2: bounds[k] for k, k2 in zip(strided_layers(net), strided_layers(fnet))},
                                  capture_error_mode=CAPTURE_MODE,
                                  key_ordered_input=bool(getattr(args, "key_order", False)))
        folded_ok = True
        for (ind, f, _), (wi, wf) in zip(data, fwant):
            got = frunner(f, ind)
            folded_ok &= bool(torch.equal(got.indices[:wi.shape[0]], wi) and torch.equal(got.features[:wi.shape[0]], wf))

        def folded_steps(k):
            for _ in range(k):
                ind, f, _ = data[cnt[0] % S]
                cnt[0] += 1
                frunner(f, ind)
        folded_ms = timed_region(D, folded_steps, warm, steps) / steps * 1e3
    except Exception as e:
        folded_ok = f"{type(e).__name__}: {e}"[:200]
        torch.cuda.synchronize()
    n_mean = sum(d[0].shape[0] for d in data) / S
    elapsed, n_total, ranks_seen = D.reduce_max_sum(elapsed, n_mean)
    if rank != 0:
        return None
    ms = elapsed / steps * 1e3
    return {"metric": "active-voxels/sec, inference forward through the SECOND-style VoxelBackBone8x, static-shape "
                      "graph replay (BASELINE config 4 network)",
            "value": n_total * steps / elapsed, "unit": "voxels/s", "n_gpus": world, "steps": steps, "warmup": warm,
            "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f16",
            "data": "synthetic",
            "eager_ms_per_step": t_eager / steps * 1e3, "graph_ms_per_step": ms,
            "live_rows_identical_to_eager": identical,
            "bn_folded_graph_ms_per_step": folded_ms, "bn_folded_live_rows_identical_to_its_eager_pass": folded_ok,
            "roofline": roofline_obj("step", ab[0] / S, ms, "whole inference pass: rulebook builders + igemm_v4 of every "
                                     "layer + eval BatchNorm / ReLU", None,
                                     {"note": "algorithmic bytes = conv layers' forward only (SURVEY.md 8d formulas per "
                                              "layer); the time also holds the rulebook builds (about half of it) and the "
                                              "normalisation layers: an end-to-end fraction, not a kernel's"}),
            "config": {"workload": f"12 sparse convs + BatchNorm1d + ReLU, eval mode, fp16, {bs} {kind} scenes of "
                                   f"~{voxels} voxels per step ({int(n_mean)} input voxels), fresh rulebooks every "
                                   f"step INSIDE the graph, input padded to {runner.max_voxels} rows",
                       "bounds": bounds, "input_voxels_per_gpu": int(n_mean), "scenes_rotated": S,
                       "launch": "hipGraph replay (rulebooks + convolutions), one graph for every scene",
                       "conv_output_order": __import__("spconv_amd.constants", fromlist=["x"]).CONV_OUTPUT_ORDER,
                       "input_row_order": "ascending coordinate key, declared (key_ordered_input)"
                                          if getattr(args, "key_order", False) else "generator order (shuffled in space)" +
                                          ("; sorted by coordinate key at the head of the captured pass (entry_sort: "
                                           "spx_key_argsort inside the graph and the timed region)"
                                           if runner.entry_sort else ""),
                       "entry_sort": bool(runner.entry_sort and not getattr(args, "key_order", False)),
                       "parallelism": f"dp{world}", "ranks_seen": ranks_seen}}


def also_block(args, D: Dist):
    """The other BASELINE configurations, a few seconds each, in the SAME process and JSON line as the
    headline (N = 1 only): driver-observed numbers for the dense-neighbourhood layer (2b), the int8
    layer (5), the stride-2 chain (3) and the backbone (4).  Compact: value, time per step, kernel-group
    times, roofline fraction, PMC traffic where a committed pass exists."""
    import copy
    import gc
    out = {}
    for cfg in ("2b", "5", "3", "4", "4i"):
        a = copy.copy(args)
        a.config, a.no_cpu_baseline, a.voxels, a.channels, a.scene = cfg, True, None, None, None
        a.dump_outputs = None                               # the headline's outputs only
        a.scenes = min(args.scenes, 4)
        a.steps = min(args.steps, 400 if cfg in ("2b", "5") else 40)
        a.warmup = min(args.warmup, 40 if cfg in ("2b", "5") else 8)
        t0 = time.perf_counter()
        try:
            r = (run_layer(a, D) if cfg == "2b" else run_int8(a, D) if cfg == "5"
                 else run_infer(a, D) if cfg == "4i" else run_net(a, D))
        except Exception as e:                              # a failing side configuration must not cost the headline
            out[cfg] = {"error": f"{type(e).__name__}: {e}"[:300]}
            continue
        roof = r.get("roofline", {})
        c = {"metric": r["metric"], "value": round(r["value"], 1), "unit": r["unit"],
             "ms_per_step": round(r["ms_per_step"], 5), "steps": r["steps"], "dtype": r["dtype"],
             "workload": r["config"]["workload"], "launch": r["config"].get("launch"),
             "roofline": {k: roof.get(k) for k in ("group", "frac", "achieved", "algorithmic_bytes", "ms", "traffic",
                                                        "traffic_over_algorithmic")},
             "wall_s": None}
        if "kernels" in r:
            c["kernels_ms"] = {k: v["ms"] for k, v in r["kernels"].items()}
        for k in ("rulebook_device_ms", "eager_device_ms_per_step", "graph_ms_per_step", "eager_ms_per_step",
                  "eager_ms_per_step_single_thread_autograd", "eager_device_ms_per_step_default_engine_runs",
                  "live_rows_identical_to_eager", "bn_folded_graph_ms_per_step",
                  "bn_folded_live_rows_identical_to_its_eager_pass"):
            if k in r:
                c[k] = r[k]
        if cfg in ("3", "4", "4i"):
            # the same network with the strided layers' outputs in the CPU reference's first-seen order (the functional
            # API's order; the modules default to ascending coordinate key: spconv_amd.constants.CONV_OUTPUT_ORDER)
            from spconv_amd import constants as _c
            c["conv_output_order"] = _c.CONV_OUTPUT_ORDER
            if _c.CONV_OUTPUT_ORDER != "first_seen":
                keep = _c.CONV_OUTPUT_ORDER
                try:
                    _c.CONV_OUTPUT_ORDER = "first_seen"
                    r2 = run_infer(a, D) if cfg == "4i" else run_net(a, D)
                    c["first_seen_order_ms_per_step"] = round(r2["ms_per_step"], 5)
                    del r2
                except Exception as e:
                    c["first_seen_order_ms_per_step"] = f"{type(e).__name__}: {e}"[:200]
                finally:
                    _c.CONV_OUTPUT_ORDER = keep
        if cfg in ("4", "4i") and not getattr(a, "key_order", False) and os.environ.get("SPCONV_AMD_ENTRY_SORT", "auto") != "0":
            # the same captured pass WITHOUT the entry sort (static.py entry_sort: level 1 in the caller's row order, its
            # rulebooks from a hash table) -- what the sort at the head of the pass buys, sort included
            keep_es = os.environ.get("SPCONV_AMD_ENTRY_SORT")
            try:
                os.environ["SPCONV_AMD_ENTRY_SORT"] = "0"
                r4 = run_infer(a, D) if cfg == "4i" else run_net(a, D)
                c["entry_sort_off_ms_per_step"] = round(r4["ms_per_step"], 5)
                del r4
            except Exception as e:
                c["entry_sort_off_ms_per_step"] = f"{type(e).__name__}: {e}"[:200]
            finally:
                os.environ.pop("SPCONV_AMD_ENTRY_SORT", None)
                if keep_es is not None:
                    os.environ["SPCONV_AMD_ENTRY_SORT"] = keep_es
        if cfg in ("4", "4i") and not getattr(a, "key_order", False):
            # the same network with the scenes handed over in coordinate-key order (a data loader that sorts once:
            # utils.sort_voxels_by_coordinate) and the captured pass told so: level 1 without a hash table
            try:
                a2 = copy.copy(a)
                a2.key_order = True
                r3 = run_infer(a2, D) if cfg == "4i" else run_net(a2, D)
                c["key_ordered_input_ms_per_step"] = round(r3["ms_per_step"], 5)
                del r3
            except Exception as e:
                c["key_ordered_input_ms_per_step"] = f"{type(e).__name__}: {e}"[:200]
        c["wall_s"] = round(time.perf_counter() - t0, 1)
        out[cfg] = c
        del r
        gc.collect()
        torch.cuda.empty_cache()
    return out


def _lib_count(family: str) -> int:
    from spconv_amd import _lib
    return int(_lib.load().spx_launch_count(family.encode()))


def tree_stamp() -> str:
    """Which tree this line measured: `git describe` where there is a repository, else the BUILD_STAMP file that
    tools/grun.sh leaves at the root before a snapshot goes to a GPU box (the box has no .git)."""
    root = os.path.dirname(os.path.abspath(__file__))
    try:
        import subprocess
        h = subprocess.check_output(["git", "-C", root, "rev-parse", "--short=12", "HEAD"], text=True,
                                    stderr=subprocess.DEVNULL).strip()
        dirty = subprocess.call(["git", "-C", root, "diff", "--quiet", "HEAD"], stderr=subprocess.DEVNULL) != 0
        return h + ("+dirty" if dirty else "")
    except Exception:
        pass
    try:
        return open(os.path.join(root, "BUILD_STAMP")).read().split()[0]
    except OSError:
        return "unknown"


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse(argv)
    maybe_spawn(args, argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: torch.cuda.is_available() is False")
    D = Dist()
    if args.gpus != D.world:
        print(f"[bench] --gpus {args.gpus} but the launcher started WORLD_SIZE={D.world}: using {D.world}",
              file=sys.stderr)
    torch.cuda.set_device(D.local_rank)
    D.dev = torch.device("cuda", D.local_rank)
    if args.config in ("2", "2b"):
        result = run_layer(args, D)
    elif args.config == "5":
        result = run_int8(args, D)
    elif args.config == "4i":
        result = run_infer(args, D)
    else:
        result = run_net(args, D)
    if D.rank == 0 and D.world == 1 and args.config == "2" and args.full and not args.no_also:
        result["also"] = also_block(args, D)
        # the same, compact, inside the object the driver's record keeps whole
        result["roofline"]["also"] = {
            cfg: ({"error": c["error"]} if "error" in c else
                  {"value": c["value"], "unit": c["unit"], "ms": c["ms_per_step"], "frac": c["roofline"].get("frac"),
                   "traffic": c["roofline"].get("traffic"),
                   "traffic_over_algorithmic": c["roofline"].get("traffic_over_algorithmic"),
                   "group": c["roofline"].get("group")})
            for cfg, c in result["also"].items()}
    if D.rank == 0:
        result["config"]["tree"] = tree_stamp()
        print(json.dumps(result), flush=True)
    D.finish()


if __name__ == "__main__":
    main()
