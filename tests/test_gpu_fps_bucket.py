"""Farthest-point sampling with bucket pruning (csrc/fps_bucket.hip, ``F.farthest_point_sample_method(...,
method="bucket")``): idx and count equal the numpy restatement tests/refsample.py AND method "scan" on the same input,
bit for bit -- they are integers.  The sizes come from the exported bucket cap and base bucket size."""
import numpy as np
import pytest
import torch

import refsample as rs
import samplescenes as ss

pytestmark = pytest.mark.gpu


def dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(cuda)


def count_of(cuda, n):
    return None if n is None else torch.tensor([n], dtype=torch.int32, device=cuda)


def cloud(sizes, seed, extent=4.0):
    """scene-contiguous uniform points in [0, extent)^3 (4 columns) with `sizes` points per scene"""
    pts = (np.random.default_rng(seed).random((int(sum(sizes)), 4)) * extent).astype(np.float32)
    return pts, np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)


def buckets_of(n):
    from spconv_amd.pytorch import _sample
    size = _sample.bucket_points()
    while -(-n // size) > _sample.bucket_cap():
        size *= 2
    return -(-n // size)


def run(cuda, pts, bid, B, K, ndim=3, n_points=None):
    """the bucket path against refsample and against the scan path; returns (idx, count, visits) as numpy"""
    from spconv_amd.pytorch import functional as F
    args = (dev(cuda, pts), dev(cuda, bid), B, K)
    s, visits = F.farthest_point_sample_method(*args, "bucket", ndim=ndim, n_points=count_of(cuda, n_points),
                                               with_visits=True)
    scan = F.farthest_point_sample_method(*args, "scan", ndim=ndim, n_points=count_of(cuda, n_points))
    idx, count = s.idx.cpu().numpy(), s.count.cpu().numpy()
    want = rs.fps(pts, bid, B, K, ndim, n_points)
    np.testing.assert_array_equal(count, want[1])
    np.testing.assert_array_equal(idx, want[0])
    assert torch.equal(s.idx, scan.idx) and torch.equal(s.count, scan.count) and torch.equal(s.batch_ids, scan.batch_ids)
    return idx, count, visits.cpu().numpy()


@pytest.mark.parametrize("ndim", [3, 2])
@pytest.mark.parametrize("K", [1, 2, 257])
@pytest.mark.parametrize("valid", [(0, 1, 63), (64, 65, 4097)])
def test_three_scenes_bit_for_bit(cuda, valid, K, ndim):
    """every scene with points carries three invalid ones as well (NaN, +inf, -inf); K exceeds some valid counts"""
    sizes = [v + 3 if v else 0 for v in valid]
    pts, bid = cloud(sizes, 200 + sum(valid))
    start = 0
    for n in sizes:
        if n:
            pts[start + 1, 0], pts[start + n // 2, ndim - 1], pts[start + n - 1, 1] = np.nan, np.inf, -np.inf
        start += n
    _, count, _ = run(cuda, pts, bid, 3, K, ndim)
    assert count.tolist() == [min(v, K) for v in valid]


@pytest.mark.parametrize("case", ["doubled_buckets", "two_buckets_per_lane"])
def test_large_scenes(cuda, case):
    """one point more than cap base buckets hold (buckets of two waves); more than 1024 buckets (a lane owns two)"""
    from spconv_amd.pytorch import _sample
    cap, size = _sample.bucket_cap(), _sample.bucket_points()
    n, K = (cap * size + 1, 32) if case == "doubled_buckets" else (1100 * size + 17, 64)
    assert buckets_of(n) == (cap // 2 + 1 if case == "doubled_buckets" else 1101) and cap >= 1101
    pts, bid = cloud([n, 5], 31, extent=60.0)
    _, count, visits = run(cuda, pts, bid, 2, K)
    assert count.tolist() == [K, 5] and visits[0] < K * buckets_of(n)


def test_exact_lattice_and_duplicates(cuda):
    """ties everywhere choose the lowest point index; with duplicates only, box distance and t are both 0 and the chosen
    point's bucket is still updated: distinct ascending indices, over four buckets"""
    idx, _, _ = run(cuda, ss.TIE_POINTS, None, 1, 6)
    assert idx[0].tolist() == ss.TIE_ORDER
    idx, _, _ = run(cuda, np.ascontiguousarray(ss.TIE_POINTS[:, :2]), None, 1, 8, ndim=2)
    assert idx[0].tolist() == ss.TIE_ORDER + [-1, -1]
    lattice = np.stack(np.meshgrid(*[np.arange(9, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    run(cuda, lattice[np.random.default_rng(5).permutation(len(lattice))], None, 1, 300)
    idx, count, _ = run(cuda, np.tile(ss.DUPLICATES[:1], (200, 1)), None, 1, 210)
    assert idx[0].tolist() == list(range(200)) + [-1] * 10 and count.tolist() == [200]


def test_two_clusters_prune(cuda):
    """two tight clusters 100 units apart: bit for bit, and fewer bucket updates than a sampler that visits every bucket
    in every step would make (count x buckets) -- without this a kernel that never prunes passes everything else"""
    rng = np.random.default_rng(77)
    n, K = 4000, 64
    pts = (rng.standard_normal((n, 3)) * 0.5).astype(np.float32)
    pts[rng.random(n) < 0.5, 0] += np.float32(100.0)
    _, count, visits = run(cuda, pts, None, 1, K)
    assert count.tolist() == [K] and buckets_of(n) <= visits[0] < K * buckets_of(n)


def test_interleaved_scenes_equal_the_contiguous_cloud(cuda):
    pts, bid, _, _ = ss.base()
    new_pts, new_bid, new_row = ss.interleaved(pts, bid)
    a, _, _ = run(cuda, pts, bid, ss.B, 128)
    b, _, _ = run(cuda, new_pts, new_bid, ss.B, 128)
    np.testing.assert_array_equal(b, new_row[a])


def test_never_samples_what_is_no_point(cuda):
    pts, bid, _, _ = ss.base()
    pts, bid = pts.copy(), bid.copy()
    live = len(pts) - 300                                            # 300 plausible rows behind the device count
    bid[3::11], bid[4::11] = -1, ss.B
    pts[5::11, 0], pts[6::11, 2], pts[0, 1] = np.nan, np.inf, -np.inf
    idx, _, _ = run(cuda, pts, bid, ss.B, 200, n_points=live)
    got = idx.reshape(-1)
    assert got.min() >= 1 and got.max() < live and np.isfinite(pts[got, :3]).all()
    assert (np.repeat(np.arange(ss.B), 200) == bid[got]).all()
    bad = pts[:50].copy()
    bad[:, 1] = np.nan
    idx, count, visits = run(cuda, bad, None, 1, 8)
    assert (idx == -1).all() and count.tolist() == [0] and visits.tolist() == [0]


def buffers(cuda, N, B, K, ndim=3):
    from spconv_amd.pytorch import _sample
    ws = torch.empty((_sample.fps_bucket_ws_bytes(N, B, ndim),), dtype=torch.uint8, device=cuda)
    return (torch.empty((B, K), dtype=torch.int32, device=cuda), torch.empty((B,), dtype=torch.int32, device=cuda), ws,
            torch.empty((B,), dtype=torch.int32, device=cuda))


def test_dirty_workspace_two_runs_identical(cuda):
    """the workspace holds NaN (all bits set) before each run; the sampling alone may run again on one build"""
    from spconv_amd import _lib
    from spconv_amd.pytorch import functional as F
    pts, bid, _, _ = ss.base()
    p = dev(cuda, pts)
    groups = F.scene_groups(dev(cuda, bid), len(pts), ss.B)
    want = rs.fps(pts, bid, ss.B, 150)
    runs = []
    for _ in range(2):
        idx, count, ws, visits = buffers(cuda, len(pts), ss.B, 150)
        for t in (idx, count, ws, visits):
            t.view(torch.uint8).fill_(0xff)
        F.fps_bucket_into(p, groups, 150, 3, idx, count, ws, visits)
        runs.append((idx.clone(), count.clone(), visits.clone()))
        np.testing.assert_array_equal(idx.cpu().numpy(), want[0])
        idx.fill_(7)
        _lib.check(_lib.load().spx_fps_bucket(len(pts), 3, ss.B, 150, idx.data_ptr(), count.data_ptr(), None, ws.data_ptr(),
                                              ws.numel(), torch.cuda.current_stream().cuda_stream))
        np.testing.assert_array_equal(idx.cpu().numpy(), want[0])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_capture_build_and_sampling_in_one_graph(cuda):
    """scene groups -> build -> sampling in one graph, replayed on a second cloud with another device point count"""
    from spconv_amd.pytorch import functional as F
    base_pts, base_bid, _, _ = ss.base()
    other_pts, other_bid, _ = ss.interleaved(base_pts * np.float32(0.97), base_bid, seed=9)
    sets = [(base_pts, base_bid, len(base_pts)), (other_pts, other_bid, len(base_pts) - 700)]
    want = [rs.fps(p, b, ss.B, 96, n_points=live) for p, b, live in sets]
    N = len(base_pts)
    points = torch.empty((N, 4), dtype=torch.float32, device=cuda)
    bid = torch.empty((N,), dtype=torch.int32, device=cuda)
    n_points = torch.empty((1,), dtype=torch.int32, device=cuda)
    idx, count, ws, visits = buffers(cuda, N, ss.B, 96)

    def step():
        F.fps_bucket_into(points, F.scene_groups(bid, N, ss.B, n_points), 96, 3, idx, count, ws, visits)

    def load(k):
        points.copy_(dev(cuda, sets[k][0]))
        bid.copy_(dev(cuda, sets[k][1]))
        n_points.fill_(sets[k][2])
    load(0)
    step()                                                           # (eager once: nothing allocates under capture but the groups)
    np.testing.assert_array_equal(idx.cpu().numpy(), want[0][0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for k in (1, 0, 1):
        load(k)
        idx.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(idx.cpu().numpy(), want[k][0])
        np.testing.assert_array_equal(count.cpu().numpy(), want[k][1])
    assert not np.array_equal(want[0][0], want[1][0])
