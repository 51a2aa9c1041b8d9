"""Instance clustering (csrc/cluster.hip, ``F.cluster_points``): root, cluster_of_point, count and the clusters' groups
equal an all-pairs float32 loop with ``F.ball_query``'s predicate followed by a Python union-find, exactly -- they are
integers.  Coordinates sit on a lattice of multiples of 0.125 with radius 0.5, so d2 == r2 is hit on purpose and must
NOT link; the cell edge is then 0.5078125, also exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

R, V = 0.5, 0.5 * (1 + 2.0 ** -6)


def reference(pts, bid, B, radius, rng, labels=None, valid=None, min_points=1, n_points=None):
    """(root [N], cluster_of_point [N], members: one ascending index array per kept cluster, by ascending root)"""
    p, N = pts[:, :3].astype(np.float32), len(pts)
    r2 = np.float32(radius) * np.float32(radius)
    b = np.zeros(N, np.int32) if bid is None else bid
    lab = np.zeros(N, np.int32) if labels is None else labels
    with np.errstate(invalid="ignore"):
        take = ((p >= np.float32(rng[:3])) & (p < np.float32(rng[3:]))).all(1)          # (false for NaN, Inf is outside)
    take &= (np.arange(N) < (N if n_points is None else n_points)) & (b >= 0) & (b < B) & (lab >= 0)
    if valid is not None:
        take &= valid.astype(bool)
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    idx = np.flatnonzero(take)
    for k, i in enumerate(idx):
        js = idx[k + 1:]
        d = p[js] - p[i]
        s = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]                  # float32, every operation rounded on its own
        s = s + d[:, 2] * d[:, 2]
        for j in js[(s < r2) & (b[js] == b[i]) & (lab[js] == lab[i])]:
            ra, rb = find(i), find(int(j))
            parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(i) if take[i] else -1 for i in range(N)], np.int32)
    cluster, members = np.full(N, -1, np.int32), []
    for r in np.unique(root[root >= 0]):                           # ascending root
        m = np.flatnonzero(root == r)
        if isinstance(min_points, np.ndarray):
            keep = lab[r] < len(min_points) and np.float32(len(m)) >= min_points[lab[r]]
        else:
            keep = len(m) >= min_points
        if keep:
            cluster[m] = len(members)
            members.append(m.astype(np.int32))
    return root, cluster, members


def dev(cuda, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def same(c, want):
    """a PointClusters against the reference's triple; returns the cluster count"""
    root, cluster, members = want
    count = int(c.count.item())
    assert int(c.status.item()) == 0
    np.testing.assert_array_equal(c.root.cpu().numpy(), root)
    np.testing.assert_array_equal(c.cluster_of_point.cpu().numpy(), cluster)
    assert count == len(members) <= c.cap and c.groups.rows is c.cluster_of_point and c.groups.n_live is c.count
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
    np.testing.assert_array_equal(c.groups.offsets.cpu().numpy()[:count + 1], offsets)
    np.testing.assert_array_equal(c.groups.list.cpu().numpy()[:offsets[-1]], np.concatenate(members + [np.zeros(0, np.int32)]))
    return count


def check(cuda, pts, bid, B, rng, labels=None, valid=None, min_points=1, n_points=None):
    from spconv_amd.pytorch import functional as F
    n_dev = None if n_points is None else torch.tensor([n_points], dtype=torch.int32, device=cuda)
    mp = dev(cuda, min_points) if isinstance(min_points, np.ndarray) else min_points
    c = F.cluster_points(dev(cuda, pts), dev(cuda, bid), B, R, rng, labels=dev(cuda, labels), valid=dev(cuda, valid),
                         min_points=mp, n_points=n_dev)
    want = reference(pts, bid, B, R, rng, labels, valid, min_points, n_points)
    return c, want, same(c, want)


@pytest.mark.parametrize("twin, components", [(R, 2), (0.875 * R, 1)])
def test_long_chain(cuda, twin, components):
    """1 500 points spaced 0.75 r in shuffled index order: long parent chains, hooking across workgroups; a twin chain
    exactly r away stays separate, one 0.875 r away merges"""
    x = np.arange(1500, dtype=np.float32) * np.float32(0.75 * R)
    pts = np.zeros((3000, 3), np.float32)
    pts[:, 0], pts[1500:, 1] = np.tile(x, 2), twin
    pts = pts[np.random.default_rng(5).permutation(3000)]
    assert check(cuda, pts, None, 1, [0, 0, 0, 600, 4, 4])[2] == components


def test_cell_stencil(cuda):
    """one pair per scene: the 26 neighbour directions straddling a face, edge or corner within r; pairs two cells
    apart; and per axis points an ulp below, on and an ulp above a cell boundary with a partner just inside r on either
    side -- (p - lo) / vsize rounds there, which the widened cell edge has to absorb"""
    lo = np.float32(-1.0)
    mid, up, down = lo + np.float32(1.75), lo + np.float32(4 * V), lo + np.float32(3 * V)     # cell 3 of every axis
    pairs = []
    for d in np.ndindex(3, 3, 3):
        d = np.array(d) - 1
        if d.any():
            a = np.where(d > 0, up - 0.125, np.where(d < 0, down + 0.125, mid))
            pairs.append((a, a + 0.25 * d))
    for ax in range(3):
        e = np.eye(3, dtype=np.float32)[ax]
        pairs.append((mid + e * (up - mid - 2.0 ** -10), mid + e * (up + np.float32(V) - mid + 2.0 ** -10)))
        for edge in (np.nextafter(up, np.float32(-np.inf)), up, np.nextafter(up, np.float32(np.inf))):
            for sign in (-1, 1):
                pairs.append((mid + e * (edge - mid), mid + e * (edge - mid + sign * np.float32(R - 2.0 ** -20))))
    pts = np.array(pairs, np.float32).reshape(-1, 3)
    bid = np.repeat(np.arange(len(pairs), dtype=np.int32), 2)
    _, (root, _, _), count = check(cuda, pts, bid, len(pairs), [-1, -1, -1, 3, 3, 3])
    assert (root[1:52:2] == root[0:52:2]).all() and count < len(pts)            # the 26 directions link


@pytest.mark.parametrize("n", [65, 300])
def test_crowded_cell(cuda, n):
    """n points in ONE cell, duplicates included (a run longer than a wave / than a workgroup), and a few around it"""
    rng = np.random.default_rng(n)
    pts = np.concatenate([rng.integers(0, 16, (n, 3)) / 32.0, rng.integers(0, 12, (40, 3)) * 0.125]).astype(np.float32)
    pts[1], pts[n - 1] = pts[0], pts[2]
    check(cuda, pts[rng.permutation(len(pts))], None, 1, [0, 0, 0, 2, 2, 2])


def test_separation(cuda):
    """identical coordinates in two scenes and under two labels never link; valid off, label -1, NaN / Inf, outside the
    range, a foreign batch id and rows beyond n_points take no part: -1"""
    blob = (np.random.default_rng(1).integers(0, 8, (12, 3)) * 0.125).astype(np.float32)
    pts = np.tile(blob, (9, 1))
    N = len(pts)
    bid, labels, valid = np.zeros(N, np.int32), np.zeros(N, np.int32), np.ones(N, np.uint8)
    bid[12:24], labels[24:36], valid[36:48], labels[48:60] = 1, 1, 0, -1
    pts[60:64, 0], pts[64:68, 1], pts[68:72, 2] = np.nan, np.inf, -np.inf
    pts[72:78, 0], pts[78:84, 2] = 2.0, -0.125                                    # hi is exclusive, below lo
    bid[84:90], bid[90:96] = 2, -1
    c, (root, cluster, _), _ = check(cuda, pts, bid, 2, [0, 0, 0, 2, 2, 2], labels, valid, n_points=N - 12)
    assert (root[36:] == -1).all() and (cluster[36:] == -1).all() and (root[:36] >= 0).all()
    assert not set(root[:12]) & set(root[12:24]) and not set(root[:12]) & set(root[24:36])


@pytest.mark.parametrize("sizes, labels, min_points, kept", [
    ([2, 3, 3, 2, 4], None, 3, 3),                                # min_points - 1 is dropped, min_points is kept
    ([3, 3, 3, 3, 3], None, 3, 5),                                # N // min_points clusters: the cap exactly reached
    ([3, 3, 4, 3, 2], [0, 1, 1, 2, 0], np.array([2.5, 4.0], np.float32), 2),   # per label; label 2 is beyond the table
])
def test_filter_and_numbering(cuda, sizes, labels, min_points, kept):
    comp = np.repeat(np.arange(len(sizes)), sizes)
    pts = np.zeros((len(comp), 3), np.float32)
    pts[:, 0], pts[:, 1] = comp * 2.0, np.concatenate([np.arange(s) for s in sizes]) * 0.25
    order = np.random.default_rng(3).permutation(len(comp))
    lab = None if labels is None else np.array(labels, np.int32)[comp][order]
    c, (root, cluster, members), count = check(cuda, pts[order], None, 1, [0, 0, 0, 16, 4, 4], lab, None, min_points)
    assert count == kept and (kept < 5 or c.cap == kept)
    firsts = [m[0] for m in members]
    assert firsts == sorted(firsts) and all(root[m[0]] == m[0] for m in members)      # numbered by ascending root


@pytest.mark.parametrize("B, extent", [(1, 10.0), (3, 7.0)])
@pytest.mark.parametrize("seed", [0, 1])
def test_random_clouds(cuda, seed, B, extent):
    """a few hundred components of mixed size, scenes interleaved, a device point count below N; the max over every
    cluster's feature rows through the groups"""
    from spconv_amd.pytorch import functional as F
    rng = np.random.default_rng(seed)
    pts = (rng.integers(0, int(extent * 8), (3000, 3)) * 0.125).astype(np.float32)
    bid = rng.integers(0, B, 3000).astype(np.int32)
    c, (_, _, members), count = check(cuda, pts, bid, B, [0, 0, 0, extent, extent, extent], min_points=2,
                                      n_points=3000 - int(rng.integers(1, 200)))
    assert count >= 100 and len({len(m) for m in members}) > 3
    feat = rng.standard_normal((3000, 5)).astype(np.float32)
    pooled = F.points_to_voxels(dev(cuda, feat), c.groups, "max").cpu().numpy()
    np.testing.assert_array_equal(pooled[:count], np.stack([feat[m].max(0) for m in members]))
    assert not pooled[count:].any()


def test_capture_replays(cuda):
    """cluster_points_into captured once; replayed with a second cloud and a smaller device count"""
    from spconv_amd.pytorch import functional as F
    N, rng_xyz, gen = 2000, [0, 0, 0, 8, 8, 8], np.random.default_rng(7)
    clouds = [(gen.integers(0, 64, (N, 3)) * 0.125).astype(np.float32) for _ in range(2)]
    plan = F.cluster_plan(R, rng_xyz, 1)
    buf = F.cluster_buffers(N, plan, F.cluster_cap(N, 2), cuda)
    pts, n_dev = torch.zeros((N, 3), device=cuda), torch.zeros((1,), dtype=torch.int32, device=cuda)
    run = lambda: F.cluster_points_into(pts, None, n_dev, plan, None, None, 2, buf)
    run()                                                          # (modules loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = run()
    for cloud, n in zip(clouds, (N, N - 301)):
        pts.copy_(dev(cuda, cloud))
        n_dev.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        same(c, reference(cloud, None, 1, R, rng_xyz, min_points=2, n_points=n))
