"""Loaders for the committed golden fixtures (see make_golden.py)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_case(name):
    return dict(np.load(os.path.join(HERE, f"case_{name}.npz")))


def case_names():
    return sorted(f[5:-4] for f in os.listdir(HERE) if f.startswith("case_") and f.endswith(".npz"))


def lidar_scene(shuffle_seed=0):
    """int32 [125562, 4] (b=0, z, y, x) coordinates of the reference's real-LiDAR fixture
    (test/data/test_spconv.pkl), in a seeded shuffled order, and the spatial shape."""
    d = np.load(os.path.join(HERE, "lidar_scene.npz"))
    shape = [int(v) for v in d["shape"]]
    lin = np.cumsum(d["delta"].astype(np.int64))
    if shuffle_seed is not None:
        np.random.default_rng(shuffle_seed).shuffle(lin)
    coords = np.stack(np.unravel_index(lin, shape), axis=-1).astype(np.int32)
    idx = np.concatenate([np.zeros((coords.shape[0], 1), dtype=np.int32), coords], axis=1)
    return np.ascontiguousarray(idx), shape


# ---- vectors produced by executing the reference's own CPU code (make_ref_golden.py) ----
def ref_case_names():
    return sorted(f[4:-4] for f in os.listdir(HERE) if f.startswith("ref_") and f.endswith(".npz"))


def load_ref_case(name):
    d = dict(np.load(os.path.join(HERE, f"ref_{name}.npz")))
    for k in ("shape", "ksize", "stride", "pad", "dil", "out_shape"):
        d[k] = [int(v) for v in d[k]]
    d["bs"], d["subm"], d["transposed"] = int(d["bs"]), bool(d["subm"]), bool(d["transposed"])
    return d


def ref_digests():
    import json
    with open(os.path.join(HERE, "ref_digests.json")) as f:
        return json.load(f)


def digest(*arrays):
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def ref_big_inputs(name):
    """Inputs of a ref_digests.json entry, regenerated from seeds / the committed fixture; chain
    levels need the previous level's output coordinates, which the caller supplies."""
    from spconv_amd.utils import synthetic
    if name == "cfg1_subm":
        return synthetic.uniform_scene([64, 64, 64], 5000, 1, seed=0), [64, 64, 64]
    if name == "cfg2_subm":
        return synthetic.uniform_scene([40, 1280, 1600], 100_000, 1, seed=0), [40, 1280, 1600]
    if name in ("fixture_subm", "fixture_chain_l0"):
        return lidar_scene()
    raise KeyError(name)


# ---- seeded inputs of the three tests that also run against the live library (oracle/_ref) where it exists; what the
# reference's own code made of them is stored in ref_live_digests.json (make_ref_live_golden.py)
def ref_live_digests():
    import json
    with open(os.path.join(HERE, "ref_live_digests.json")) as f:
        return json.load(f)


def rulebook_sweep_cases():
    """40 random rulebook problems (1-4 d, SubM / strided / transposed): (idx, bs, shape, ksize, stride, pad, dil, subm,
    transposed)."""
    from spconv_amd.utils import synthetic
    rng = np.random.default_rng(2024)
    for trial in range(40):
        nd = int(rng.integers(1, 5))
        shape = [int(v) for v in rng.integers(6, 20 if nd > 2 else 60, nd)]
        bs = int(rng.integers(1, 4))
        n = int(min(rng.integers(1, 800), np.prod(shape) // 2))
        subm = bool(rng.integers(0, 2))
        transposed = (not subm) and bool(rng.integers(0, 3) == 0)
        ksize = [int(v) for v in (rng.choice([1, 3, 5], nd) if subm else rng.integers(1, 4, nd))]
        stride = [1] * nd if subm else [int(v) for v in rng.integers(1, 4, nd)]
        dil = [int(v) for v in rng.integers(1, 3, nd)]
        pad = [int(v) for v in rng.integers(0, 3, nd)]
        idx = synthetic.uniform_scene(shape, n, bs, seed=trial)
        yield idx, bs, shape, ksize, stride, pad, dil, subm, transposed


def native_loop_cases(dyadic):
    """The per-offset conv loop's problems (SubM, stride 2): (key, idx, bs, shape, subm, stride, f, w, g).  dyadic: values
    k / 64 in [-1, 1], so that every sum of the loop is exact in fp32 and its result cannot depend on the GEMM's order."""
    import torch
    from spconv_amd.utils import synthetic
    import oracle
    rng = np.random.default_rng(5)
    C, K = 5, 7

    def values(shape):
        if dyadic:
            return torch.from_numpy((rng.integers(-64, 65, shape) / 64.0).astype(np.float32))
        return torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32))
    for subm, stride in ((True, 1), (False, 2)):
        shape, bs = [14, 15, 16], 2
        idx = synthetic.uniform_scene(shape, 700, bs, seed=3)
        out_inds, pair, num, _ = oracle.get_indice_pairs(idx, bs, shape, [3] * 3, [stride] * 3, [1] * 3, [1] * 3,
                                                         None, subm, False)
        f, w, g = values((idx.shape[0], C)), values((K, 3, 3, 3, C)), values((out_inds.shape[0], K))
        yield f"subm{int(subm)}_s{stride}", out_inds, pair, num, subm, f, w, g


def section_8f_inputs():
    """Points of the voxeliser runs and the max-pool problem of the section-8f live comparison."""
    from spconv_amd.utils import synthetic
    import oracle
    rng = np.random.default_rng(8)
    p2v = []
    for seed in range(3):
        pts = rng.uniform((-1, -5, -3, 0), (9, 5, 3, 1), (3000, 4)).astype(np.float32)
        pts[:1500, :3] = pts[:1500, :3] * 0.03 + np.float32(2.0)
        p2v.append((pts, [0.2, 0.1, 0.1], [-2, -4, 0, 2, 4, 8], [20, 80, 80], 900 + 2000 * seed))
    idx = synthetic.uniform_scene([16, 16, 16], 1200, 2, 5)
    _, pair, num, _ = oracle.get_indice_pairs(idx, 2, [16] * 3, [2] * 3, [2] * 3, [0] * 3, [1] * 3, None, False, False)
    n_out = int(pair[1].max()) + 1
    f = (rng.integers(-64, 65, (idx.shape[0], 5)) / 64.0).astype(np.float32)
    dout = (rng.integers(-32, 33, (n_out, 5)) / 64.0).astype(np.float32)
    return p2v, (pair, num, n_out, f, dout)
