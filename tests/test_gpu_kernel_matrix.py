"""Every reachable gather-GEMM / backward / wgrad kernel INSTANCE against the fp64 reference of refconv.py.

Each case names the entry it calls, its scene, dtype, widths, kernel geometry and table form, and the instance key
(include/spconv_amd.h, spx_launch_count) the dispatcher must reach.  A case snapshots that key's counter, runs the
entry eagerly, asserts that the counter moved, and compares every output element with util.assert_close_abs_sum
against the fp64 reference (c = 1e-6 for 16-bit tensors, 1e-5 for fp32), on inputs rounded to the kernel dtype.

reachable() lists the instances the dispatchers can produce; the CPU test at the end asserts that the cases claim every
one of them but the EXCLUDED ones, so a new kernel variant cannot land without a reference case."""
import fnmatch
import functools
import zlib

import numpy as np
import pytest
import torch

from refconv import conv_from_pairs, out_spatial_shape, pairs
from util import HALF_ULP, assert_close_abs_sum, match_rows

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTN = {F16: "f16", BF16: "bf16", F32: "f32"}
MFMA_COUT = (16, 32, 64, 128, 256)
# (NKS, PK) forms of a 16-bit launch: v4_pack (igemm_v4.h:832-841) and the launch switches (:858-885, igemm_bwd.h:386-396)
FORMS16 = [(1, 4), (1, 2), (1, 1), (2, 1), (2, 32), (2, 16), (2, 8)]


# ---------------------------------------------------------------- dispatch model (the keys a call must reach)
def lane(dtype):
    return 4 if dtype == F32 else 8


def padw(c, dtype):
    return -(-c // lane(dtype)) * lane(dtype)


def round_cout(c):
    for v in MFMA_COUT:
        if c <= v:
            return v
    return 0


def pack_form(dtype, red, mode, fused):
    """(NKS, PK) of a 16-bit launch with reduction rows of `red` channels (v4_pack + the launch switch)."""
    rb = red * 2
    if mode == 0:
        pk = 1
    elif mode == 3 or (mode == 1 and fused):
        pk = 32 if rb <= 16 else (16 if rb <= 32 else (8 if rb <= 64 else 1))
    else:
        pk = 4 if rb <= 16 else (2 if rb <= 32 else 1)
    if pk in (32, 16, 8):
        return 2, pk
    if pk in (4, 2):
        return 1, pk
    return (1, 1) if rb <= 64 else (2, 1)


def v4_key(dtype, red, cout, n_dst, bt, pk_mode=1):
    """igemm_v4 instance of a forward (bt False) / dgrad (bt True) with kv <= 128 (grouped launches included)."""
    if dtype == F32:                      # igemm_f32.hip:8-15: 128-row tiles but at 256; NKS by row bytes
        mb = 1 if cout == 256 else 2
        nks, pk = (1 if red * 4 <= 64 else 2), 1
    else:                                 # igemm_v4.h:1075 tile height rule
        mb = 1 if (n_dst <= 32 * 1024 or cout >= 128) else 2
        nks, pk = pack_form(dtype, red, pk_mode, False)
    return f"igemm_v4/{cout}/{mb}/{DTN[dtype]}/{'bt' if bt else 'fwd'}/{nks}/{pk}"


def bwd_key(dtype, C, K, pk_mode=1):
    """igemm_bwd instance of the fused backward (dispatch_bwd, igemm_bwd.h:400-409: MB = 2; dgrad rows are K wide)."""
    if dtype == F32:
        nks, pk = (1 if K * 4 <= 64 else 2), 1
    else:
        nks, pk = pack_form(dtype, K, pk_mode, True)
    return f"igemm_bwd/{C}/2/{DTN[dtype]}/{nks}/{pk}"


def wgrad_key(dtype, C, K):
    """first stage of spx_igemm_wgrad for lane-multiple widths (igemm_wgrad.hip igemm_wgrad_impl: sl from the padded widths)."""
    if dtype == F32:
        return "wgrad_f32"
    C, K = padw(C, dtype), padw(K, dtype)
    sl = 2 if (C <= 16 and K <= 16) else (4 if (C <= 32 and K <= 32) else 8)
    return f"wgrad_tr/{DTN[dtype]}/{sl}"


def reachable():
    """Every instance the dispatchers can launch, read off the switches:
    - igemm_v4, 16-bit: dispatch_gather_gemm (igemm_v4.h:1062-1098): COUT 16 / 32 / 64 with MB 1 / 2, 128 and 256 with
      MB 1 only; launch_v4 (:843-890) BT for dgrad (strideD != 1), the seven (NKS, PK) forms of v4_pack (:832-841)
      under SPX_PK = 1 / 2 / 3 / 0;
    - igemm_v4, fp32: dispatch_gather_gemm_f32 (igemm_f32.hip:8-15), NKS 1 / 2, PK 1;
    - igemm_v4, int8: dispatch of igemm_i8.hip:15-21 (forward only: launch_v4 never takes BT for DT 2);
    - igemm_bwd: dispatch_bwd (igemm_bwd.h:400-409) for COUT 16..128, MB 2; launch_bwd's forms (:386-396);
    - igemm_ws: launch_gather_gemm_ws (igemm_ws.hip:413-445), f16 / bf16;
    - igemm_bwd_rows: spx_igemm_bwd_rows (igemm_bwdn.hip:431-435): eight waves at C = K = 16 only;
    - wgrad_tr / wgrad_f32 / wgrad_mfma / wgrad_generic: igemm_wgrad_impl (igemm_wgrad.hip:749-828);
    - generic: run_gather_gemm_single (igemm.hip:105-134); gen1: launch_gen1_cout (igemm_gen1.hip:284-293)."""
    keys = set()
    for dt in ("f16", "bf16"):
        for cout, mb in ((16, 1), (16, 2), (32, 1), (32, 2), (64, 1), (64, 2), (128, 1), (256, 1)):
            for bt in ("fwd", "bt"):
                for nks, pk in FORMS16:
                    keys.add(f"igemm_v4/{cout}/{mb}/{dt}/{bt}/{nks}/{pk}")
        for cout in (16, 32, 64, 128):
            for nks, pk in FORMS16:
                keys.add(f"igemm_bwd/{cout}/2/{dt}/{nks}/{pk}")
        keys.add(f"igemm_ws/{dt}")
        for c, k in ((16, 16), (16, 32), (32, 16), (32, 32)):
            keys.add(f"igemm_bwd_rows/{c}/{k}/{dt}/{1 if c == k == 16 else 0}")
        for sl in (2, 4, 8):
            keys.add(f"wgrad_tr/{dt}/{sl}")
        keys.add(f"wgrad_mfma/{dt}")
        for cout in MFMA_COUT:
            keys.add(f"gen1/{cout}/{dt}")
    for cout in MFMA_COUT:
        mb = 1 if cout == 256 else 2
        for bt in ("fwd", "bt"):
            for nks in (1, 2):
                keys.add(f"igemm_v4/{cout}/{mb}/f32/{bt}/{nks}/1")
    for cout in (16, 32, 64, 128):
        for nks in (1, 2):
            keys.add(f"igemm_bwd/{cout}/2/f32/{nks}/1")
    for cout, mb in ((16, 2), (32, 2), (64, 2), (128, 1), (128, 2), (256, 1)):
        for nks in (1, 2):
            keys.add(f"igemm_v4/{cout}/{mb}/i8/fwd/{nks}/1")
    keys.add("wgrad_f32")
    for dt in ("f16", "bf16", "f32"):
        keys.add(f"wgrad_generic/{dt}")
        keys.add(f"generic/{dt}")
    return keys


# Instances deliberately without a case here, and why
EXCLUDED = [
    ("igemm_v4/*/*/i8/*", "int8 instances have a matrix of their own, bit for bit against refint8.py: test_gpu_int8_matrix.py, "
                          "whose test_cases_claim_every_int8_instance holds every one of these keys to a case"),
    ("gen1/*", "first-generation kernel: only tensors beyond 32-bit buffer offsets (multi-GB) reach it; "
               "test_gpu_conv.py covers that form"),
    ("wgrad_mfma/*", "16-bit wgrad fallback: only pair lists beyond 32-bit offsets (n_in * 4 * (kv + 1) >= 2 GiB) reach it"),
]


# ---------------------------------------------------------------- scenes and geometries
GEOMS = {
    # ksize, stride, padding, dilation, subm
    "subm3": ([3, 3, 3], [1] * 3, [1] * 3, [1] * 3, True),
    "subm3d2": ([3, 3, 3], [1] * 3, [2] * 3, [2] * 3, True),
    "s2": ([3, 3, 3], [2] * 3, [1] * 3, [1] * 3, False),
    "k2s2": ([2, 2, 2], [2] * 3, [0] * 3, [1] * 3, False),
    "k2s1": ([2, 2, 2], [1] * 3, [0] * 3, [1] * 3, False),          # kv 8, regular, stride 1
    "line": ([1, 1, 3], [1] * 3, [0, 0, 1], [1] * 3, True),         # kv 3: cheap large-row SubM scenes
    "lines2": ([1, 1, 3], [1, 1, 2], [0, 0, 1], [1] * 3, False),    # kv 3, strided
    "k1": ([1, 1, 1], [1] * 3, [0] * 3, [1] * 3, True),             # kv 1
    "k45": ([5, 3, 3], [1] * 3, [2, 1, 1], [1] * 3, True),          # grouped: two mask words
    "k125": ([5, 5, 5], [1] * 3, [2] * 3, [1] * 3, True),           # grouped: four mask words
    "k216": ([6, 6, 6], [2] * 3, [2] * 3, [1] * 3, False),          # generic kernel; wgrad in groups of 128
    "k343": ([7, 7, 7], [1] * 3, [3] * 3, [1] * 3, True),
}

SCENES = {
    # kind, shape, voxels per scene, batch, seed
    "small": ("u", [16, 16, 16], 1500, 2, 1),
    "mid": ("u", [20, 20, 20], 2500, 1, 2),
    "n1": ("u", [4, 4, 4], 1, 1, 3),
    "n63": ("u", [6, 6, 6], 63, 1, 4),
    "n65": ("u", [6, 6, 6], 65, 1, 5),
    "n32768": ("u", [40, 40, 40], 32768, 1, 6),
    "n32769": ("u", [20, 60, 60], 32769, 1, 7),          # dense class when it carries a rows layout
    "n33025": ("u", [40, 1280, 1600], 33025, 1, 8),      # 128 x 258 + 1 rows, sparse class
    "n40000": ("u", [24, 60, 80], 40000, 1, 9),
    "empty1": ("gap", [16, 16, 16], 800, 3, 10),         # batch 1 of 3 holds nothing
    "big524k": ("u", [40, 200, 200], 524289, 1, 11),
    "n106k": ("u", [40, 400, 400], 106496, 1, 12),
    "n115k": ("u", [40, 400, 400], 114689, 1, 13),
}


@functools.lru_cache(maxsize=None)
def scene_indices(name):
    from spconv_amd.utils import synthetic
    kind, shape, n, bs, seed = SCENES[name]
    if kind == "gap":
        idx = synthetic.uniform_scene(shape, n, bs, seed)
        idx = idx[idx[:, 0] != 1]
    else:
        idx = synthetic.uniform_scene(shape, n, bs, seed)
    return np.ascontiguousarray(idx.astype(np.int32)), shape, bs


_RB = {}


def rulebook(scene, geom, table):
    key = (scene, geom, table)
    if key not in _RB:
        from util import gpu_rulebook
        if len(_RB) > 24:
            _RB.clear()
        idx, shape, bs = scene_indices(scene)
        ks, st, pd, dl, subm = GEOMS[geom]
        sort = {"row": False, "sort": True, "layout": "layout"}[table]
        _RB[key] = gpu_rulebook(idx, bs, shape, ks, st, pd, dl, subm, do_sort=sort)[0]
    return _RB[key]


_PAIRS = {}


def ref_pairs(scene, geom, dev):
    key = (scene, geom)
    if key not in _PAIRS:
        if len(_PAIRS) > 24:
            _PAIRS.clear()
        idx, shape, bs = scene_indices(scene)
        ks, st, pd, dl, subm = GEOMS[geom]
        _PAIRS[key] = pairs(idx, bs, shape, ks, st, pd, dl, subm, device=dev)
    return _PAIRS[key]


# ---------------------------------------------------------------- the case table
def case(entry, key, scene, geom, dtype, C, K, table="row", opts=None, content="uniform", act=None, wipe=False,
         name=None):
    return dict(entry=entry, key=key, scene=scene, geom=geom, dtype=dtype, C=C, K=K, table=table, opts=opts or {},
                content=content, act=act, wipe=wipe, name=name)


def _n_dst(scene, geom, entry):
    """rows of the launch for the cases whose key depends on them (SubM scenes and dgrad: voxel counts)."""
    _, _, n, bs, _ = SCENES[scene]
    return n * bs


def _v4_cases():
    out = []
    red_for = {(1, 4): [3, 5, 8], (1, 2): [16, 12], (1, 1): [24, 32, 17], (2, 1): [40, 64, 96, 136],
               (2, 32): [8, 5], (2, 16): [16, 10], (2, 8): [24, 32]}
    width_for = {16: [16, 5], 32: [24, 32], 64: [64, 48, 40], 128: [96, 128], 256: [129, 200, 256]}
    mb1_sites = [("small", "subm3"), ("small", "s2"), ("mid", "k2s2"), ("n63", "subm3"), ("n65", "subm3"),
                 ("n1", "subm3"), ("small", "subm3d2"), ("mid", "k2s1"), ("n32768", "line"), ("mid", "lines2"),
                 ("small", "k1"), ("empty1", "s2")]
    mb2_sites = [("n32769", "line"), ("n33025", "line"), ("n40000", "lines2")]
    i = 0
    for dtype in (F16, BF16):
        for cout, mb in ((16, 1), (16, 2), (32, 1), (32, 2), (64, 1), (64, 2), (128, 1), (256, 1)):
            for bt in (False, True):
                for form in FORMS16:
                    i += 1
                    red = red_for[form][i % len(red_for[form])]
                    width = width_for[cout][i % len(width_for[cout])]
                    mode = 3 if form[1] in (32, 16, 8) else 1
                    if mb == 2:
                        sites = mb2_sites if bt else mb2_sites[:2]     # (a strided forward has fewer output rows)
                    else:
                        sites = mb1_sites
                    scene, geom = sites[i % len(sites)]
                    subm = GEOMS[geom][4]
                    tables = ["row", "sort", "layout"] if (mb == 2 and subm) else ["row", "sort"]
                    table = tables[(i // 3) % len(tables)]
                    C, K = (width, red) if bt else (red, width)
                    key = v4_key(dtype, padw(red, dtype), cout, _n_dst(scene, geom, "x"), bt, mode)
                    out.append(case("dgrad" if bt else "fwd", key, scene, geom, dtype, C, K, table,
                                    {"SPX_PK": mode} if mode != 1 else None))
    for cout in MFMA_COUT:
        for bt in (False, True):
            for nks in (1, 2):
                i += 1
                red = [4, 13, 16][i % 3] if nks == 1 else [20, 64, 36][i % 3]
                width = {16: 16, 32: 24, 64: 64, 128: 100, 256: 256}[cout]
                scene, geom = mb1_sites[i % len(mb1_sites)]
                C, K = (width, red) if bt else (red, width)
                key = v4_key(F32, padw(red, F32), cout, 0, bt)
                out.append(case("dgrad" if bt else "fwd", key, scene, geom, F32, C, K, ["row", "sort"][i % 2]))
    return out


def _bwd_cases():
    out = []
    sites = [("small", "subm3"), ("mid", "s2"), ("n65", "subm3"), ("mid", "k2s2"), ("small", "subm3d2"),
             ("n40000", "line"), ("n32769", "line")]
    i = 0
    for dtype in (F16, BF16):
        for C in (16, 32, 64, 128):
            for form, K, mode in (((2, 32), 8, 1), ((2, 16), 16, 1), ((2, 8), 24, 1), ((2, 8), 32, 1),
                                  ((2, 1), 48, 1), ((2, 1), 96, 1), ((1, 4), 8, 2), ((1, 2), 16, 2),
                                  ((1, 1), 24, 2), ((1, 1), 32, 0)):
                i += 1
                if form == (2, 8) and K == 32 and C in (16, 32):
                    continue                                 # (K = 24 covers the form there)
                if form == (2, 1) and K == 96 and C != 128:
                    continue
                scene, geom = sites[i % len(sites)]
                subm = GEOMS[geom][4]
                tl = ["row", "sort", "layout"] if subm and scene in ("n40000", "n32769") else ["row", "sort"]
                table = tl[i % len(tl)]
                out.append(case("bwd", bwd_key(dtype, C, K, mode), scene, geom, dtype, C, K, table,
                                {"SPX_PK": mode} if mode != 1 else None))
    for C in (16, 32, 64, 128):
        for K in (12, 40):
            i += 1
            scene, geom = sites[i % len(sites)]
            out.append(case("bwd", bwd_key(F32, C, K), scene, geom, F32, C, K, ["row", "sort"][i % 2]))
    return out


def _other_cases():
    out = []
    # weight-stationary kernel, 64 -> 64, with tails
    ws = {"SPX_WS": 1}
    out += [case("fwd", "igemm_ws/f16", "n65", "subm3", F16, 64, 64, opts=ws),
            case("dgrad", "igemm_ws/f16", "n32769", "line", F16, 64, 64, opts=ws),
            case("fwd", "igemm_ws/bf16", "n33025", "line", BF16, 64, 64, "layout", opts=ws),
            case("dgrad", "igemm_ws/bf16", "mid", "s2", BF16, 64, 64, opts=ws),
            case("fwd", "igemm_ws/bf16", "small", "subm3", BF16, 64, 64, "sort", opts=ws)]
    # rows walk of narrow layers
    for dtype in (F16, BF16):
        for C, K, scene, geom in ((16, 16, "small", "subm3"), (16, 32, "mid", "s2"), (32, 16, "n65", "subm3"),
                                  (32, 32, "mid", "k2s2")):
            out.append(case("bwd_rows", f"igemm_bwd_rows/{C}/{K}/{DTN[dtype]}/{1 if C == K == 16 else 0}", scene,
                            geom, dtype, C, K))
    # the weight gradient alone
    for dtype, C, K, scene, geom in ((F16, 16, 16, "small", "subm3"), (F16, 24, 32, "mid", "s2"),
                                     (F16, 64, 40, "small", "subm3d2"), (BF16, 5, 16, "n65", "subm3"),
                                     (BF16, 32, 24, "mid", "k2s2"), (BF16, 136, 64, "small", "subm3"),
                                     (F32, 16, 16, "mid", "s2"), (F32, 3, 24, "small", "subm3")):
        out.append(case("wgrad", wgrad_key(dtype, C, K), scene, geom, dtype, C, K))
    # the weight-gradient fallback kernels (odd widths through the C ABI: ops.igemm_wgrad pads to lane pieces)
    for dtype, C, K, scene, geom in ((F16, 5, 7, "small", "subm3"), (BF16, 3, 12, "mid", "s2"),
                                     (F32, 6, 5, "small", "subm3")):
        out.append(case("wgrad_capi", f"wgrad_generic/{DTN[dtype]}", scene, geom, dtype, C, K))
    # kernel volumes beyond 32: grouped launches (fp32 scratch), the generic kernel (> 128), wgrad in groups of 128
    for dtype, C, K, geom in ((F16, 32, 64, "k45"), (BF16, 64, 64, "k125"), (F32, 16, 24, "k125")):
        out.append(case("fwd", v4_key(dtype, padw(C, dtype), round_cout(K), 2500, False), "mid", geom, dtype, C, K))
        out.append(case("dgrad", v4_key(dtype, padw(K, dtype), round_cout(C), 2500, True), "mid", geom, dtype, C, K))
        out.append(case("bwd", v4_key(dtype, padw(K, dtype), round_cout(C), 2500, True), "mid", geom, dtype, C, K))
    out.append(case("fwd", "generic/f16", "mid", "k125", F16, 32, 32, "argsort"))   # mask-order rows: no fp32 scratch
    for dtype, C, K, geom in ((F16, 16, 16, "k216"), (BF16, 8, 16, "k343"), (F32, 5, 12, "k343")):
        out.append(case("fwd", f"generic/{DTN[dtype]}", "mid", geom, dtype, C, K))
        out.append(case("dgrad", f"generic/{DTN[dtype]}", "mid", geom, dtype, C, K))
        out.append(case("wgrad", wgrad_key(dtype, C, K), "mid", geom, dtype, C, K))
    # tile order with more tiles than resident workgroups (lpt): 625 tiles of 64 rows at COUT 128
    out.append(case("fwd", v4_key(F16, 64, 128, 40000, False), "n40000", "line", F16, 64, 128, "sort"))
    out.append(case("fwd", v4_key(BF16, 32, 128, 40000, False), "n40000", "line", BF16, 32, 128, "sort"))
    # wgrad chunk / group rules at their edges (the fp64 reference runs on the device)
    out.append(case("wgrad", "wgrad_tr/bf16/2", "big524k", "subm3", BF16, 16, 16))
    out.append(case("bwd", bwd_key(F16, 16, 16), "big524k", "subm3", F16, 16, 16, "layout"))
    out.append(case("bwd", bwd_key(F16, 32, 32), "n106k", "subm3", F16, 32, 32, "layout"))
    out.append(case("bwd", bwd_key(BF16, 64, 64), "n115k", "subm3", BF16, 64, 64, "layout"))
    out.append(case("wgrad", "wgrad_tr/f16/8", "n115k", "subm3", F16, 64, 32))
    # epilogue: bias + activation, COUT 256 and padded K included
    for dtype, C, K, act, scene, geom in ((F16, 64, 256, "relu", "small", "subm3"), (BF16, 32, 200, "leaky", "mid", "s2"),
                                          (F32, 16, 129, "sigmoid", "small", "subm3"), (F16, 24, 48, "sigmoid", "mid", "s2"),
                                          (BF16, 64, 64, "relu", "n32769", "line"), (F32, 40, 24, "leaky", "mid", "k2s2")):
        out.append(case("fwd", v4_key(dtype, padw(C, dtype), round_cout(K), _n_dst(scene, geom, "fwd"), False), scene,
                        geom, dtype, C, K, act=act, name=f"epilogue-{act}"))
    # content edges
    out.append(case("fwd", v4_key(F16, 32, 64, 0, False), "mid", "s2", F16, 32, 64, act="leaky", wipe=True,
                    name="no-neighbour-rows"))
    out.append(case("fwd", v4_key(BF16, 64, 256, 0, False), "mid", "s2", BF16, 64, 256, wipe=True,
                    name="no-neighbour-rows-nobias"))
    out.append(case("fwd", v4_key(BF16, 64, 64, 0, False), "mid", "subm3", BF16, 64, 64, content="big",
                    name="bf16-beyond-f16-range"))
    out.append(case("bwd", bwd_key(BF16, 64, 64), "mid", "subm3", BF16, 64, 64, content="big", name="bf16-beyond-f16-range"))
    for dtype, entry, C, K in ((F16, "fwd", 64, 64), (BF16, "dgrad", 32, 64), (F32, "fwd", 32, 32), (F16, "bwd", 32, 64),
                               (BF16, "wgrad", 64, 32)):
        key = {"fwd": v4_key(dtype, padw(C, dtype), round_cout(K), 0, False),
               "dgrad": v4_key(dtype, padw(K, dtype), round_cout(C), 0, True),
               "bwd": bwd_key(dtype, C, K), "wgrad": wgrad_key(dtype, C, K)}[entry]
        out.append(case(entry, key, "mid", "s2", dtype, C, K, content="scales", name="channel-scales"))
    out.append(case("bwd", bwd_key(F16, 32, 32), "empty1", "s2", F16, 32, 32, name="empty-scene-in-batch"))
    out.append(case("fwd", v4_key(BF16, 16, 32, 0, False), "empty1", "k2s2", BF16, 16, 32, "sort",
                    name="empty-scene-in-batch"))
    # the backward of a module inside deferred_wgrad() under a real backward call
    out.append(case("bwd_deferred", bwd_key(F16, 64, 64), "small", "subm3", F16, 64, 64, name="deferred"))
    out.append(case("bwd_deferred", bwd_key(BF16, 32, 64), "mid", "subm3", BF16, 32, 64, name="deferred"))
    return out


CASES = _v4_cases() + _bwd_cases() + _other_cases()


def _case_id(c):
    """the instance key (dots for slashes) and the case: `pytest --collect-only` lists which case reaches which key"""
    return c["key"].replace("/", ".") + "-" + _seed_id(c)


def _seed_id(c):
    return (f"{c['name'] + '-' if c['name'] else ''}{c['entry']}-{DTN[c['dtype']]}-C{c['C']}-K{c['K']}-{c['scene']}-"
            f"{c['geom']}-{c['table']}")


# ---------------------------------------------------------------- running a case
def _rounded(t, dtype):
    return t.to(dtype).to(torch.float64)


def _operands(c, n_in, n_out, ks, dev):
    """fp64 tensors holding values representable in the case's dtype."""
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(_seed_id(c).encode()))
    C, K, dtype = c["C"], c["K"], c["dtype"]
    kv = int(np.prod(ks))
    f = torch.rand((n_in, C), generator=g, dtype=torch.float64) * 2 - 1
    w = torch.rand((K, kv, C), generator=g, dtype=torch.float64) * 2 - 1
    d = (torch.rand((n_out, K), generator=g, dtype=torch.float64) * 2 - 1) * 0.2
    if c["content"] == "big":          # partial sums far beyond the fp16 range (~1e5 .. 1e6), all of one sign
        f = 16 + 16 * torch.rand((n_in, C), generator=g, dtype=torch.float64)
        w = 16 + 16 * torch.rand((K, kv, C), generator=g, dtype=torch.float64)
        d = 4 + 4 * torch.rand((n_out, K), generator=g, dtype=torch.float64)
    elif c["content"] == "scales":     # per-channel scales over 2^-8 .. 2^8: a swapped channel or offset shows
        ec = torch.randint(-8, 9, (C,), generator=g).to(torch.float64)
        ek = torch.randint(-2, 3, (K,), generator=g).to(torch.float64)
        eo = torch.randint(-6, 7, (kv,), generator=g).to(torch.float64)
        f = f * torch.exp2(ec)
        w = w * torch.exp2(-ec)[None, None, :] * torch.exp2(ek)[:, None, None] * torch.exp2(eo)[None, :, None]
        d = d * torch.exp2(-ek)
    bias = (torch.rand((K,), generator=g, dtype=torch.float64) * 2 - 1) if c["act"] else None
    f, w, d = _rounded(f, dtype), _rounded(w, dtype).reshape(K, *ks, C), _rounded(d, dtype)
    if bias is not None:
        bias = _rounded(bias, dtype)
    return f.to(dev), w.to(dev), d.to(dev), (None if bias is None else bias.to(dev))


def _act(x, act):
    if act == "relu":
        return torch.relu(x)
    if act == "leaky":
        return torch.where(x >= 0, x, x * 0.1)
    if act == "sigmoid":
        return torch.sigmoid(x)
    return x


def _check(got, want, A, dtype, name, shape=None):
    assert got.is_contiguous(), f"{name}: not contiguous"
    if shape is not None:
        assert tuple(got.shape) == tuple(shape), (name, tuple(got.shape), shape)
    c = 1e-5 if dtype == F32 else 1e-6
    a, r, A = got.double().cpu().numpy(), want.cpu().numpy(), A.cpu().numpy()
    if dtype == F16:
        # below 2^-14 fp16 is subnormal: the one output rounding errs by up to half the fixed spacing 2^-24 there, which
        # u |ref| does not express (the channel-scale cases put cancelling sums there); the same c holds on top of it
        tiny = np.abs(r) < 2.0 ** -14
        bad = tiny & (np.abs(a - r) > 2.0 ** -25 + c * A)
        assert not bad.any(), f"{name}: {int(bad.sum())} subnormal-range elements outside 2^-25 + {c:g} A"
        a = np.where(tiny, r, a)
    assert_close_abs_sum(a, r, A, dtype, c, name=name)


def _tables(c, rb, which, width):
    from spconv_amd.pytorch import ops
    if c["table"] == "row":
        pair, mask = (rb.pair_fwd, rb.mask_fwd) if which == "fwd" else (rb.pair_bwd, rb.mask_bwd)
        return pair, mask, None, 0
    if c["table"] == "argsort":        # rows listed in mask order (first mask word) over row-order tables
        pair, mask = (rb.pair_fwd, rb.mask_fwd) if which == "fwd" else (rb.pair_bwd, rb.mask_bwd)
        return pair, mask, ops.mask_argsort(mask[:, :1].contiguous()), 0
    return ops.tables_of(rb, which, width)


def _run(c, dev):
    from spconv_amd import _lib
    from spconv_amd.pytorch import ops
    import spconv_amd.pytorch as spconv
    L = _lib.load()
    idx, shape, bs = scene_indices(c["scene"])
    ks, st, pd, dl, subm = GEOMS[c["geom"]]
    kv = int(np.prod(ks))
    dtype, C, K = c["dtype"], c["C"], c["K"]
    rb = rulebook(c["scene"], c["geom"], "row" if c["table"] == "argsort" else c["table"])
    out_idx, cand = ref_pairs(c["scene"], c["geom"], dev)
    n_in, n_out = idx.shape[0], out_idx.shape[0]
    assert rb.n_out == n_out and rb.n_in == n_in
    out_shape = out_spatial_shape(shape, ks, st, pd, dl, subm)
    perm = torch.from_numpy(match_rows(rb.out_indices.cpu().numpy(), out_idx.cpu().numpy(), out_shape)).to(dev)
    f, w, d_gpu_order, bias = _operands(c, n_in, n_out, ks, dev)
    d = torch.empty_like(d_gpu_order)
    d[perm] = d_gpu_order                           # dout in the reference's row order
    if c["wipe"]:                                   # output rows whose every neighbour is gone
        dead = torch.arange(3, n_out, max(7, n_out // 40), device=dev)
        pair = rb.pair_fwd.clone()
        mask = rb.mask_fwd.clone()
        pair[:, dead] = -1
        mask[dead] = 0
        gone = perm[dead]
        cand = [(k, i[~torch.isin(o, gone)], o[~torch.isin(o, gone)]) for k, i, o in cand]
    ref = conv_from_pairs(out_idx, cand, f, w, d)
    fg, wg, dg = f.to(dtype), w.to(dtype), d_gpu_order.to(dtype)
    key = c["key"].encode()
    before = L.spx_launch_count(key)
    assert before >= 0, f"unknown instance key {c['key']}"
    restore = {}
    try:
        for name, v in c["opts"].items():
            restore[name] = {"SPX_PK": 1, "SPX_WS": -1}[name]
            L.spx_set_option(name.encode(), v)
        got = {}
        if c["entry"] == "fwd":
            if c["wipe"]:
                tabs = (pair, mask, None, 0)
            else:
                tabs = _tables(c, rb, "fwd", K)
            act = {None: ops.Activation.None_, "relu": ops.Activation.ReLU, "leaky": ops.Activation.LeakyReLU,
                   "sigmoid": ops.Activation.Sigmoid}[c["act"]]
            got["out"] = ops.igemm_fwd(fg, wg, tabs[0], tabs[1], tabs[2], rb.n_out, kv // 2 if subm else -1,
                                       bias=None if bias is None else bias.to(dtype), act_type=act, act_alpha=0.1,
                                       tile_order=tabs[3])
        elif c["entry"] == "dgrad":
            tabs = _tables(c, rb, "fwd" if subm else "bwd", C)
            got["din"] = ops.igemm_dgrad(dg, wg, tabs[0], tabs[1], tabs[2], rb.n_in, subm, tile_order=tabs[3])
        elif c["entry"] == "wgrad":
            got["dW"] = ops.igemm_wgrad(fg, dg, wg.shape, rb.pair_native, rb.num_per_loc, subm, ops._plan_of(rb))
        elif c["entry"] == "wgrad_capi":
            dw = torch.empty_like(wg)
            ws = torch.empty((L.spx_igemm_wgrad_ws_bytes(n_in, C, K, kv),), dtype=torch.uint8, device=dev)
            _lib.check(L.spx_igemm_wgrad(fg.data_ptr(), dg.data_ptr(), dw.data_ptr(), rb.pair_native.data_ptr(),
                                         rb.num_per_loc.data_ptr(), None, n_in, n_out, C, K, kv, ops._dtype_code(fg),
                                         int(subm), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
            got["dW"] = dw
        elif c["entry"] in ("bwd", "bwd_rows"):
            tabs = _tables(c, rb, "fwd" if subm else "bwd", C)
            got["din"], got["dW"] = ops.igemm_bwd(fg, dg, wg, tabs[0], tabs[1], tabs[2], rb.pair_native,
                                                  rb.num_per_loc, subm, ops._plan_of(rb), tile_order=tabs[3],
                                                  dense_rows=c["entry"] == "bwd_rows")
        elif c["entry"] == "bwd_deferred":
            net = spconv.SubMConv3d(C, K, ks, bias=False, indice_key="m").to(dev, dtype)
            with torch.no_grad():
                net.weight.copy_(wg)
            feats = fg.clone().requires_grad_(True)
            x = spconv.SparseConvTensor(feats, torch.from_numpy(idx).to(dev), shape, bs)
            with ops.deferred_wgrad():
                y = net(x)
                y.features.backward(dg)
            got["out"], got["din"], got["dW"] = y.features.detach(), feats.grad, net.weight.grad
        torch.cuda.synchronize()
    finally:
        for name, v in restore.items():
            L.spx_set_option(name.encode(), v)
    after = L.spx_launch_count(key)
    assert after > before, f"{c['key']} was not launched (counter {before} -> {after})"
    if "out" in got:
        want, A = ref.out, ref.out_abs
        if bias is not None:
            want, A = want + bias, A + bias.abs()
        want = _act(want, c["act"])
        _check(got["out"], want[perm], A[perm], dtype, "out", (n_out, K))
        if c["wipe"]:
            # rows with no neighbour: exactly act(bias) in the output dtype (zeros without a bias)
            rows = got["out"][dead].float()
            b32 = torch.zeros((K,), device=dev) if bias is None else bias.float()
            exp = _act(b32, c["act"]).to(dtype).float().expand_as(rows)
            assert torch.equal(rows, exp), "rows without neighbours differ from act(bias)"
    if "din" in got:
        _check(got["din"], ref.din, ref.din_abs, dtype, "din", (n_in, C))
    if "dW" in got:
        _check(got["dW"], ref.dW, ref.dW_abs, dtype, "dW", tuple(w.shape))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[_case_id(c) for c in CASES])
def test_instance_against_fp64(cuda, c):
    _run(c, cuda)


# ---------------------------------------------------------------- CPU: the table, the key grammar and the checker
def test_cases_cover_every_reachable_instance():
    reach = reachable()
    claimed = {c["key"] for c in CASES}
    assert claimed <= reach, sorted(claimed - reach)
    excluded = set()
    for pat, why in EXCLUDED:
        hit = {k for k in reach if fnmatch.fnmatchcase(k, pat)}
        assert hit, f"exclusion {pat!r} matches no reachable instance"
        assert not (hit & claimed), f"{pat!r} excludes instances a case claims: {sorted(hit & claimed)}"
        excluded |= hit
    missing = reach - claimed - excluded
    assert not missing, f"instances with neither a case nor a reason: {sorted(missing)}"


def test_instance_keys_parse():
    """spx_launch_count knows every reachable key and rejects malformed ones (host only: nothing launches)."""
    from spconv_amd import _lib
    L = _lib.load()
    for k in sorted(reachable()):
        assert L.spx_launch_count(k.encode()) >= 0, k
    for fam in ("igemm_v4", "igemm_ws", "igemm_bwd", "igemm_bwd_rows", "generic"):
        assert L.spx_launch_count(fam.encode()) >= 0, fam
    for bad in ("igemm_v4/48/1/f16/fwd/2/1", "igemm_v4/64/3/f16/fwd/2/1", "igemm_v4/64/1/f64/fwd/2/1",
                "igemm_v4/64/1/f16/fwd/2", "igemm_v4/64/1/f16/up/2/1", "igemm_v4/64/1/f16/fwd/2/3",
                "igemm_bwd/64/2/f16/2/1/0", "igemm_ws/", "wgrad_tr/f16/6", "wgrad_f32/f32",
                "gen1/64", "igemm_bwd_rows/64/16/f16/0", "no_such_family", "", "/", "igemm_v4//1/f16/fwd/2/1"):
        assert L.spx_launch_count(bad.encode()) == -1, bad


def _checker_case(dtype):
    rng = np.random.default_rng(7)
    from util import scene
    shape = [12, 12, 12]
    idx = scene(shape, 600, 1, 3)
    C, K = 16, 16
    f = _rounded(torch.from_numpy(rng.uniform(-1, 1, (idx.shape[0], C))), dtype)
    w = _rounded(torch.from_numpy(rng.uniform(-1, 1, (K, 3, 3, 3, C))), dtype)
    out_idx, cand = pairs(idx, 1, shape, [3] * 3, [1] * 3, [1] * 3, [1] * 3, True)
    return out_idx, cand, f, w


@pytest.mark.parametrize("dtype", [F16, BF16, F32])
def test_checker_rejects_a_missing_pair(dtype):
    out_idx, cand, f, w = _checker_case(dtype)
    ref = conv_from_pairs(out_idx, cand, f, w, None)
    c = 1e-5 if dtype == F32 else 1e-6
    good = ref.out.to(dtype).double().numpy()
    assert_close_abs_sum(good, ref.out.numpy(), ref.out_abs.numpy(), dtype, c)
    # drop one pair of a non-centre offset
    k, i, o = next(t for t in cand if t[0] != 13 and t[1].numel() > 0)
    cut = [(kk, ii[1:], oo[1:]) if kk == k else (kk, ii, oo) for kk, ii, oo in cand]
    bad = conv_from_pairs(out_idx, cut, f, w, None).out.to(dtype).double().numpy()
    with pytest.raises(AssertionError):
        assert_close_abs_sum(bad, ref.out.numpy(), ref.out_abs.numpy(), dtype, c)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_checker_rejects_four_ulp(dtype):
    out_idx, cand, f, w = _checker_case(dtype)
    ref = conv_from_pairs(out_idx, cand, f, w, None)
    got = ref.out.to(dtype).double()
    # the element whose value is largest against its magnitude sum, moved by 4 ulp of the output dtype
    i = int(torch.argmax(ref.out.abs() / ref.out_abs).item())
    r, col = divmod(i, got.shape[1])
    v = float(got[r, col])
    ulp = 2 * HALF_ULP[str(dtype).replace("torch.", "")] * 2.0 ** np.floor(np.log2(abs(v)))
    moved = v - 4 * ulp * np.sign(v)                                   # (towards zero: stays representable)
    got[r, col] = moved
    assert float(got[r, col].to(dtype).double()) == moved
    c = 1e-6
    with pytest.raises(AssertionError):
        assert_close_abs_sum(got.numpy(), ref.out.numpy(), ref.out_abs.numpy(), dtype, c)
