"""The whole launch-counter table, checked on the host: tests/counters_main.cpp links csrc/counters.cpp and
csrc/common.cpp as plain C++ (no GPU is opened) and answers two questions.  Which keys does spx_launch_count accept --
exactly the inventory the comment above it in include/spconv_amd.h spells out, out of a candidate set with every field
of the grammar widened beyond its legal values?  And is key -> storage slot a bijection: every slot moves at most one
key, a declared slot the key it is declared with, every key is moved by exactly one slot, and the only slots without
a key are the igemm_v4w instances that are never built?  No GPU test can see a name that drifted from its enumerator or
two keys that share a slot: `after > before` holds for the neighbour as well."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spconv_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# ---- the inventory, from the header's grammar ----------------------------------------------------------------------
FAMILIES = ["igemm_v4", "igemm_ws", "igemm_bwd", "igemm_bwd_rows", "igemm_i8_stream", "generic", "wgrad_stage2",
            "wgrad_stage2_batch", "igemm_f64", "igemm_v4w"]
F64 = ["igemm_f64/fwd", "igemm_f64/dgrad", "wgrad_f64", "pool/f64"]
FLAT = {
    "sparse_hint": ["v4", "bwd"],
    "dense": ["map", "scatter_cl", "scatter_cf", "gather_cl", "gather_cf", "compact"],
    "union": ["mark", "prefix", "claim", "fill", "add_fwd", "add_bwd"],
    "collapse": ["mark", "prefix", "rank", "list", "fwd", "bwd"],
    "pointvoxel": ["groups", "gather", "decorate"],
    "interp": ["corners_ranked", "corners_hash", "fwd", "bwd"],
    "query": ["ranked", "hash", "group_fwd", "group_bwd"],
    "sample": ["fps", "ball_query", "knn_query"],
    "box": ["corners", "pairs", "aligned", "key", "mask", "reduce"],
    "serialize": ["keys", "sort", "offsets", "plan", "bwd"],
    "select": ["score", "hist", "pick", "ties", "flags", "count", "scan", "scatter", "map"],
    "rulebook": ["subm_probe3", "subm_probe4", "subm_probe5", "subm_mask_pass", "subm_lists", "native_lists_v1",
                 "conv3/1", "conv3/2", "conv3/4", "conv3/8", "conv_generic", "conv_lists_v1", "conv_shrunk",
                 "conv_retry", "conv3_shares/1", "conv3_shares/2", "conv3_shares/4", "conv3_shares/8"],
}
NAMED = FAMILIES + F64 + [f"{fam}/{leaf}" for fam, leaves in FLAT.items() for leaf in leaves]

COUTS, MBS, DTS, DIRS, NKSS, PKS = [16, 32, 64, 128, 256], [1, 2], ["f16", "bf16", "i8", "f32"], ["fwd", "bt"], [1, 2], \
    [1, 2, 4, 8, 16, 32]
POOL_OPS, POOL_DTS, PIECES = ["max_fwd", "max_bwd", "avg_fwd", "avg_bwd"], ["f16", "bf16", "f32", "f64", "i8"], ["v", "s"]


def v4w_exists(dt, d, nks, pk):
    """PK in {1, 2, 4}, PK > 1 with NKS 1 and a 16-bit dt; i8: fwd."""
    return pk in (1, 2, 4) and (pk == 1 or (nks == 1 and dt in ("f16", "bf16"))) and not (dt == "i8" and d == "bt")


def keys(fmt, *fields):
    return [fmt.format(*v) for v in itertools.product(*fields)]


def instance_keys(couts, mbs, dts, dirs, nkss, pks, nts, cks, w8s, sls, exists):
    """{family: keys} of the per-instance grammar over the given field values."""
    return {
        "v4": keys("igemm_v4/{}/{}/{}/{}/{}/{}", couts, mbs, dts, dirs, nkss, pks),
        "v4w": [k for k, v in zip(keys("igemm_v4w/{}/{}/{}/{}/{}", nts, dts, dirs, nkss, pks),
                                  itertools.product(nts, dts, dirs, nkss, pks)) if exists(*v[1:])],
        "bwd": keys("igemm_bwd/{}/{}/{}/{}/{}", couts, mbs, dts, nkss, pks),
        "ws": keys("igemm_ws/{}", dts),
        "bwd_rows": keys("igemm_bwd_rows/{}/{}/{}/{}", cks, cks, dts, w8s),
        "wgrad_tr": keys("wgrad_tr/{}/{}", dts, sls),
        "wgrad_f32": ["wgrad_f32"],
        "wgrad_mfma": keys("wgrad_mfma/{}", dts),
        "wgrad_generic": keys("wgrad_generic/{}", dts),
        "generic": keys("generic/{}", dts),
        "gen1": keys("gen1/{}/{}", couts, dts),
    }


INSTANCES = instance_keys(COUTS, MBS, DTS, DIRS, NKSS, PKS, [128], [16, 32], [0, 1], [2, 4, 8], v4w_exists)
POOL = keys("pool/{}/{}/{}", POOL_OPS, POOL_DTS, PIECES)
INVENTORY = NAMED + [k for fam in INSTANCES.values() for k in fam] + POOL


def candidates():
    """The inventory's grammar with every field widened beyond its legal set, and the flat names crossed."""
    wide_dts = DTS + ["f64", "f8"]
    wide = instance_keys([8, 16, 32, 48, 64, 128, 256, 384, 512], [0, 1, 2, 3], wide_dts, DIRS + ["up"], [0, 1, 2, 3],
                         [0, 1, 2, 3, 4, 8, 16, 32, 64], [64, 128, 256], [8, 16, 32, 64], [0, 1, 2], [1, 2, 4, 8, 16],
                         lambda *v: True)
    out = [k for fam in wide.values() for k in fam]
    out += keys("pool/{}/{}/{}", POOL_OPS + ["sum_fwd"], wide_dts, PIECES + ["x"])
    leaves = sorted({leaf for ls in FLAT.values() for leaf in ls})
    out += keys("{}/{}", list(FLAT), leaves)
    out += list(FLAT) + [fam + "/" for fam in FLAT] + [fam + "/" for fam in FAMILIES]
    out += ["rulebook/conv3/16", "rulebook/conv3_shares/3", "conv3/1", "subm_probe3", "pool", "pool/", "wgrad_f32/",
            "igemm_v4/", "", "/"]
    return sorted(set(out) | set(INVENTORY))


def test_inventory_is_the_headers():
    assert len(NAMED) == 86 and len(POOL) == 40
    assert {fam: len(ks) for fam, ks in INSTANCES.items()} == {
        "v4": 960, "v4w": 22, "bwd": 480, "ws": 4, "bwd_rows": 32, "wgrad_tr": 12, "wgrad_f32": 1, "wgrad_mfma": 4,
        "wgrad_generic": 4, "generic": 4, "gen1": 20}
    assert len(INVENTORY) == len(set(INVENTORY)) == 86 + 40 + 1543 == 1669


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    """tests/counters_main.cpp + counters.cpp + common.cpp as host C++: no offload, no HIP runtime linked."""
    exe = str(tmp_path_factory.mktemp("counters") / "counters_main")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "include")
    subprocess.run([HIPCC, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-std=c++17", "-O1", "-Wall", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), "-I", rocm_include, os.path.join(ROOT, "tests", "counters_main.cpp"),
                    os.path.join(CSRC, "counters.cpp"), os.path.join(CSRC, "common.cpp"), "-o", exe], check=True)
    return exe


def run(prog, mode, lines):
    r = subprocess.run([prog, mode], input="".join(k + "\n" for k in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_accepted_keys_are_the_inventory(prog):
    cand = candidates()
    accepted = set(run(prog, "--classify", cand))
    inventory = set(INVENTORY)
    print(f"{len(cand)} candidates: {len(accepted)} accepted, {len(cand) - len(accepted)} rejected")
    assert len(cand) > 30000 and inventory <= set(cand)
    assert sorted(accepted - inventory) == [], "accepted outside the header's grammar"
    assert sorted(inventory - accepted) == [], "keys of the header's grammar that are refused"
    assert len(accepted) == 1669


def test_key_to_slot_is_a_bijection(prog):
    (line,) = run(prog, "--bijection", INVENTORY)    # its own asserts: one key per slot, a declared slot its own name,
    words = line.split()                             # every key moved by exactly one slot
    got = dict(zip(words[::2], map(int, words[1::2])))
    print(line)
    assert got["keys"] == len(INVENTORY) and got["named"] == len(NAMED)
    assert got["dead"] == got["slots"] - len(INVENTORY) == 26 and got["dead_outside_v4w"] == 0
    assert got["slots"] == 1695
