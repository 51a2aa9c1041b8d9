"""float64 plumbing that needs no GPU: the ABI constant, the dtype tables, the counter keys, the workspace query and the
entries that refuse float64 (they return before anything is enqueued)."""
import ctypes
import os
import re
import subprocess

import torch

from spconv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dtype_constant_matches_header():
    with open(os.path.join(ROOT, "include", "spconv_amd.h")) as fh:
        enum = re.search(r"enum spx_dtype \{([^}]*)\}", fh.read()).group(1)
    assert "SPX_F64 = 4" in enum
    assert _lib.DTYPE_F64 == 4


def test_python_dtype_tables_take_float64():
    from spconv_amd.pytorch import ops
    assert ops._DTYPES[torch.float64] == _lib.DTYPE_F64
    assert ops._POOL_CODES[torch.float64] == _lib.DTYPE_F64
    assert ops._dtype_code(torch.zeros(1, dtype=torch.float64)) == _lib.DTYPE_F64


def test_float64_counter_keys_parse():
    L = _lib.load()
    for k in ("igemm_f64", "igemm_f64/fwd", "igemm_f64/dgrad", "wgrad_f64", "pool/f64"):
        assert L.spx_launch_count(k.encode()) >= 0, k
    # the template instances keep their dt vocabulary {f16, bf16, i8, f32}
    for bad in ("igemm_v4/64/1/f64/fwd/2/1", "igemm_bwd/64/2/f64/1/1", "igemm_ws/f64", "generic/f64",
                "igemm_f64/bt", "igemm_f64/", "pool/f32", "wgrad_f64/f64"):
        assert L.spx_launch_count(bad.encode()) == -1, bad


def test_wgrad_workspace_query_by_dtype():
    L = _lib.load()
    for n, C, K, kv in ((1, 3, 5, 27), (1000, 16, 300, 27), (100000, 64, 64, 27), (5000, 8, 8, 216)):
        for dt in (_lib.DTYPE_F32, _lib.DTYPE_F16, _lib.DTYPE_BF16):
            assert L.spx_igemm_wgrad_ws_bytes_dtype(n, C, K, kv, dt) == L.spx_igemm_wgrad_ws_bytes(n, C, K, kv)
        b = L.spx_igemm_wgrad_ws_bytes_dtype(n, C, K, kv, _lib.DTYPE_F64)
        tiles = -(-C // 64) * -(-K // 64)
        assert b >= kv * tiles * 64 * 64 * 8 and b % 256 == 0


def test_deferred_and_rows_entries_refuse_float64():
    L = _lib.load()
    job = ctypes.create_string_buffer(64)
    rc = L.spx_igemm_bwd_deferred(None, None, None, None, None, None, None, None, 0, None, None, None,
                                  10, 10, 8, 8, 27, _lib.DTYPE_F64, 1, None, 0, None, job)
    assert rc != 0 and b"float64" in L.spx_last_error()
    rc = L.spx_igemm_wgrad_deferred(None, None, None, None, None, None, 10, 10, 8, 8, 27, _lib.DTYPE_F64, 1,
                                    None, 0, None, job)
    assert rc != 0 and b"float64" in L.spx_last_error()
    rc = L.spx_igemm_bwd_rows(None, None, None, None, None, None, None, 10, 10, 16, 16, 27, 1, _lib.DTYPE_F64,
                              None, 0, None)
    assert rc != 0


def test_empty_float64_pooling_counts_no_launch():
    """pool/f64 counts launches that happen: an empty output enqueues nothing and leaves the counter alone."""
    L = _lib.load()
    before = L.spx_launch_count(b"pool/f64")
    one = ctypes.c_void_p(16)            # never dereferenced: nothing is launched for zero rows
    assert L.spx_maxpool_fwd(one, one, one, None, 0, 8, 27, _lib.DTYPE_F64, 0, None) == 0
    assert L.spx_avgpool_fwd(one, one, None, one, None, 0, 8, 27, _lib.DTYPE_F64, None) == 0
    assert L.spx_launch_count(b"pool/f64") == before


def test_every_build_script_links_every_unit():
    """The timeline (build_debug.sh) and ablation (build_ablate.sh) libraries link every translation unit of the
    product build (csrc/build.sh --list): a unit missing there leaves symbols undefined, and the library then fails to
    load although its link succeeded.  Both scripts take their objects from that list; `--list` prints what they link."""
    csrc = os.path.join(ROOT, "spconv_amd", "csrc")
    units = [os.path.splitext(os.path.basename(o))[0] for o in _lib.linked_objects()]
    assert len(units) > 20 and "igemm" in units and "common" in units
    for script, arg, fmt in (("build_debug.sh", [], "../lib/dbg/{}.o"), ("build_ablate.sh", ["3"], "../lib/{}.o")):
        out = subprocess.check_output(["bash", os.path.join(csrc, script), "--list"] + arg, text=True).split()
        want = ["../lib/abl/igemm3.o" if (script == "build_ablate.sh" and u == "igemm") else fmt.format(u) for u in units]
        assert out == want, script
        with open(os.path.join(csrc, script)) as fh:
            link = [ln for ln in fh if "-shared" in ln]
        assert len(link) == 1, script       # one link line, and it links that list
        assert ("$OBJS" if script == "build_debug.sh" else "$(objs $v)") in link[0], script
