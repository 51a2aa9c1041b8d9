"""The gather-GEMM, dgrad and wgrad kernels on the inputs the kernel matrix does not use: dirty memory on entry, rows that
no pair names, and NaN / Inf in rows that pairs do name (include/spconv_amd.h, "What the gather-GEMM entries may be handed").

Scenes, geometries, rulebook and reference caches, operands, checker and the instance-key model are those of
test_gpu_kernel_matrix.py; the cases here reach every kernel FAMILY once per dtype (test_cases_claim_every_family), on the
smallest scenes, and each asserts through spx_launch_count that its key moved.  Three groups:

  dirty    the C entries with caller-owned buffers: every output, workspace byte and statistics record starts as 0x00 in one
           run and as 0xFF (NaN in every float type, -1 = "absent" in every index) in the other; the two runs agree bit for
           bit and the second one meets the fp64 reference.
  unnamed  every pair that names a chosen 5 % of the rows is removed from the tables and lists; those rows hold zeros in one
           run and NaN (or +Inf) in the other: no output bit changes, and the zero run meets the reference of the edited
           tables.  An entry that is told of an identity offset (identity_k >= 0, subm = 1) names every row through it, so
           the forward runs with identity_k = -1 and the centre pair in its table, the backward entries on strided
           geometries; the rows walk reads its whole table and takes SubM as it is.
  named    NaN, +Inf and -Inf in a few channels of rows that pairs name (chosen so that some output receives +Inf and -Inf
           together: tests/nonfinite.py, held to its conditions by test_refconv.py): out and din are NaN / +Inf / -Inf
           exactly where the reference is, dW swallows nothing and is non-finite only in a poisoned channel or column; the
           finite elements meet the matrix's bound.  Bias + ReLU / LeakyReLU / sigmoid epilogues, spx_bias_act_inplace and
           the fused BatchNorm + ReLU apply follow torch's semantics (relu(NaN) = NaN)."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import test_gpu_kernel_matrix as M
from nonfinite import masks_of, poison_rows, poisoned, unnamed_rows
from refconv import conv_from_pairs, out_spatial_shape
from util import match_rows

F16, BF16, F32, F64 = M.F16, M.BF16, M.F32, torch.float64
M.DTN.setdefault(F64, "f64")            # (the matrix names its operands' seeds by dtype; float64 has cases only here)
DTN = M.DTN


def _act_code(act):
    from spconv_amd.pytorch import ops
    return {None: ops.Activation.None_, "relu": ops.Activation.ReLU, "leaky": ops.Activation.LeakyReLU,
            "sigmoid": ops.Activation.Sigmoid}[act]


# ---------------------------------------------------------------- the case table
def _families(c):
    """the families of the issue's list that a case reaches, read off its instance key"""
    key, dt = c["key"], DTN.get(c["dtype"], "i8")
    p = key.split("/")
    if p[0] == "igemm_v4" and p[3] == "i8":
        return {"int8-fwd"}
    if p[0] == "igemm_v4":
        if p[4] == "bt":
            return {f"v4-bt/{dt}"}
        fam = {f"v4-fwd-nks{p[5]}/{dt}"}
        if c["geom"] in ("k45", "k125"):
            fam.add(f"grouped-{c['geom']}/{dt}")
        if p[2] == "1":
            fam.add(f"v4-fwd-mb1/{dt}")
        elif c["scene"] == "n32769":
            fam.add(f"v4-fwd-mb2-n32769/{dt}")
        return fam
    if p[0] == "igemm_v4w":
        return {"wide"}
    if p[0] == "igemm_bwd_rows":
        return {f"bwd_rows-{'16x16' if p[1] == p[2] == '16' else 'other'}/{dt}"}
    if p[0] == "wgrad_tr":
        return {f"wgrad_tr-sl{p[2]}/{dt}"}
    if p[0] in ("igemm_bwd", "igemm_ws", "wgrad_generic", "generic"):
        return {f"{p[0]}/{dt}"}
    return {key}                         # wgrad_f32, igemm_f64/fwd, igemm_f64/dgrad, wgrad_f64


def required_families():
    req = {"wgrad_f32", "igemm_f64/fwd", "igemm_f64/dgrad", "wgrad_f64", "wide", "int8-fwd"}
    for dt in ("f16", "bf16", "f32"):
        req |= {f"{f}/{dt}" for f in ("v4-fwd-mb1", "v4-fwd-mb2-n32769", "v4-fwd-nks1", "v4-fwd-nks2", "v4-bt",
                                      "grouped-k45", "grouped-k125", "igemm_bwd", "wgrad_generic", "generic")}
    for dt in ("f16", "bf16"):
        req |= {f"{f}/{dt}" for f in ("igemm_ws", "bwd_rows-16x16", "bwd_rows-other", "wgrad_tr-sl2", "wgrad_tr-sl4",
                                      "wgrad_tr-sl8")}
    return req


def _cases():
    case, v4, pw, rc = M.case, M.v4_key, M.padw, M.round_cout
    out = []

    def fwd(dtype, scene, geom, C, K, n_dst=0, **kw):
        out.append(case(kw.pop("entry", "fwd"), v4(dtype, pw(C, dtype), rc(K), n_dst, False), scene, geom, dtype, C, K, **kw))

    def dgrad(dtype, scene, geom, C, K, **kw):
        out.append(case("dgrad", v4(dtype, pw(K, dtype), rc(C), 0, True), scene, geom, dtype, C, K, **kw))

    # igemm_v4 forward: MB 1 with NKS 1 and 2, MB 2 on n32769 (fp32: MB 1 at 256 columns only)
    fwd(F16, "small", "subm3", 32, 64)
    fwd(F16, "mid", "s2", 64, 128)
    fwd(F16, "n32769", "line", 32, 64, 32769)
    fwd(BF16, "n65", "subm3", 24, 32)
    fwd(BF16, "small", "s2", 40, 64)
    fwd(BF16, "n32769", "line", 16, 32, 32769)
    fwd(F32, "small", "subm3", 16, 256)
    fwd(F32, "mid", "s2", 40, 256)
    fwd(F32, "n32769", "line", 8, 16)
    fwd(F32, "mid", "k2s2", 20, 32)
    fwd(F16, "small", "subm3", 32, 64, entry="fwd_stats", name="stats")
    # bt
    dgrad(F16, "small", "s2", 64, 32)
    dgrad(BF16, "mid", "k2s2", 32, 64)
    dgrad(F32, "mid", "s2", 32, 16)
    # grouped kernel volumes (fp32 partial sums through a scratch)
    for dtype, C, K in ((F16, 32, 64), (BF16, 64, 64), (F32, 16, 32)):
        for geom in ("k45", "k125"):
            fwd(dtype, "mid", geom, C, K, 2500)
    # fused backward, its deferred form, weight-stationary kernel, rows walk
    out.append(case("bwd", M.bwd_key(F16, 64, 32), "mid", "s2", F16, 64, 32))
    out.append(case("bwd", M.bwd_key(BF16, 32, 64), "mid", "k2s2", BF16, 32, 64))
    out.append(case("bwd", M.bwd_key(F32, 16, 12), "mid", "s2", F32, 16, 12))
    out.append(case("bwd_deferred", M.bwd_key(F16, 64, 64), "small", "subm3", F16, 64, 64, name="deferred"))
    ws = {"SPX_WS": 1}
    out.append(case("fwd", "igemm_ws/f16", "n65", "subm3", F16, 64, 64, opts=ws))
    out.append(case("dgrad", "igemm_ws/bf16", "mid", "s2", BF16, 64, 64, opts=ws))
    out.append(case("fwd", "igemm_ws/bf16", "small", "subm3", BF16, 64, 64, opts=ws))
    out.append(case("dgrad", "igemm_ws/f16", "small", "s2", F16, 64, 64, opts=ws))
    for dtype, C, K, scene, geom in ((F16, 16, 16, "small", "subm3"), (BF16, 16, 16, "mid", "s2"), (F16, 16, 32, "mid", "s2"),
                                     (BF16, 32, 16, "n65", "subm3")):
        out.append(case("bwd_rows", f"igemm_bwd_rows/{C}/{K}/{DTN[dtype]}/{1 if C == K == 16 else 0}", scene, geom, dtype,
                        C, K))
    # the weight gradient alone
    for dtype, C, K, scene, geom in ((F16, 16, 16, "mid", "s2"), (F16, 24, 32, "mid", "k2s2"), (F16, 64, 40, "small", "s2"),
                                     (BF16, 8, 16, "mid", "k2s2"), (BF16, 32, 24, "mid", "s2"), (BF16, 136, 64, "mid", "s2"),
                                     (F32, 16, 16, "mid", "s2")):
        out.append(case("wgrad", M.wgrad_key(dtype, C, K), scene, geom, dtype, C, K))
    for dtype, C, K in ((F16, 5, 7), (BF16, 3, 12), (F32, 6, 5)):
        out.append(case("wgrad", f"wgrad_generic/{DTN[dtype]}", "mid", "s2", dtype, C, K))
    # the generic kernel (kernel volume 216, strided)
    out.append(case("fwd", "generic/f16", "mid", "k216", F16, 16, 16))
    out.append(case("dgrad", "generic/bf16", "mid", "k216", BF16, 8, 16))
    out.append(case("fwd", "generic/f32", "mid", "k216", F32, 8, 12))
    # float64
    out.append(case("fwd", "igemm_f64/fwd", "small", "subm3", F64, 7, 9))
    out.append(case("dgrad", "igemm_f64/dgrad", "mid", "s2", F64, 9, 6))
    out.append(case("wgrad", "wgrad_f64", "mid", "s2", F64, 6, 10))
    # one width beyond 256
    out.append(case("fwd", "igemm_v4w/128/f16/fwd/1/1", "small", "subm3", F16, 32, 384))
    return out


CASES = _cases()
INT8_CASE = M.case("fwd_int8", "igemm_v4/64/2/i8/fwd/1/1", "small", "subm3", torch.int8, 32, 64)
# the epilogue: bias + activation on accumulators that are NaN, +Inf and -Inf
ACT_CASES = [M.case("fwd", M.v4_key(dtype, M.padw(C, dtype), M.round_cout(K), 0, False) if dtype != F64 else "igemm_f64/fwd",
                    scene, geom, dtype, C, K, act=act, name=f"epilogue-{act}")
             for dtype, C, K, scene, geom, act in (
                 (F16, 32, 64, "small", "subm3", "relu"), (BF16, 24, 32, "mid", "s2", "leaky"),
                 (F16, 64, 128, "mid", "s2", "sigmoid"), (BF16, 32, 256, "small", "subm3", "relu"),
                 (F32, 16, 32, "small", "subm3", "relu"), (F32, 20, 16, "mid", "s2", "leaky"),
                 (F32, 16, 256, "small", "subm3", "sigmoid"), (F64, 7, 9, "small", "subm3", "relu"),
                 (F64, 5, 4, "mid", "s2", "leaky"), (F64, 6, 3, "mid", "s2", "sigmoid"))]


def _id(c):
    return M._case_id(c)


def _subm(c):
    return M.GEOMS[c["geom"]][4]


def _has_unnamed_form(c):
    """entries that can be run with rows no pair names (module docstring): not those that name every row by identity"""
    return c["entry"] in ("fwd", "fwd_stats", "bwd_rows") or not _subm(c)


@pytest.fixture(autouse=True)
def _end_the_run_at_a_gpu_fault(request):
    """A mismatch is one failed test.  A faulted device fails every later launch as well: the run ends at the first."""
    yield
    if request.node.get_closest_marker("gpu") is not None and torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"the GPU faulted in {request.node.nodeid}: {e}", returncode=3)


# ---------------------------------------------------------------- one launch through the C entries
class Tables:
    """the tables and lists of a case (row order), as the C entries take them; edit() removes the pairs of dead rows"""

    def __init__(self, c, rb):
        self.subm, self.kv = bool(rb.subm), int(rb.kv)
        self.n_in, self.n_out = rb.n_in, rb.n_out
        self.pair_fwd, self.mask_fwd = rb.pair_fwd, rb.mask_fwd
        self.pair_bwd, self.mask_bwd = (rb.pair_fwd, rb.mask_fwd) if rb.subm else (rb.pair_bwd, rb.mask_bwd)
        self.native, self.num = rb.pair_native, rb.num_per_loc
        self.identity = self.kv // 2 if rb.subm else -1
        self.lists_subm = bool(rb.subm)
        self.plan = None

    @staticmethod
    def _mask_of(pair, old):
        kv, n = pair.shape
        words = old.shape[1]
        bits = (pair >= 0).to(torch.int64)
        new = torch.zeros((n, words), dtype=torch.int64, device=pair.device)
        for k in range(kv):
            new[:, k // 32] |= bits[k] << (k % 32)
        new = torch.where(new >= 2 ** 31, new - 2 ** 32, new).to(torch.int32)
        return (old.view(torch.int32) & new).view(old.dtype).contiguous()

    def edit(self, dead_in, dead_out):
        """Every pair that names an input row of dead_in or an output row of dead_out goes: -1 in the tables, mask bits
        cleared, list entries dropped (counts and plan follow).  Rows in this rulebook's own (GPU) order."""
        di, do = dead_in.to(self.pair_fwd.device), dead_out.to(self.pair_fwd.device)
        pf = self.pair_fwd.clone()
        pf[torch.isin(pf, di.to(pf.dtype))] = -1
        pf[:, do] = -1
        self.pair_fwd, self.mask_fwd = pf, self._mask_of(pf, self.mask_fwd)
        if self.subm:
            self.pair_bwd, self.mask_bwd = self.pair_fwd, self.mask_fwd
            self.identity = -1          # (the centre pair is in the table, and gone for the dead rows)
            self.native = self.num = None
        else:
            pb = self.pair_bwd.clone()
            pb[torch.isin(pb, do.to(pb.dtype))] = -1
            pb[:, di] = -1
            self.pair_bwd, self.mask_bwd = pb, self._mask_of(pb, self.mask_bwd)
            nat, num = self.native, self.num
            cap = nat.shape[2]
            valid = torch.arange(cap, device=nat.device)[None, :] < num.to(torch.int64)[:, None]
            keep = valid & ~torch.isin(nat[0], di.to(nat.dtype)) & ~torch.isin(nat[1], do.to(nat.dtype))
            order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)
            cnt = keep.sum(1)
            live = torch.arange(cap, device=nat.device)[None, :] < cnt[:, None]
            new = torch.stack([torch.where(live, torch.gather(nat[j], 1, order), torch.full_like(nat[j], -1))
                               for j in (0, 1)])
            self.native, self.num = new.contiguous(), cnt.to(num.dtype).contiguous()
        self.plan = None
        return self

    def build_plan(self):
        from spconv_amd.pytorch import ops
        if self.plan is None and self.kv <= 128:
            self.plan = ops.wgrad_plan(self.num, self.n_in, self.kv, self.lists_subm)
        return self.plan


def _buf(shape, dtype, fill, dev):
    """a caller-owned buffer whose every byte is `fill`"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((max(n, 16),), fill, dtype=torch.uint8, device=dev)
    return raw[:n].view(dtype).reshape(shape) if n else torch.empty(shape, dtype=dtype, device=dev)


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _launch(c, tabs, f, w, d, bias, fill, dev, plan=True):
    """the case's entry, once, on buffers filled with `fill`; {name: tensor} of everything the entry writes for its caller"""
    from spconv_amd import _lib
    from spconv_amd.pytorch import ops
    L = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    C, K, kv, dtype = c["C"], c["K"], tabs.kv, c["dtype"]
    n_in, n_out = tabs.n_in, tabs.n_out
    code = None if dtype == torch.int8 else ops._dtype_code(f)
    ptr = lambda t: None if t is None else t.data_ptr()
    ws_of = lambda nbytes: _buf((max(int(nbytes), 16),), torch.uint8, fill, dev)
    got = {}
    entry = c["entry"]
    if entry in ("fwd", "fwd_stats"):
        out = _buf((n_out, K), dtype, fill, dev)
        head = (f.data_ptr(), w.data_ptr(), out.data_ptr(), tabs.pair_fwd.data_ptr(), tabs.mask_fwd.data_ptr(), None, 0,
                n_in, n_out, C, K, kv, code, tabs.identity)
        if entry == "fwd":
            ws = ws_of(L.spx_igemm_acc_bytes(n_out, K, kv)) if (kv > 32 and dtype != F64) else None
            _lib.check(L.spx_igemm_fwd(*head, ptr(bias), _act_code(c["act"]), 0.1, ptr(ws), 0 if ws is None else ws.numel(),
                                       stream))
        else:
            slots = int(L.spx_igemm_fwd_stats_slots(n_out))
            rec = _buf((3 * K * slots,), torch.float32, fill, dev)
            used = ctypes.c_int(0)
            _lib.check(L.spx_igemm_fwd_stats(*head, None, 0, 0.0, None, 0, rec.data_ptr(), slots, None, ctypes.byref(used),
                                             stream))
            assert 0 < used.value <= slots, (used.value, slots)
            got["stats"] = rec[:3 * K * used.value].view(3, K, used.value)
        got["out"] = out
    elif entry == "fwd_int8":
        out = _buf((n_out, K), torch.int8, fill, dev)
        _lib.check(L.spx_igemm_fwd_int8(f.data_ptr(), w.data_ptr(), out.data_ptr(), tabs.pair_fwd.data_ptr(),
                                        tabs.mask_fwd.data_ptr(), None, n_in, n_out, C, K, kv, tabs.identity, d.data_ptr(),
                                        bias.data_ptr(), None, 0.0, _lib.DTYPE_I8, 0, 0.0, stream))
        got["out"] = out
    elif entry == "dgrad":
        din = _buf((n_in, C), dtype, fill, dev)
        ws = None if dtype == F64 else ws_of(max(L.spx_igemm_dgrad_ws_bytes(C, K, kv, code),
                                                 L.spx_igemm_acc_bytes(n_in, C, kv)))
        _lib.check(L.spx_igemm_dgrad(d.data_ptr(), w.data_ptr(), din.data_ptr(), tabs.pair_bwd.data_ptr(),
                                     tabs.mask_bwd.data_ptr(), None, 0, n_out, n_in, C, K, kv, code, int(tabs.identity >= 0),
                                     ptr(ws), 0 if ws is None else ws.numel(), stream))
        got["din"] = din
    elif entry == "wgrad":
        dw = _buf(tuple(w.shape), dtype, fill, dev)
        assert kv <= 128                                # (one call covers 128 offsets)
        ws = ws_of(L.spx_igemm_wgrad_ws_bytes_dtype(n_in, C, K, kv, code))
        pl = tabs.build_plan() if plan else None
        _lib.check(L.spx_igemm_wgrad(f.data_ptr(), d.data_ptr(), dw.data_ptr(), tabs.native.data_ptr(), tabs.num.data_ptr(),
                                     ptr(pl), n_in, n_out, C, K, kv, code, int(tabs.lists_subm), ws.data_ptr(), ws.numel(),
                                     stream))
        got["dW"] = dw
    elif entry in ("bwd", "bwd_deferred"):
        din, dw = _buf((n_in, C), dtype, fill, dev), _buf(tuple(w.shape), dtype, fill, dev)
        ws = ws_of(L.spx_igemm_wgrad_ws_bytes(n_in, C, K, kv))
        pl = tabs.build_plan() if plan else None
        args = (f.data_ptr(), d.data_ptr(), w.data_ptr(), din.data_ptr(), dw.data_ptr(), tabs.pair_bwd.data_ptr(),
                tabs.mask_bwd.data_ptr(), None, 0, tabs.native.data_ptr(), tabs.num.data_ptr(), ptr(pl), n_in, n_out, C, K, kv,
                code, int(tabs.lists_subm), ws.data_ptr(), ws.numel(), stream)
        if entry == "bwd":
            _lib.check(L.spx_igemm_bwd(*args))
        else:
            job = ctypes.create_string_buffer(64)
            _lib.check(L.spx_igemm_bwd_deferred(*args, job))
            _lib.check(L.spx_wgrad_stage2_batch(job.raw, 1, stream))
        got["din"], got["dW"] = din, dw
    elif entry == "bwd_rows":
        wt = w.reshape(K, kv, C).permute(1, 2, 0).contiguous()
        din, dw = _buf((n_in, C), dtype, fill, dev), _buf(tuple(w.shape), dtype, fill, dev)
        ws = ws_of(L.spx_igemm_bwd_rows_ws_bytes(n_in, C, K, kv))
        _lib.check(L.spx_igemm_bwd_rows(f.data_ptr(), d.data_ptr(), wt.data_ptr(), din.data_ptr(), dw.data_ptr(),
                                        tabs.pair_bwd.data_ptr(), tabs.mask_bwd.data_ptr(), n_in, n_out, C, K, kv,
                                        int(tabs.subm), code, ws.data_ptr(), ws.numel(), stream))
        got["din"], got["dW"] = din, dw
    else:
        raise AssertionError(entry)
    torch.cuda.synchronize()
    return got


class Setup:
    """scene, tables, operands (fp64 and in the case's dtype) and row orders of a case"""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        idx, shape, bs = M.scene_indices(c["scene"])
        self.ks, st, pd, dl, self.subm = M.GEOMS[c["geom"]]
        self.rb = M.rulebook(c["scene"], c["geom"], "row")
        self.out_idx, self.cand = M.ref_pairs(c["scene"], c["geom"], dev)
        self.n_in, self.n_out = idx.shape[0], self.out_idx.shape[0]
        assert self.rb.n_out == self.n_out and self.rb.n_in == self.n_in
        out_shape = out_spatial_shape(shape, self.ks, st, pd, dl, self.subm)
        self.perm = torch.from_numpy(match_rows(self.rb.out_indices.cpu().numpy(), self.out_idx.cpu().numpy(),
                                                out_shape)).to(dev)
        fc = dict(c, dtype=F32) if c["dtype"] == torch.int8 else c
        self.f, self.w, d_gpu, self.bias = M._operands(fc, self.n_in, self.n_out, self.ks, dev)
        self.d = torch.empty_like(d_gpu)
        self.d[self.perm] = d_gpu                       # dout in the reference's row order
        self.seed = zlib.crc32(M._seed_id(fc).encode())

    def run(self, tabs, f, d, fill, plan=True):
        """f [n_in, C], d [n_out, K] fp64 in the reference's row order -> the entry's outputs"""
        c, dt = self.c, self.c["dtype"]
        bias = None if self.bias is None else self.bias.to(dt)
        return _launch(c, tabs, f.to(dt).contiguous(), self.w.to(dt).contiguous(), d[self.perm].to(dt).contiguous(), bias,
                       fill, self.dev, plan)

    def reference(self, cand, f, d):
        return conv_from_pairs(self.out_idx, cand, f, self.w, d)


class moved:
    """the case's instance key must move inside the block; its options hold there"""

    def __init__(self, c):
        self.c = c

    def __enter__(self):
        from spconv_amd import _lib
        self.L = _lib.load()
        self.before = self.L.spx_launch_count(self.c["key"].encode())
        assert self.before >= 0, f"unknown instance key {self.c['key']}"
        for name, v in self.c["opts"].items():
            self.L.spx_set_option(name.encode(), v)
        return self

    def __exit__(self, *exc):
        for name in self.c["opts"]:
            self.L.spx_set_option(name.encode(), {"SPX_PK": 1, "SPX_WS": -1}[name])
        if exc[0] is None:
            after = self.L.spx_launch_count(self.c["key"].encode())
            assert after > self.before, f"{self.c['key']} was not launched (counter {self.before} -> {after})"
        return False


def _expected(s, ref, name):
    """(want, A) of output `name` in the GPU's row order, bias and activation applied"""
    c = s.c
    if name == "out":
        want, A = ref.out, ref.out_abs
        if s.bias is not None:
            want, A = want + s.bias, A + s.bias.abs()
        return M._act(want, c["act"])[s.perm], A[s.perm]
    return (ref.din, ref.din_abs) if name == "din" else (ref.dW, ref.dW_abs)


def _check_all(s, got, ref):
    for name in ("out", "din", "dW"):
        if name in got:
            want, A = _expected(s, ref, name)
            M._check(got[name], want, A, s.c["dtype"], name, tuple(want.shape))


def _assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        same = torch.equal(_bits(a[name]), _bits(b[name]))
        if not same:
            diff = (_bits(a[name]) != _bits(b[name])).reshape(a[name].shape + (-1,)).any(-1)
            raise AssertionError(f"{what}: {name} differs in {int(diff.sum())} of {diff.numel()} elements; first at "
                                 f"{tuple(int(v) for v in torch.nonzero(diff)[0])}")


# ---------------------------------------------------------------- (a) dirty memory on entry
def _dirty(c, dev, plan=True):
    s = Setup(c, dev)
    tabs = Tables(c, s.rb)
    with moved(c):
        zero = s.run(tabs, s.f, s.d, 0x00, plan)
        ones = s.run(tabs, s.f, s.d, 0xFF, plan)
    _assert_same_bits(zero, ones, "0x00 against 0xFF on entry")
    stats = ones.pop("stats", None)
    _check_all(s, ones, s.reference(s.cand, s.f, s.d if any(k in ones for k in ("din", "dW")) else None))
    if stats is not None:
        # the records of the launch against the rows it stored: {rows, mean, M2} per workgroup merge to the column statistics
        rows, mean, m2 = (stats[j].double() for j in range(3))
        y = ones["out"].double()
        n = rows.sum(1)
        assert torch.equal(n, torch.full_like(n, float(s.n_out)))
        tot = (rows * mean).sum(1) / n
        assert torch.allclose(tot, y.mean(0), rtol=1e-4, atol=1e-5)
        var = (m2 + rows * (mean - tot[:, None]) ** 2).sum(1) / n
        assert torch.allclose(var, y.var(0, unbiased=False), rtol=1e-3, atol=1e-6)
    return ones


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[_id(c) for c in CASES])
def test_dirty_memory_on_entry(cuda, c):
    got = _dirty(c, cuda)
    if c["entry"] in ("wgrad", "bwd"):      # plan == NULL: the entry rebuilds it inside the (dirty) workspace
        _assert_same_bits({"dW": got["dW"]}, {"dW": _dirty(c, cuda, plan=False)["dW"]}, "caller's plan against plan == NULL")


@pytest.mark.gpu
def test_dirty_memory_on_entry_int8(cuda):
    import refint8
    c = INT8_CASE
    s = Setup(c, cuda)
    rng = np.random.default_rng(s.seed)
    f8 = rng.integers(-127, 128, (s.n_in, c["C"]), dtype=np.int8)
    w8 = rng.integers(-127, 128, (c["K"], *s.ks, c["C"]), dtype=np.int8)
    scale = (rng.uniform(0.5, 1.5, c["K"]) * 2e-3).astype(np.float32)
    bias = rng.uniform(-5, 5, c["K"]).astype(np.float32)
    tabs = Tables(c, s.rb)
    run = lambda fill: _launch(c, tabs, torch.from_numpy(f8).to(cuda), torch.from_numpy(w8).to(cuda),
                               torch.from_numpy(scale).to(cuda), torch.from_numpy(bias).to(cuda), fill, cuda)
    with moved(c):
        zero, ones = run(0x00), run(0xFF)
    _assert_same_bits(zero, ones, "0x00 against 0xFF on entry")
    acc = refint8.int_acc(s.out_idx, s.cand, f8, w8, device=cuda)
    want = refint8.epilogue(np.asarray(acc.cpu() if torch.is_tensor(acc) else acc), scale, bias, out="i8")
    assert np.array_equal(ones["out"].cpu().numpy(), np.asarray(want)[s.perm.cpu().numpy()])


@pytest.fixture
def stale_workspace(monkeypatch):
    from spconv_amd.pytorch import _gemm, ops
    full = lambda nbytes, device: torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=device)
    monkeypatch.setattr(_gemm, "_ws", full)
    if hasattr(ops, "_ws"):
        monkeypatch.setattr(ops, "_ws", full)
    return monkeypatch


def _module_pass(kind, dev):
    import spconv_amd.pytorch as spconv
    idx, shape, bs = M.scene_indices("small")
    C, K = 32, 64
    g = torch.Generator().manual_seed(5)
    if kind == "subm":
        net = spconv.SubMConv3d(C, K, 3, bias=True, indice_key="iso_s")
    else:
        net = spconv.SparseConv3d(C, K, 3, 2, 1, bias=True, indice_key="iso_d")
    net = net.to(dev, F16)
    with torch.no_grad():
        net.weight.copy_((torch.rand(net.weight.shape, generator=g) * 2 - 1).to(dev, F16))
        net.bias.copy_((torch.rand(net.bias.shape, generator=g) * 2 - 1).to(dev, F16))
    feats = (torch.rand((idx.shape[0], C), generator=g) * 2 - 1).to(dev, F16).requires_grad_(True)
    y = net(spconv.SparseConvTensor(feats, torch.from_numpy(idx).to(dev), shape, bs))
    dout = ((torch.rand(tuple(y.features.shape), generator=g) * 2 - 1) * 0.2).to(dev, F16)
    y.features.backward(dout)
    torch.cuda.synchronize()
    return {"out": y.features.detach(), "din": feats.grad, "dW": net.weight.grad, "db": net.bias.grad}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["subm", "strided"])
def test_modules_on_a_stale_workspace(cuda, kind, request):
    clean = _module_pass(kind, cuda)
    request.getfixturevalue("stale_workspace")
    _assert_same_bits(clean, _module_pass(kind, cuda), "0xFF workspaces against the allocator's")


# ---------------------------------------------------------------- (b) rows that no pair names
UNNAMED = [c for c in CASES if _has_unnamed_form(c)]
_seen = set()
UNNAMED_PARAMS = []
for _c in UNNAMED:
    UNNAMED_PARAMS.append((_c, "nan"))
    _fam = sorted(_families(_c))[0].split("/")[0]
    if _fam not in _seen:                   # one case per family with +Inf
        _seen.add(_fam)
        UNNAMED_PARAMS.append((_c, "inf"))


@pytest.mark.gpu
@pytest.mark.parametrize("c,value", UNNAMED_PARAMS, ids=[f"{_id(c)}-{v}" for c, v in UNNAMED_PARAMS])
def test_rows_that_no_pair_names(cuda, c, value):
    s = Setup(c, cuda)
    if s.subm:
        dead_in = dead_out = unnamed_rows(s.n_in, s.seed)
    else:
        dead_in, dead_out = unnamed_rows(s.n_in, s.seed), unnamed_rows(s.n_out, s.seed + 1)
    if c["entry"] in ("fwd", "fwd_stats") and not s.subm:
        dead_out = dead_out[:0]             # (a forward's unnamed rows are feature rows)
    tabs = Tables(c, s.rb).edit(dead_in, dead_out)
    gone_in, gone_out = dead_in.to(cuda), s.perm[dead_out.to(cuda)]          # (the reference's row order)
    cand = []
    for k, i, o in s.cand:
        keep = ~torch.isin(i, gone_in) & ~torch.isin(o, gone_out)
        cand.append((k, i[keep], o[keep]))
    v = float("nan") if value == "nan" else float("inf")
    f0, d0, f1, d1 = s.f.clone(), s.d.clone(), s.f.clone(), s.d.clone()
    f0[gone_in], d0[gone_out], f1[gone_in], d1[gone_out] = 0.0, 0.0, v, v
    with moved(c):
        zero = s.run(tabs, f0, d0, 0xFF)
        full = s.run(tabs, f1, d1, 0xFF)
    zero.pop("stats", None), full.pop("stats", None)
    _assert_same_bits(zero, full, f"unnamed rows holding 0 against {value}")
    _check_all(s, zero, s.reference(cand, f0, d0 if any(k in zero for k in ("din", "dW")) else None))


# ---------------------------------------------------------------- (c), (d) non-finite values in named rows
def named_inputs(c, cand, f, d):
    """(f, d) of the named group: fp64 operands with the poison in place (d None for a forward)"""
    seed = zlib.crc32(M._seed_id(c).encode())
    fwd_only = c["entry"] in ("fwd", "fwd_stats")
    if c["entry"] != "dgrad":
        f = poisoned(f, poison_rows(cand, f.shape[0], f.shape[1], seed))
    if not fwd_only:
        d = poisoned(d, poison_rows(cand, d.shape[0], d.shape[1], seed + 1, swap=True))
    return f, (None if fwd_only else d)


def _check_rows(got, want, A, pre, dtype, name):
    """placement of NaN / +Inf / -Inf as in the reference; the matrix's bound on the finite elements; elements whose
    accumulator is non-finite but whose activation is not (relu(-Inf) = 0, sigmoid(+-Inf) = 1 / 0) exactly"""
    for kind, g, r in zip(("NaN", "+Inf", "-Inf"), masks_of(got.double()), masks_of(want)):
        assert torch.equal(g, r), (f"{name}: {kind} in {int(g.sum())} elements, the reference has {int(r.sum())}; "
                                   f"{int((g & ~r).sum())} extra, {int((r & ~g).sum())} missing")
    fin = torch.isfinite(want)
    exact = fin & ~torch.isfinite(pre)
    assert torch.equal(got[exact].double(), want[exact].to(dtype).double()), f"{name}: act(+-Inf)"
    sel = fin & ~exact
    z = torch.zeros_like(want)
    M._check(torch.where(sel, got.double(), z).to(got.dtype), torch.where(sel, want, z), torch.where(sel, A, z), dtype, name)
    assert 0 < int((~fin).sum()) < fin.numel() and int(sel.sum()) > 0


def _named(c, dev):
    s = Setup(c, dev)
    f, d = named_inputs(c, s.cand, s.f, s.d)
    tabs = Tables(c, s.rb)
    with moved(c):
        got = s.run(tabs, f, s.d if d is None else d, 0xFF)
    got.pop("stats", None)
    ref = s.reference(s.cand, f, d)
    dtype = c["dtype"]
    if "out" in got:
        want, A = _expected(s, ref, "out")
        pre = (ref.out if s.bias is None else ref.out + s.bias)[s.perm]
        _check_rows(got["out"], want, A, pre, dtype, "out")
    if "din" in got:
        _check_rows(got["din"], ref.din, ref.din_abs, ref.din, dtype, "din")
    if "dW" in got:
        dw, want = got["dW"].double(), ref.dW
        bad_got, bad_ref = ~torch.isfinite(dw), ~torch.isfinite(want)
        assert not bool((bad_ref & ~bad_got).any()), f"dW: {int((bad_ref & ~bad_got).sum())} non-finite elements swallowed"
        named_i = torch.unique(torch.cat([i for _, i, _ in s.cand]))
        named_o = torch.unique(torch.cat([o for _, _, o in s.cand]))
        bad_c = ~torch.isfinite(f[named_i]).all(0)                       # [C]
        bad_k = ~torch.isfinite(d[named_o]).all(0)                       # [K]
        shape = [1] * want.dim()
        allowed = bad_k.reshape([-1] + shape[1:]) | bad_c.reshape(shape[:-1] + [-1])
        assert not bool((bad_got & ~allowed).any()), (f"dW: {int((bad_got & ~allowed).sum())} non-finite elements outside "
                                                      f"the poisoned channels and columns")
        sel = ~bad_got & ~bad_ref
        z = torch.zeros_like(want)
        M._check(torch.where(sel, dw, z).to(got["dW"].dtype), torch.where(sel, want, z), torch.where(sel, ref.dW_abs, z),
                 dtype, "dW")
        assert int(bad_ref.sum()) > 0 and int(sel.sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES + ACT_CASES, ids=[_id(c) for c in CASES + ACT_CASES])
def test_non_finite_values_in_named_rows(cuda, c):
    _named(c, cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("act", ["relu", "leaky", "sigmoid"])
@pytest.mark.parametrize("dtype", [F16, BF16, F32, F64], ids=["f16", "bf16", "f32", "f64"])
def test_bias_act_inplace_non_finite(cuda, dtype, act):
    from spconv_amd.pytorch import ops
    n, K = 301, 40
    g = torch.Generator().manual_seed(11)
    x = M._rounded(torch.rand((n, K), generator=g, dtype=torch.float64) * 4 - 2, dtype)
    b = M._rounded(torch.rand((K,), generator=g, dtype=torch.float64) * 2 - 1, dtype)
    x[torch.arange(0, n, 7), torch.arange(0, n, 7) % K] = float("nan")
    x[torch.arange(1, n, 7), torch.arange(1, n, 7) % K] = float("inf")
    x[torch.arange(2, n, 7), torch.arange(2, n, 7) % K] = float("-inf")
    x, b = x.to(cuda), b.to(cuda)
    got = ops.bias_act_inplace(x.to(dtype).clone(), b.to(dtype), _act_code(act), 0.1)
    torch.cuda.synchronize()
    want = M._act(x + b, act)
    A = x.abs() + b.abs() + (1.0 if act == "sigmoid" else 0.0)
    _check_rows(got, want, A, x + b, dtype, f"bias_act {act}")


@pytest.mark.gpu
@pytest.mark.parametrize("C", [24, 320], ids=["narrow", "column-blocked"])
@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=["f16", "bf16", "f32"])
def test_batchnorm_relu_eval_non_finite(cuda, dtype, C):
    """the fused evaluation-mode apply against relu(batch_norm(x)) of torch in float64: NaN stays NaN, -Inf becomes 0"""
    from spconv_amd.pytorch import norm
    n = 333
    g = torch.Generator().manual_seed(C)
    x = M._rounded(torch.rand((n, C), generator=g, dtype=torch.float64) * 4 - 2, dtype)
    r = torch.arange(0, n, 5)
    x[r, r % C], x[r + 1, (r + 1) % C], x[r + 2, (r + 2) % C] = float("nan"), float("inf"), float("-inf")
    bn = torch.nn.BatchNorm1d(C).to(cuda)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.weight[::3] *= -1                            # (a negative scale: +Inf leaves as 0, -Inf as +Inf)
        bn.bias.copy_(torch.rand(C, generator=g) - 0.5)
        bn.running_mean.copy_(torch.rand(C, generator=g) - 0.5)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    bn.eval()
    x = x.to(cuda)
    assert norm.supported(x.to(dtype), bn)
    with torch.no_grad():
        got = norm.batch_norm(x.to(dtype), bn, relu=True)
        torch.cuda.synchronize()
        sc = bn.weight.double() * torch.rsqrt(bn.running_var.double() + bn.eps)
        pre = torch.nn.functional.batch_norm(x, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(),
                                             bn.bias.double(), False, 0.0, bn.eps)
        want = torch.relu(pre)
        A = x.abs() * sc.abs() + (bn.running_mean.double() * sc).abs() + bn.bias.double().abs()
    _check_rows(got, want, A, pre, dtype, "bn+relu")


# ---------------------------------------------------------------- CPU: the table
def test_cases_claim_every_family():
    claimed = set().union(*[_families(c) for c in CASES + [INT8_CASE]])
    missing = required_families() - claimed
    assert not missing, f"families without a case: {sorted(missing)}"
    reach = M.reachable()
    for c in CASES + ACT_CASES + [INT8_CASE]:
        k = c["key"]
        assert k in reach or k.split("/")[0] in ("igemm_f64", "wgrad_f64", "igemm_v4w"), k
        assert c["scene"] in ("small", "n65", "mid", "n32769"), c["scene"]
    # every family has a case in each group it can be run in; the unnamed-rows group reaches every family but the deferred
    # form of the fused backward (same kernel as igemm_bwd) through an entry that names no row by identity
    unnamed = set().union(*[_families(c) for c in UNNAMED])
    assert required_families() - unnamed == {"int8-fwd"}, sorted(required_families() - unnamed)
    acts = {(DTN[c["dtype"]], c["act"]) for c in ACT_CASES}
    for a in ("relu", "leaky", "sigmoid"):
        assert (("f16", a) in acts or ("bf16", a) in acts) and ("f32", a) in acts and ("f64", a) in acts, a
