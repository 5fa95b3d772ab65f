"""cvgs_warp_tables_from_points without a GPU: cvgs_warp_table_build_host (the bytes the kernel must write) against the independent
float64 model of tests/warp_point_cases.py, the validity rules pinned by hand, every validation error of both entry points (all of it is
decided on the host before the first HIP call), and the lowering of warp chains over a caller-owned device table."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import helpers as H
from tests import warp_point_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2.0 ** -23  # the final narrowing to float is the only rounding that matters (<= 2^-24)


def _frame(cv_type=cvgs.CV_8UC3, rows=61, cols=97, step=304, data=4096):
    return cvgs.GpuMat(rows, cols, cv_type, data, step)


def _desc(**kw):
    tmpl = kw.pop("tmpl", P.TMPL5)
    return cvgs.warp_table_desc(kw.pop("frame", None) or _frame(), kw.pop("points", 1 << 20), kw.pop("table", 2 << 20), kw.pop("max_items", 24),
                                kw.pop("dsize", (112, 112)), tmpl, kw.pop("fit", cvgs.WARP_FIT_SIMILARITY), kw.pop("warp_type", cvgs.WARP_AFFINE),
                                kw.pop("count", None), kw.pop("valid", None))


def _host(pts, tmpl, fit=cvgs.WARP_FIT_SIMILARITY, count=None, dsize=(112, 112), frame=None):
    """(entries: structured array, valid: bool [n]) from cvgs_warp_table_build_host."""
    d = _desc(frame=frame, max_items=len(pts), tmpl=tmpl, fit=fit, dsize=dsize)
    raw, valid = cvgs.build_warp_table_host(d, pts, count)
    tab = np.frombuffer(raw, np.dtype([("data", "<u8"), ("w", "<i4"), ("h", "<i4"), ("step", "<i4"), ("m", "<f4", (9,)), ("dw", "<i4"), ("dh", "<i4")]))
    return tab, np.array(valid, bool), raw


def _held_to_model(name, fit, tmpl, pts):
    tab, valid, _ = _host(pts, tmpl, fit)
    # the test's own preconditions: landmark spread above 1 px, coordinates below 2^14
    p64 = pts.astype(np.float64)
    spread = np.sqrt(((p64 - p64.mean(axis=1, keepdims=True)) ** 2).sum(axis=(1, 2)) / pts.shape[1])
    assert spread.min() > 1.0 and np.abs(pts).max() < 2 ** 14, (name, spread.min(), np.abs(pts).max())
    assert valid.all(), (name, np.flatnonzero(~valid)[:5])
    model = P.model_inverse(fit, pts, tmpl)
    lin, tr = P.errors(tab["m"], model)
    print("%s: %d items, linear error max %.3g, translation error max %.3g (bound %.3g)" % (name, len(pts), lin.max(), tr.max(), BOUND))
    assert lin.max() <= BOUND and tr.max() <= BOUND, (name, lin.max(), tr.max(), int(lin.argmax()), int(tr.argmax()))
    assert (tab["m"][:, 6:] == np.array([0, 0, 1], np.float32)).all()
    return lin.max(), tr.max()


def test_host_builder_is_held_to_the_svd_model():
    """20,000 random 5-point items (full-circle rotation, scale 0.2..6, translation 0..4000, 2 px noise, float32 points) and 2,000 each
    of K = 2, 3, 16 and a mirrored landmark set: every matrix within 2^-23 of Umeyama's SVD fit in float64, inverted by np.linalg.inv."""
    total = 0
    for name, tmpl, pts in P.similarity_grid(20000, 2000):
        _held_to_model(name, cvgs.WARP_FIT_SIMILARITY, tmpl, pts)
        total += len(pts)
    assert total >= 28000


def test_host_builder_affine3_is_held_to_the_solve_model():
    pts = P.random_affine_items(4000, 11)
    _held_to_model("affine3", cvgs.WARP_FIT_AFFINE3, P.TMPL_BOX, pts)
    # the fit is exact at the corners: M (q_j, 1) = p_j
    tab, _, _ = _host(pts[:50], P.TMPL_BOX, cvgs.WARP_FIT_AFFINE3)
    m = tab["m"].astype(np.float64).reshape(-1, 3, 3)
    q1 = np.concatenate([P.TMPL_BOX.astype(np.float64), np.ones((3, 1))], axis=1)
    back = np.einsum("nij,kj->nki", m[:, :2, :], q1)
    assert np.abs(back - pts[:50]).max() <= 4700 * 3 * 2.0 ** -23


def test_forward_fit_direction_and_pixel_centres():
    """Landmarks that ARE the template moved by (+7, +3): the table maps destination (x, y) to source (x + 7, y + 3) exactly."""
    pts = (P.TMPL5.astype(np.float64) + np.array([7.0, 3.0])).astype(np.float32)[None]
    tab, valid, _ = _host(pts, P.TMPL5)
    assert valid[0]
    np.testing.assert_allclose(tab["m"][0], [1, 0, 7, 0, 1, 3, 0, 0, 1], atol=2e-5)
    # a 90 degree rotation about the origin, scale 2: p = 2 R q  ->  dst -> src is the same map
    q = P.TMPL5.astype(np.float64)
    pts = (2.0 * np.stack([-q[:, 1], q[:, 0]], axis=1)).astype(np.float32)[None]
    tab, _, _ = _host(pts, P.TMPL5)
    np.testing.assert_allclose(tab["m"][0], [0, -2, 0, 2, 0, 0, 0, 0, 1], atol=2e-5)


@pytest.mark.parametrize("k", [2, 5, 16])
def test_validity_rules_pinned(k):
    """NaN / +inf / -inf in each coordinate slot, coincident landmarks: the documented entry byte for byte, valid_out equals the model; the
    frame's data / w / h / step and the target are in every entry."""
    tmpl = {2: P.TMPL2, 5: P.TMPL5, 16: P.TMPL16}[k]
    pts, want_valid = P.pinned_invalid(k, tmpl)
    assert len(pts) == 3 + 6 * k and (~want_valid).sum() == 6 * k + 1
    frame = _frame(data=0x7f0012345600)
    tab, valid, raw = _host(pts, tmpl, dsize=(70, 9), frame=frame)
    assert (valid == want_valid).all() and (valid == P.model_valid(P.SIMILARITY, pts)).all()
    inv = P.entry_bytes(frame.data, 97, 61, 304, P.INVALID_M, 70, 9)
    for i, ok in enumerate(want_valid):
        e = raw[64 * i:64 * i + 64]
        assert (e == inv) == (not ok), (i, e.hex())
        assert e[:20] == inv[:20] and e[56:] == inv[56:]
        if ok:
            assert np.isfinite(tab["m"][i]).all()


def test_affine3_validity_pinned():
    pts, _ = P.pinned_invalid(3, P.TMPL_BOX + np.float32(5.0))
    tab, valid, raw = _host(pts, P.TMPL_BOX, cvgs.WARP_FIT_AFFINE3)
    want = P.model_valid(P.AFFINE3, pts)
    assert (valid == want).all() and (~want).sum() == 18  # coincident corners are a (degenerate but finite) affine: valid
    inv = P.entry_bytes(4096, 97, 61, 304, P.INVALID_M, 112, 112)
    assert all((raw[64 * i:64 * i + 64] == inv) == (not ok) for i, ok in enumerate(want))
    # an overflow of the narrowing (finite doubles, infinite floats) is invalid too
    big = np.array([[[0, 0], [3e38, 0], [0, 3e38]]], np.float32)
    _, valid, raw = _host(big, np.array([[0, 0], [0.5, 0], [0, 0.5]], np.float32), cvgs.WARP_FIT_AFFINE3)
    assert not valid[0] and raw[:64] == inv


@pytest.mark.parametrize("count,live", [(None, 7), (0, 0), (1, 1), (6, 6), (7, 7), (12, 7), (-3, 0)])
def test_count_rule(count, live):
    pts = P.random_items(P.TMPL5, 7, 21)
    full, _, raw_full = _host(pts, P.TMPL5)
    tab, valid, raw = _host(pts, P.TMPL5, count=count)
    assert valid.tolist() == [True] * live + [False] * (7 - live) and (valid == P.model_valid(P.SIMILARITY, pts, count)).all()
    inv = P.entry_bytes(4096, 97, 61, 304, P.INVALID_M, 112, 112)
    assert raw == raw_full[:64 * live] + inv * (7 - live)


# ---- validation ---------------------------------------------------------------------------------------------------------------------
def _set_tmpl(d, i, x, y):
    d.tmpl[i][0], d.tmpl[i][1] = x, y


BAD = [  # (what, descriptor mutation, status, message fragment)
    ("struct_size", lambda d: setattr(d, "struct_size", 216), capi.ERR_INVALID, b"size mismatch"),
    ("flags", lambda d: setattr(d, "flags", 1), capi.ERR_INVALID, b"flags must be 0"),
    ("read kind out of range", lambda d: setattr(d, "read_kind", 9), capi.ERR_INVALID, b"bad read kind"),
    ("pixel reads", lambda d: setattr(d, "read_kind", capi.READ_PIXEL), capi.ERR_UNSUPPORTED, b"WARP_AFFINE / WARP_PERSPECTIVE"),
    ("resize reads", lambda d: setattr(d, "read_kind", capi.READ_RESIZE_LINEAR), capi.ERR_UNSUPPORTED, b"WARP_AFFINE / WARP_PERSPECTIVE"),
    ("NV12 reads", lambda d: setattr(d, "read_kind", capi.READ_NV12_RESIZE_LINEAR), capi.ERR_UNSUPPORTED, b"WARP_AFFINE / WARP_PERSPECTIVE"),
    ("max_items 0", lambda d: setattr(d, "max_items", 0), capi.ERR_INVALID, b"max_items must be in [1, 65535]"),
    ("max_items 65536", lambda d: setattr(d, "max_items", 65536), capi.ERR_INVALID, b"max_items must be in [1, 65535]"),
    ("fit", lambda d: setattr(d, "fit", 2), capi.ERR_INVALID, b"bad warp fit"),
    ("similarity with 1 point", lambda d: setattr(d, "n_points", 1), capi.ERR_INVALID, b"2..16 points"),
    ("similarity with 17 points", lambda d: setattr(d, "n_points", 17), capi.ERR_INVALID, b"2..16 points"),
    ("affine3 with 5 points", lambda d: setattr(d, "fit", capi.WARP_FIT_AFFINE3), capi.ERR_INVALID, b"exactly 3 points"),
    ("null points", lambda d: setattr(d, "points", None), capi.ERR_INVALID, b"points is null"),
    ("points alignment", lambda d: setattr(d, "points", (1 << 20) + 2), capi.ERR_INVALID, b"alignment"),
    ("count alignment", lambda d: setattr(d, "count", (3 << 20) + 1), capi.ERR_INVALID, b"alignment"),
    ("valid alignment", lambda d: setattr(d, "valid_out", (3 << 20) + 2), capi.ERR_INVALID, b"alignment"),
    ("target 0", lambda d: setattr(d, "dst_width", 0), capi.ERR_INVALID, b"warp target must be positive"),
    ("target negative", lambda d: setattr(d, "dst_height", -4), capi.ERR_INVALID, b"warp target must be positive"),
    ("target too large", lambda d: setattr(d, "dst_height", (1 << 24) + 1), capi.ERR_UNSUPPORTED, b"2^24"),
    ("template NaN", lambda d: _set_tmpl(d, 3, float("nan"), 1.0), capi.ERR_INVALID, b"not finite"),
    ("template inf", lambda d: _set_tmpl(d, 0, 1.0, float("inf")), capi.ERR_INVALID, b"not finite"),
    ("template coincides", lambda d: [_set_tmpl(d, i, 5.0, 6.0) for i in range(5)], capi.ERR_INVALID, b"all coincide"),
    ("affine3 template of zero area", lambda d: (setattr(d, "fit", capi.WARP_FIT_AFFINE3), setattr(d, "n_points", 3),
                                                 [_set_tmpl(d, i, 1.0 + i, 2.0 + 2 * i) for i in range(3)]), capi.ERR_INVALID, b"zero area"),
    ("source type", lambda d: setattr(d, "src_type", capi.make_type(capi.DEPTH_8U, 5)), capi.ERR_INVALID, b"bad source type"),
    ("CV_64F source", lambda d: (setattr(d, "src_type", cvgs.CV_64FC1), setattr(d.frame, "step", 1024)), capi.ERR_UNSUPPORTED, b"CV_64F"),
    ("null frame", lambda d: setattr(d.frame, "data", None), capi.ERR_INVALID, b"empty source plane"),
    ("empty frame", lambda d: setattr(d.frame, "height", 0), capi.ERR_INVALID, b"empty source plane"),
    ("frame too wide", lambda d: (setattr(d.frame, "width", (1 << 24) + 1), setattr(d.frame, "step", 1 << 30)), capi.ERR_UNSUPPORTED, b"2^24 pixels"),
    ("frame too tall", lambda d: setattr(d.frame, "height", (1 << 24) + 1), capi.ERR_UNSUPPORTED, b"2^24 pixels"),
    ("step", lambda d: setattr(d.frame, "step", 97 * 3 - 1), capi.ERR_INVALID, b"step smaller than a row"),
    ("uv_offset", lambda d: setattr(d.frame, "uv_offset", 64), capi.ERR_INVALID, b"uv_offset belongs to the NV12 kinds"),
]
BAD_DEVICE_ONLY = [  # cvgs_warp_table_build_host writes to its own argument and ignores desc.table_out
    ("null table", lambda d: setattr(d, "table_out", None), capi.ERR_INVALID, b"table_out is null"),
    ("table alignment", lambda d: setattr(d, "table_out", (2 << 20) + 4), capi.ERR_INVALID, b"alignment"),
]


@pytest.mark.parametrize("what,mut,code,msg", BAD + BAD_DEVICE_ONLY, ids=[b[0] for b in BAD + BAD_DEVICE_ONLY])
def test_validation_errors_device_entry_point(lib, what, mut, code, msg):
    d = _desc()
    mut(d)
    arr = (capi.WarpTableDesc * 1)(d)
    rc = lib.cvgs_warp_tables_from_points(arr, 1, None)
    assert rc == code and msg in lib.cvgs_last_error(), (what, rc, lib.cvgs_last_error())
    with pytest.raises(capi.CvgsError):
        cvgs.warp_tables_from_points(None, [d])


@pytest.mark.parametrize("what,mut,code,msg", BAD, ids=[b[0] for b in BAD])
def test_validation_errors_host_entry_point(lib, what, mut, code, msg):
    pts = np.zeros((24, 17, 2), np.float32)
    cnt = C.c_int32(24)
    out = (C.c_uint8 * (64 * 24))()
    d = _desc(points=pts.ctypes.data, count=C.addressof(cnt))
    mut(d)
    rc = lib.cvgs_warp_table_build_host(C.byref(d), out)
    assert rc == code and msg in lib.cvgs_last_error(), (what, rc, lib.cvgs_last_error())
    assert bytes(out) == bytes(64 * 24)  # nothing was written


def test_null_arguments_n_out_of_range_and_overlap(lib):
    assert lib.cvgs_warp_tables_from_points(None, 1, None) == capi.ERR_INVALID and b"null descriptors" in lib.cvgs_last_error()
    assert lib.cvgs_warp_table_build_host(None, None) == capi.ERR_INVALID and b"null argument" in lib.cvgs_last_error()
    d = _desc()
    assert lib.cvgs_warp_table_build_host(C.byref(d), None) == capi.ERR_INVALID
    for n in (0, -1, 17):
        arr = (capi.WarpTableDesc * 17)(*([_desc(table=(2 << 20) + 4096 * k) for k in range(17)]))
        assert lib.cvgs_warp_tables_from_points(arr, n, None) == capi.ERR_INVALID and b"[1, 16]" in lib.cvgs_last_error()
    # the SECOND descriptor of a call is validated like the first
    arr = (capi.WarpTableDesc * 2)(d, _desc(max_items=0, table=4 << 20))
    assert lib.cvgs_warp_tables_from_points(arr, 2, None) == capi.ERR_INVALID and b"max_items" in lib.cvgs_last_error()
    # output buffers of one call that overlap: two tables, a table and a validity buffer, a table and its own validity buffer
    for a, b in ((_desc(), _desc(table=(2 << 20) + 64 * 23)), (_desc(), _desc(table=4 << 20, valid=(2 << 20) + 64)), (_desc(valid=(2 << 20) + 1000), None)):
        arr = (capi.WarpTableDesc * 2)(a, b if b is not None else _desc(table=4 << 20))
        assert lib.cvgs_warp_tables_from_points(arr, 2, None) == capi.ERR_INVALID and b"overlap" in lib.cvgs_last_error(), lib.cvgs_last_error()


def test_layout(lib, tmp_path):
    """A C99 -pedantic -Werror compile of the extension header pins sizeof(cvgs_warp_table_desc); the binding mirrors it."""
    assert [lib.cvgs_warp_table_bytes(n) for n in (-1, 0, 1, 24, 65535)] == [0, 0, 64, 64 * 24, 64 * 65535]
    assert C.sizeof(capi.WarpTableDesc) == 224
    W = capi.WarpTableDesc
    assert (W.frame.offset, W.src_type.offset, W.fit.offset, W.tmpl.offset, W.max_items.offset, W.points.offset, W.valid_out.offset) == (8, 32, 48, 56, 184, 192, 216)
    src = tmp_path / "ext.c"
    src.write_text('#include <stddef.h>\n#include "include/cvgs_hip_ext.h"\n'
                   'int main(void) { cvgs_warp_table_desc d; d.struct_size = (uint32_t)sizeof d;\n'
                   '  return d.struct_size == 224 && offsetof(cvgs_warp_table_desc, tmpl) == 56 && offsetof(cvgs_warp_table_desc, points) == 192\n'
                   '         && sizeof(cvgs_box_table_desc) == 96 ? 0 : 1; }\n')
    exe = tmp_path / "ext"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + ROOT, str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


# ---- lowering -----------------------------------------------------------------------------------------------------------------------
N = 24  # more planes than a CV_64F program's inline block (8): the host-described twin of that shape reads a table too


def _chain(rd, cn, out, dsize, kind="f32"):
    f = cvgs.make_type(cvgs.CV_32F, cn)
    ops = [rd, cvgs.cvtColor(cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA, f), cvgs.multiply(f, [H.K1_ALPHA] * cn),
           cvgs.subtract(f, H.K1_SUB[cn]), cvgs.divide(f, H.K1_DIV[cn])]
    if kind in ("f16", "bf16"):
        o = cvgs.make_type(cvgs.CV_16F, cn) | (capi.TYPE_FLAG_BF16 if kind == "bf16" else 0)
        return ops + [cvgs.convertTo(f, o), cvgs.split_tensor(o, out, dsize[0], dsize[1], N)]
    if kind == "packed":
        return ops + [cvgs.WriteIOp(capi.WRITE_PIXEL_3D, f, out, dsize[0], dsize[1], 0, N)]
    if kind == "f64":
        d = cvgs.make_type(cvgs.CV_64F, cn)
        return ops + [cvgs.convertTo(f, d), cvgs.multiply(d, [1.0 / 3.0] * cn), cvgs.convertTo(d, f), cvgs.split_tensor(f, out, dsize[0], dsize[1], N)]
    return ops + [cvgs.split_tensor(f, out, dsize[0], dsize[1], N)]


def _host_twin(kind, frame, dsize, used=None, default=None):
    rd = cvgs.ReadIOp(kind, frame.cv_type, [frame] * N, used, dsize, cvgs.IGNORE_AR, default)
    rd.warp = [1.0, 0.0, 0.5, 0.0, 1.0, 0.25, 0.0, 0.0, 1.0] * N
    rd.warp_sizes = None
    return rd


LOWER = [(cvgs.CV_8UC3, 3, "f32", 0), (cvgs.CV_8UC3, 3, "f16", 0), (cvgs.CV_8UC3, 3, "bf16", 0), (cvgs.CV_8UC3, 3, "packed", 0),
         (cvgs.CV_8UC4, 4, "f32", 0), (cvgs.CV_8UC4, 4, "f16", 0), (cvgs.CV_8UC4, 4, "bf16", 0), (cvgs.CV_8UC4, 4, "packed", 0),
         (cvgs.CV_8UC3, 3, "f32", capi.CHAIN_FORCE_GENERIC), (cvgs.CV_8UC3, 3, "f64", 0), (cvgs.CV_16UC3, 3, "f32", 0)]


@pytest.mark.parametrize("warp_type", [cvgs.WARP_AFFINE, cvgs.WARP_PERSPECTIVE], ids=["affine", "perspective"])
@pytest.mark.parametrize("cv_type,cn,kind,flags", LOWER, ids=["%d-%s-%d" % (c[0], c[2], c[3]) for c in LOWER])
def test_lowering_names_equal_the_host_described_twin(lib, warp_type, cv_type, cn, kind, flags):
    frame = _frame(cv_type, step=97 * 8 + 24)
    rk = capi.READ_WARP_AFFINE if warp_type == cvgs.WARP_AFFINE else capi.READ_WARP_PERSPECTIVE
    dev = _chain(cvgs.warp_table(warp_type, frame, 2 << 20, N, (70, 9)), cn, 8 << 20, (70, 9), kind)
    host = _chain(_host_twin(rk, frame, (70, 9)), cn, 8 << 20, (70, 9), kind)
    low = cvgs.lower(dev, flags)
    r = low.desc.read
    assert (r.kind, r.batch, r.used_planes, r.src, r.flags) == (rk, N, N, 2 << 20, capi.READ_FLAG_TABLE_ON_DEVICE)
    assert not r.warp_matrices and not r.warp_dst_sizes
    assert (r.table_src_lo, r.table_src_hi) == (4096, 4096 + 60 * (97 * 8 + 24) + 97 * cvgs.elem_size(cv_type))
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.OK, lib.cvgs_last_error()
    name = cvgs.kernel_name(*dev, flags=flags)
    assert name == cvgs.kernel_name(*host, flags=flags)
    base = "warp_affine" if warp_type == cvgs.WARP_AFFINE else "warp_perspective"
    if kind == "f64":
        assert name == "warp64_table"
    elif flags or cv_type == cvgs.CV_16UC3:
        assert name == base + "_interp"
    else:
        want = {"f32": "_swap_mul_sub_div", "f16": "_swap_mul_sub_div_f16", "bf16": "_swap_mul_sub_div_bf16", "packed": "_packed_f32"}[kind]
        assert name == "%s_u8c%d%s" % (base, cn, want)


def test_lowering_used_planes_and_refusals(lib):
    frame = _frame()
    ops = _chain(cvgs.warp_table(cvgs.WARP_AFFINE, frame, 2 << 20, N, (16, 8), used_planes=20, default_value=[1.0, 2.0, 3.0]), 3, 8 << 20, (16, 8))
    low = cvgs.lower(ops)
    assert (low.desc.read.batch, low.desc.read.used_planes, list(low.desc.read.background)[:3]) == (N, 20, [1.0, 2.0, 3.0])
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.OK, lib.cvgs_last_error()
    # matrices or per-plane sizes beside a device table
    m = (C.c_float * (9 * N))()
    low.desc.read.warp_matrices = C.cast(m, C.POINTER(C.c_float))
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_INVALID and b"must be null" in lib.cvgs_last_error()
    low = cvgs.lower(ops)
    sz = (C.c_int32 * (2 * N))(*([16, 8] * N))
    low.desc.read.warp_dst_sizes = C.cast(sz, C.POINTER(C.c_int32))
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_INVALID and b"must be null" in lib.cvgs_last_error()
    # the table's plane extent is the chain's to state
    low = cvgs.lower(ops)
    low.desc.read.dst_width = 0
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_INVALID
    # used_planes beyond the batch, a batch beyond 65535
    low = cvgs.lower(ops)
    low.desc.read.used_planes = N + 1
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_INVALID
    low = cvgs.lower(ops)
    low.desc.read.batch = 65536
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_INVALID
    # CV_64F sources take host descriptors
    f64 = _frame(cvgs.CV_64FC3, step=97 * 24)
    f = cvgs.CV_32FC3
    low = cvgs.lower([cvgs.warp_table(cvgs.WARP_AFFINE, f64, 2 << 20, N, (16, 8)), cvgs.split_tensor(f, 8 << 20, 16, 8, N)])
    assert lib.cvgs_validate(C.byref(low.desc)) == capi.ERR_UNSUPPORTED and b"CV_64F" in lib.cvgs_last_error()
    # the host builders of PLANE tables keep refusing warp kinds
    low = cvgs.lower(ops)
    buf = (C.c_uint8 * (64 * N))()
    assert lib.cvgs_plane_table_build(C.byref(low.desc.read), buf) != capi.OK
