"""tests/nv12_write_edge_cases.py without a GPU: the case table builds and is counted, the windows the cases run have the edges the kernels
can get wrong (from the library's plane geometry), the hand-made special-value pictures produce the stated floats, the fp32 restatement and the
float64 model agree on every windowed picture away from ties, and every chain of every case lowers, validates and is dispatched (dry run) to
the nv12w_* kernel the case names.  The stored bytes are the GPU item's (tests/test_zz_gpu_write_nv12_edges.py)."""
import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import nv12_write_edge_cases as E
from tests import nv12_write_model as M
from tests import test_gpu_nv12_write as W


@pytest.fixture(scope="module")
def walked(lib, oracle):
    """Every case walked dry: (labels, the context with its log)."""
    ctx = E.Ctx(None, lib, oracle)
    labels = []
    for label, body in E.all_cases():
        body(ctx)
        labels.append(label)
    return labels, ctx


def test_the_case_table_builds_and_is_counted():
    cases = E.all_cases()
    assert len(cases) == E.N_CASES == 34
    labels = [l for l, _ in cases]
    assert len(set(labels)) == len(labels)
    for name in E.LAYOUTS:  # every layout: one full-resolution and one resized read
        assert "%s full resolution" % name in labels and "%s resized" % name in labels
    assert sorted(E.LAYOUTS) == ["I420", "I444", "NV21", "P010", "UYVY", "YUYV", "YV12"]


def test_the_windows_have_the_edges_the_issue_names():
    ws = E.window_set()
    assert len(ws) == 6 and all(len(v) == len(E.CROPS) == 7 for v in ws.values())
    E.assert_window_coverage(ws)
    # crop 40 x 30 into 34 x 14: a 19-wide window starting at column 7; rounded down to even: 18 wide from column 8; left-aligned: from column 0
    assert ws[("PRESERVE_AR", E.PILLAR)][1] == (7, 0, 25, 13)
    assert ws[("PRESERVE_AR_RN_EVEN", E.PILLAR)][1] == (8, 0, 25, 13)
    assert ws[("PRESERVE_AR_LEFT", E.PILLAR)][1] == (0, 0, 18, 13)
    assert ws[("PRESERVE_AR", E.LETTER)][1] == (0, 11, 13, 21)
    # each mode on its own brings a window that is smaller than the surface in both targets
    for (mode, d), lst in ws.items():
        assert sum(w != (0, 0, d[0] - 1, d[1] - 1) for w in lst) >= 6, (mode, d, lst)
    # a 2 x 2 chroma block straddles a window edge: an odd first column / row, or an even last one
    assert any(w[0] & 1 for w in ws[("PRESERVE_AR", E.PILLAR)]) and any(not w[2] & 1 for w in ws[("PRESERVE_AR_LEFT", E.PILLAR)])
    assert any(w[1] & 1 for w in ws[("PRESERVE_AR", E.LETTER)]) and any(not w[3] & 1 for w in ws[("PRESERVE_AR", E.LETTER)])


@pytest.mark.parametrize("rng,prim", [(M.FULL, M.BT601), (M.LIMITED, M.BT709)])
def test_the_special_value_picture_produces_the_stated_floats(rng, prim):
    pic, checks = E.special_picture(rng, prim)
    assert pic.shape == (8, 16, 3) and pic.dtype == np.float32
    assert E.assert_special_picture(pic, checks, rng, prim) == len(checks)
    exact = [(p, float(c)) for p, _, _, c in checks if not isinstance(c, str)]
    named = [(p, c) for p, _, _, c in checks if isinstance(c, str)]
    for plane in (0, 1, 2):  # Y, and separately the U and the V mean
        ties = [v for p, v in exact if p == plane and v - np.floor(v) == 0.5]
        assert any(int(v) % 2 == 0 for v in ties) and any(int(v) % 2 == 1 for v in ties), (plane, ties)
        for t in ties:  # just either side of every tie
            lo, hi = float(np.nextafter(np.float32(t), np.float32(-1e9))), float(np.nextafter(np.float32(t), np.float32(1e9)))
            assert (plane, lo) in exact and (plane, hi) in exact, (plane, t)
        assert {c for p, c in named if p == plane} >= {"neg", "big", ">2^31", "<-2^31"}, plane
    assert {c for p, c in named if p in (1, 2)} >= {"+inf", "-inf", "nan"}
    if rng == M.FULL:  # (a limited-range Y is y * sy + 16 and a chroma sample c + 128: neither can be -0)
        assert any(p == 0 and v == 0.0 and np.signbit(np.float32(c)) for (p, v), (_, _, _, c) in
                   zip([(p, float(c)) if not isinstance(c, str) else (p, None) for p, _, _, c in checks], checks) if v is not None)
    # the picture holds non-finite values in single channels of single pixels
    assert np.isnan(pic).sum() == 1 and np.isinf(pic).sum() == 2
    # a check that does not hold is noticed: move one solved pixel by one float
    bad = pic.copy()
    plane, r, c, _ = next(k for k in checks if k[0] == 0 and not isinstance(k[3], str))
    bad[r, c, 2] = np.nextafter(bad[r, c, 2], np.float32(1e9)) + np.float32(1.0)
    with pytest.raises(AssertionError):
        E.assert_special_picture(bad, checks, rng, prim)


def test_fp32_restatement_and_float64_model_agree_on_the_windowed_pictures_away_from_ties(walked):
    """Bytes differ only where the float64 value lies within 1e-3 of a tie, and at most 2 % of a picture's bytes lie that close: a condition on
    the sources' seeds and the background (a constant background near a tie would fail it), checked here."""
    _, ctx = walked
    pictures = 0
    for e in ctx.log:
        if not e["windowed"]:
            continue
        rng, prim, layout = e["out"]
        for z in range(e["rgb"].shape[0]):
            rgb = e["rgb"][z]
            a, b = M.write_f32(rgb, rng, prim, layout), M.write_f64(rgb, rng, prim, layout)
            Y, ub, vb = M.yuv_f64(rgb, rng, prim)
            cf = np.empty((ub.shape[0], 2 * ub.shape[1]))
            cf[:, 0::2], cf[:, 1::2] = (ub, vb) if layout == M.NV12 else (vb, ub)
            vals = np.concatenate([Y.ravel(), cf.ravel()])
            near = np.abs(vals - np.floor(vals) - 0.5) <= 1e-3
            differ = np.concatenate([(a[0] != b[0]).ravel(), (a[1] != b[1]).ravel()])
            step = np.concatenate([np.abs(a[i].astype(np.int32) - b[i].astype(np.int32)).ravel() for i in (0, 1)])
            assert not (differ & ~near).any() and step.max() <= 1, (e["what"], z, int((differ & ~near).sum()))
            assert near.mean() <= 0.02, (e["what"], z, float(near.mean()))
            pictures += 1
    print("%d windowed pictures" % pictures)
    assert pictures >= 150


def test_every_chain_lowers_and_is_dispatched_to_the_kernel_its_case_names(walked):
    """The walk itself asserts cvgs_validate and the dry-run kernel name of every chain (Ctx.lowers), forced generic too wherever the fast
    kernel is dispatched; here: that every case was walked, and how the chains divide between the two kernels."""
    labels, ctx = walked
    assert len(labels) == E.N_CASES
    fast = [e["what"] for e in ctx.log if e["kernel"] == E.FAST]
    interp = [e["what"] for e in ctx.log if e["kernel"] == E.INTERP]
    assert len(fast) == 21 and len(interp) == 29, (len(fast), len(interp))
    for name in E.LAYOUTS:
        assert "%s full resolution" % name in interp and "%s resized" % name in interp
    assert sum(e["windowed"] for e in ctx.log) == 30


def test_the_dry_run_names_as_tests_test_yuv_dispatch_names_asks_them(lib):
    """cvgs_kernel_name over host memory, the chains spelt out once more without the case module's helpers."""
    _, hm, _ = W.frame(None, "NV12")
    out = cvgs.write_nv12([W.Surface("cpu", 34, 14).mat])
    rd = cvgs.read_nv12([hm.nv12_roi(2, 4, 40, 30)], (34, 14), capi.YUV_LIMITED, capi.BT601, alpha=False)
    rd.ar = cvgs.PRESERVE_AR
    assert cvgs.kernel_name(rd, out) == "nv12w_nv12_resize" and cvgs.kernel_name(rd, out, flags=capi.CHAIN_FORCE_GENERIC) == "nv12w_interp"
    assert cvgs.kernel_name(rd, cvgs.multiply(cvgs.CV_32FC3, [0.5] * 3), out) == "nv12w_interp"
    for name, lay in E.LAYOUTS.items():
        m = E.source(None, name)[1]
        full = cvgs.write_nv12([W.Surface("cpu", m.cols, m.rows).mat])
        assert cvgs.kernel_name(cvgs.read_nv12(m, None, alpha=False, layout=lay), *([cvgs.multiply(cvgs.CV_32FC3, [0.25] * 3)] if name == "P010" else []),
                                full) == "nv12w_interp", name
        if name != "NV21":
            assert cvgs.kernel_name(cvgs.read_nv12(m, (34, 14), alpha=False, layout=lay), out) == "nv12w_interp", name
