"""cvgs_plane_table_hull against the exact byte sets of tests/byte_model.py, over a seeded grid of read stages (no GPU: the function
reads descriptors, never pixels -- the addresses below are made up).

For every read stage of the grid that cvgs_validate accepts:
  * lo == min(reads) and hi >= max(reads) + 1   -- soundness: nothing that is read lies outside the stated range;
  * hi == max(reads) + 1                        -- tightness: a range that reaches further silently un-fuses ticks (round 4's defect).
The ONE documented exception is planar chroma (I420 / YV12): source_range states "two half-width planes: the upper bound", i.e. whole
`step`-byte rows for the two quarter planes, where the last V row really ends step / 2 - width / 2 bytes earlier.  There the test asserts
hi - (max + 1) <= step, and that the exception is actually met on the grid.

The grid: surfaces of at most 97 x 61; every layout (u8 / u16 / s16 / f32 / f16 / bf16 pixels with 1-4 channels, NV12, NV21, I420, YV12,
P010, YUYV, UYVY, I444); views of 1 x 1, 1 x N, N x 1, odd and even origins and sizes, views that touch the last row and column; dense and
padded (odd) steps; uv_offset at its default / minimum and larger; used_planes of 1, batch - 1 and batch; batches scattered over two
surfaces.  A combination cvgs_validate refuses (an odd 4:2:0 width, an odd P010 step ...) is left out, and every layout must keep cases.

The model is checked here too: every small view's read set is built a second, slow way -- one address per sample index -- and compared,
and the two predicates are pinned on hand-made groups.

Not reachable through validated descriptors, hence not on the grid: source_range's clamp of width / height <= 0 to 1 (cvgs_validate
refuses empty planes before any range is taken)."""
import ctypes as C

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import byte_model as B

BASES = (0x7E0000100000, 0x7E0000180004)  # two "surfaces" far apart; 4-byte aligned (packed 4:2:2 needs it), never dereferenced
DST = (8, 4)

PLAIN_TYPES = [(name, cvgs.make_type(d, cn) | flag) for name, d, flag in (("u8", cvgs.DEPTH_8U, 0), ("u16", cvgs.DEPTH_16U, 0), ("s16", cvgs.DEPTH_16S, 0),
                                                                           ("f32", cvgs.DEPTH_32F, 0), ("f16", cvgs.DEPTH_16F, 0), ("bf16", cvgs.DEPTH_16F, capi.TYPE_FLAG_BF16))
               for cn in (1, 2, 3, 4)]
YUV420 = {"nv12": capi.YUV_NV12, "nv21": capi.YUV_NV21, "p010": capi.YUV_P010}
PLANAR = {"i420": capi.YUV_I420, "yv12": capi.YUV_YV12}
YUV422 = {"yuyv": capi.YUV_YUYV, "uyvy": capi.YUV_UYVY}

ANY_RECTS = [(0, 0, 1, 1), (96, 60, 1, 1), (5, 0, 1, 17), (0, 7, 23, 1), (3, 5, 8, 6), (4, 6, 9, 7), (0, 0, 97, 61), (90, 50, 7, 11), (1, 60, 96, 1),
             (96, 0, 1, 61), (31, 15, 2, 3), (0, 59, 97, 2)]
EVEN_RECTS = [(0, 0, 2, 2), (94, 58, 2, 2), (4, 0, 2, 18), (0, 8, 24, 2), (2, 6, 8, 6), (0, 0, 96, 60), (90, 50, 6, 10), (0, 58, 96, 2), (94, 0, 2, 60)]
ODD_TRIES = [(1, 1, 3, 3), (0, 0, 5, 2), (0, 0, 4, 3)]  # 4:2:0 views cvgs_validate may refuse: tried, kept only where it accepts
PAIR_RECTS = [(0, 0, 1, 1), (94, 60, 1, 1), (4, 0, 1, 17), (0, 7, 23, 1), (2, 5, 8, 6), (4, 6, 9, 7), (0, 0, 96, 61), (90, 50, 5, 11), (0, 60, 96, 1),
              (94, 0, 2, 61), (94, 3, 1, 4)]


def _random_rects(rng, n, fw, fh, even=False, even_x=False):
    out = []
    for _ in range(n):
        w, h = int(rng.integers(1, fw + 1)), int(rng.integers(1, fh + 1))
        x, y = int(rng.integers(0, fw - w + 1)), int(rng.integers(0, fh - h + 1))
        if even:
            x, y, w, h = x & ~1, y & ~1, max(2, w & ~1), max(2, h & ~1)
        if even_x:
            x &= ~1
        out.append((x, y, w, h))
    return out


def _accepted(lib, rd, out_cn):
    f = cvgs.make_type(cvgs.DEPTH_32F, out_cn)
    ch = cvgs.lower([rd, cvgs.WriteIOp(capi.WRITE_PIXEL_3D, f, 16, DST[0], DST[1], 0, rd.batch)])
    return lib.cvgs_validate(C.byref(ch.desc)) == capi.OK


def _stages():
    """(layout name, read stage) for the whole grid, before validation."""
    rng = np.random.default_rng(20240611)
    for name, t in PLAIN_TYPES:
        px = cvgs.elem_size(t)
        for pad in (0, 7, 12):
            step = 97 * px + pad
            surfs = [cvgs.GpuMat(61, 97, t, b, step) for b in BASES]
            rects = ANY_RECTS + _random_rects(rng, 4, 97, 61)
            mats = [surfs[i % 2].roi(*r) for i, r in enumerate(rects)]
            for used in (1, len(mats) - 1, len(mats)):
                yield name, cvgs.resize(t, cvgs.INTER_LINEAR, mats, DST, used)
            for m in mats[:6]:
                yield name, cvgs.resize(t, cvgs.INTER_LINEAR, [m], DST, 1)
    for name, layout in YUV420.items():
        es = 2 if layout == capi.YUV_P010 else 1
        t = cvgs.make_type(cvgs.DEPTH_16U if es == 2 else cvgs.DEPTH_8U, 1)
        for pad in (0, 7, 12):
            for extra_rows in (0, 6):  # the chroma plane directly below the luma plane, or further (an aligned-height decoder surface)
                step = 96 * es + pad
                surfs = []
                for b in BASES:
                    s = cvgs.GpuMat(60, 96, t, b, step)
                    s.uv_offset = (60 + extra_rows) * step if extra_rows else 0
                    surfs.append(s)
                rects = EVEN_RECTS + _random_rects(rng, 4, 96, 60, even=True)
                mats = []
                for i, r in enumerate(rects):
                    try:
                        mats.append(surfs[i % 2].nv12_roi(*r))
                    except ValueError:
                        pass
                for used in (1, len(mats) - 1, len(mats)):
                    rd = cvgs.read_nv12(mats, DST, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
                    rd.used_planes = used
                    yield name, rd
                for m in [surfs[0], surfs[1]] + mats[:5]:  # the whole surface (uv_offset 0 = height * step, or stated) and single crops
                    yield name, cvgs.read_nv12([m], DST, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
                for (x, y, w, h) in ODD_TRIES:  # odd views, spelled by hand (nv12_roi refuses them before the library can)
                    m = cvgs.GpuMat(h, w, t, BASES[0] + y * step + x * es, step)
                    m.uv_offset = 60 * step + (y // 2 - y) * step
                    yield name, cvgs.read_nv12([m], DST, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
                short = cvgs.GpuMat(20, 96, t, BASES[1], step)  # uv_offset 0 on a view shorter than its surface: chroma at 20 * step, by definition
                yield name, cvgs.read_nv12([short], DST, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
    for name, layout in PLANAR.items():
        t = cvgs.CV_8UC1
        for pad in (0, 6, 14, 7):
            sizes = [(96, 60), (2, 2), (2, 18), (24, 2), (8, 6), (90, 50), (96, 2), (5, 3)] + [(w, h) for (_, _, w, h) in _random_rects(rng, 3, 96, 60, even=True)]
            mats = [cvgs.GpuMat(h, w, t, BASES[i % 2] + 4096 * (i // 2), 96 + pad) for i, (w, h) in enumerate(sizes)]  # whole surfaces, some narrower than the pitch
            mats += [cvgs.GpuMat(h, w, t, BASES[0] + 0x20000 + 4096 * i, w) for i, (w, h) in enumerate(sizes[:4])]     # dense: step == w
            for used in (1, len(mats) - 1, len(mats)):
                rd = cvgs.read_nv12(mats, DST, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
                rd.used_planes = used
                yield name, rd
            for m in mats:
                yield name, cvgs.read_nv12([m], DST, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
    for name, layout in YUV422.items():
        t = cvgs.make_type(cvgs.DEPTH_8U, 2)
        for pad in (0, 4, 12, 7):
            surfs = [cvgs.GpuMat(61, 96, t, b, 192 + pad) for b in BASES]
            rects = PAIR_RECTS + _random_rects(rng, 4, 96, 61, even_x=True)
            mats = [surfs[i % 2].yuv422_roi(*r) for i, r in enumerate(rects)]
            for used in (1, len(mats) - 1, len(mats)):
                rd = cvgs.read_yuv422(mats, DST, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
                rd.used_planes = used
                yield name, rd
            for m in mats[:6]:
                yield name, cvgs.read_yuv422([m], DST, capi.YUV_LIMITED, capi.BT709, False, layout=layout)
    for pad in (0, 7, 12):
        step = 97 + pad
        for extra in (0, 1, 333):  # uv_offset at its minimum -- the planes touch -- and larger
            surfs = []
            for b in BASES:
                s = cvgs.GpuMat(61, 97, cvgs.CV_8UC1, b + 1, step)  # (an odd address: the layout needs no alignment)
                s.uv_offset = 60 * step + 97 + extra
                surfs.append(s)
            rects = ANY_RECTS + _random_rects(rng, 4, 97, 61)
            mats = [surfs[i % 2].yuv444_roi(*r) for i, r in enumerate(rects)]
            for used in (1, len(mats) - 1, len(mats)):
                rd = cvgs.read_yuv444(mats, DST, capi.YUV_LIMITED, capi.BT709, False)
                rd.used_planes = used
                yield "i444", rd
            for m in mats[:6]:
                yield "i444", cvgs.read_yuv444([m], DST, capi.YUV_LIMITED, capi.BT709, False)


@pytest.fixture(scope="module")
def grid(lib):
    """The validated grid, computed once: [(layout name, read stage, (lo, hi) of the product, model intervals)]."""
    out = []
    for name, rd in _stages():
        out_cn = 3 if B._is_yuv(rd) else cvgs.type_cn(rd.src_type)
        if not _accepted(lib, rd, out_cn):
            continue
        out.append((name, rd, cvgs.table_hull(rd), B.reads([rd])))
    return out


def test_the_grid_keeps_every_layout(grid):
    names = [n for n, _, _, _ in grid]
    for want in [n for n, _ in PLAIN_TYPES] + list(YUV420) + list(PLANAR) + list(YUV422) + ["i444"]:
        assert names.count(want) >= 20, "layout %s has only %d validated cases" % (want, names.count(want))
    # the variations the grid promises are met among the accepted cases
    def some(pred):
        return any(pred(rd, m) for _, rd, _, _ in grid for m in B.views([rd]))
    assert some(lambda rd, m: m.cols == 1 and m.rows == 1) and some(lambda rd, m: m.cols == 1 and m.rows > 1) and some(lambda rd, m: m.rows == 1 and m.cols > 1)
    assert some(lambda rd, m: not B._is_yuv(rd) and m.step == m.cols * cvgs.elem_size(rd.src_type)) and some(lambda rd, m: m.step & 1)
    assert some(lambda rd, m: B._is_yuv(rd) and getattr(m, "uv_offset", 0) == 0) and some(lambda rd, m: getattr(m, "uv_offset", 0) > (m.rows + 5) * m.step)
    assert any(rd.used_planes == 1 and rd.batch > 2 for _, rd, _, _ in grid) and any(rd.used_planes == rd.batch - 1 for _, rd, _, _ in grid)
    assert any(len({int(m.data) >> 18 for m in B.views([rd])}) > 1 for _, rd, _, _ in grid), "batches scattered over two surfaces"


def test_hull_is_sound_and_tight(grid):
    slack_seen = 0
    for name, rd, (lo, hi), model in grid:
        first, last1 = B.span(model)
        what = "%s batch=%d used=%d" % (name, rd.batch, rd.used_planes)
        assert lo == first, "%s: lo is %+d bytes from the first byte read" % (what, lo - first)
        assert hi >= last1, "%s: UNSOUND: %d bytes that are read lie behind the stated range" % (what, last1 - hi)
        if name in PLANAR:
            # the documented upper bound (source_range: "two half-width planes: the upper bound"): at most one row pitch of the view that ends last
            step = max(int(m.step) for m in B.views([rd]))
            assert hi - last1 <= step, "%s: %d bytes beyond the last byte read, more than a row pitch (%d)" % (what, hi - last1, step)
            slack_seen += hi > last1
        else:
            assert hi == last1, "%s: the stated range reaches %d bytes beyond the last byte read" % (what, hi - last1)
    assert slack_seen > 0, "the planar-chroma exception never occurred: drop it from the test"


def test_interval_sets_equal_the_sample_by_sample_sets(grid):
    """Every small view of the grid, a second way: one address per sample index."""
    checked = {}
    for name, rd, _, _ in grid:
        for m in B.views([rd]):
            key = (name, int(m.data), m.cols, m.rows, m.step, getattr(m, "uv_offset", 0))
            if m.cols * m.rows > 700 or key in checked:
                continue
            fast = set()
            for a, b in B.view_reads(rd, m):
                fast.update(range(a, b))
            assert fast == B.slow_view_addresses(rd, m), key
            checked[key] = True
    assert len(checked) >= 300 and {k[0] for k in checked} == {n for n, _, _, _ in grid}


class _Mat:
    def __init__(self, data, cols, rows, step, uv_offset=0):
        self.data, self.cols, self.rows, self.step, self.uv_offset = data, cols, rows, step, uv_offset


class _Read:
    def __init__(self, mats, kind=B.READ_RESIZE, src_type=16, layout=0, used=None, table=None):  # 16 = CV_8UC3
        self.kind, self.src_type, self.mats, self.batch, self.yuv_layout, self.table = kind, src_type, mats, len(mats), layout, table
        self.used_planes = len(mats) if used is None else used


class _Write:
    def __init__(self, kind, data, width=8, height=4, planes=0, dst_type=21):  # 21 = CV_32FC3
        self.kind, self.data, self.width, self.height, self.planes, self.dst_type = kind, data, width, height, planes, dst_type


def test_the_write_sets():
    rd = _Read([_Mat(1 << 20, 8, 8, 64)] * 2)
    plane = 8 * 4 * 4
    assert B.writes([rd, _Write(B.WRITE_SPLIT, 4096)]) == [(4096, 4096 + 2 * 3 * plane)]
    assert B.writes([rd, _Write(B.WRITE_PIXEL_3D, 4096)]) == [(4096, 4096 + 2 * 3 * plane)]
    # CNHW with 5 images in the tensor: three separate runs of 2 planes, 5 planes apart -- not one hull
    assert B.writes([rd, _Write(B.WRITE_T_SPLIT, 4096, planes=5)]) == [(4096 + k * 5 * plane, 4096 + (k * 5 + 2) * plane) for k in range(3)]
    assert B.writes([rd, _Write(B.WRITE_T_SPLIT, 4096, planes=2)]) == [(4096, 4096 + 6 * plane)]  # planes == batch: the runs join
    # planes behind used_planes are written, but not read
    rd1 = _Read([_Mat(1 << 20, 8, 8, 64), _Mat(1 << 21, 8, 8, 64)], used=1)
    assert B.writes([rd1, _Write(B.WRITE_SPLIT, 4096)]) == [(4096, 4096 + 6 * plane)] and B.span(B.reads([rd1, None])) == ((1 << 20), (1 << 20) + 7 * 64 + 24)


def test_the_predicates_on_hand_made_groups():
    plane = 8 * 4 * 4
    size = 3 * plane
    src = lambda at: _Read([_Mat(at, 8, 8, 64)])  # rows of 24 bytes, 40 bytes of padding behind each
    a = [src(1 << 20), _Write(B.WRITE_SPLIT, 1 << 16)]
    assert B.classify([a, [src(1 << 21), _Write(B.WRITE_SPLIT, 1 << 17)]]) == "clear"
    assert B.classify([a, [src(1 << 21), _Write(B.WRITE_SPLIT, (1 << 16) + size - 4)]]) == "conflict"  # the targets share 4 bytes
    assert B.classify([a, [src(1 << 21), _Write(B.WRITE_SPLIT, (1 << 16) + size)]]) == "clear"         # ... abut
    assert B.classify([a, [src(1 << 21), _Write(B.WRITE_SPLIT, (1 << 20) - size)]]) == "clear"         # ends where a's view begins
    assert B.classify([a, [src(1 << 21), _Write(B.WRITE_SPLIT, (1 << 20) - size + 1)]]) == "conflict"  # ... one byte into it
    assert B.classify([a, [src(1 << 21), _Write(B.WRITE_SPLIT, (1 << 20) + 7 * 64 + 24)]]) == "clear"  # begins behind a's last byte
    assert B.classify([a, [src(1 << 21), _Write(B.WRITE_SPLIT, (1 << 20) + 7 * 64 + 23)]]) == "conflict"
    # a target of 16 bytes inside the padding of a's first row: nothing read is written, but the spans meet -- grey
    tiny = _Write(B.WRITE_SPLIT, (1 << 20) + 24, width=2, height=2, dst_type=5)  # one CV_32FC1 plane of 2 x 2
    assert B.classify([a, [src(1 << 21), tiny]]) == "grey"
    # a chain that reads its own target
    assert B.classify([[src(1 << 16), _Write(B.WRITE_SPLIT, 1 << 16)], [src(1 << 21), _Write(B.WRITE_SPLIT, 1 << 17)]]) == "conflict"
    # two CNHW writers of one tensor of 4 images, images 0-1 and 2-3: interleaved, not conflicting -- grey
    t0 = [_Read([_Mat(1 << 20, 8, 8, 64)] * 2), _Write(B.WRITE_T_SPLIT, 1 << 16, planes=4)]
    t1 = [_Read([_Mat(1 << 21, 8, 8, 64)] * 2), _Write(B.WRITE_T_SPLIT, (1 << 16) + 2 * plane, planes=4)]
    assert B.classify([t0, t1]) == "grey"
    t2 = [_Read([_Mat(1 << 21, 8, 8, 64)] * 2), _Write(B.WRITE_T_SPLIT, (1 << 16) + plane, planes=4)]
    assert B.classify([t0, t2]) == "conflict"
    # a target between two crops of one frame: clear view by view, grey for a device-table chain (the host sees one hull)
    two = lambda table: _Read([_Mat(1 << 20, 8, 4, 64), _Mat((1 << 20) + 40 * 64, 8, 4, 64)], table=table)
    between = [src(1 << 21), _Write(B.WRITE_SPLIT, (1 << 20) + 8 * 64)]
    assert B.classify([[two(None), _Write(B.WRITE_SPLIT, 1 << 16)], between]) == "clear"
    assert B.classify([[two(1234), _Write(B.WRITE_SPLIT, 1 << 16)], between]) == "grey"
