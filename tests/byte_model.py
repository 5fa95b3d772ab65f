"""An independent model of the BYTES a chain reads and writes, as exact sets of addresses.

cvgs_execute_many (and a group behind one gate of the descriptor queue) runs the chains of a tick concurrently only when no chain writes
what another chain reads or writes; the product decides that from byte RANGES (chains_independent, cvgs_plane_table_hull).  This module
states the same question on exact byte SETS, written from the layout definitions of include/cvgs_hip.h -- a pitched 2D view, the FOURCC
layouts (NV12, NV21, I420, YV12, P010, YUYV, UYVY, I444), the dense NCHW / CNHW / packed tensors -- and from the sample addressing of
tests/f64_model.yuv_taps, NOT from cvgs_api.cpp.  Nothing here imports oracle/ or the product package: the iop objects the tests build are
read by attribute only (a chain is [read, pointwise..., write]; a source view has data / cols / rows / step and, for the YUV layouts,
uv_offset), and the numeric codes below are those of the public C header.

    reads(chain), writes(chain)  sorted, disjoint, non-adjacent [lo, hi) intervals of byte addresses
    exact_conflict(chains)       some chain writes a byte another chain writes, or a byte ANY chain (itself included) reads
    clear(chains)                every view's closed span and every target's closed span are pairwise apart: the coarsest statement
                                 under which the product must still fuse
Groups that are neither form the grey zone (a target inside a view's row padding, between the planes of an I444 view, interleaved CNHW
writers): either answer is allowed there.

A chain whose plane table lives on the device (read.table is set) is seen by the host through ONE stated range only, the hull of all its
views: clear() takes that hull as the chain's single span.  What such a chain must do when nothing is stated (or when its caller vouches)
is a rule about the statement, not about bytes, and is left to the tests."""

# include/cvgs_hip.h
DEPTH_BYTES = {0: 1, 1: 1, 2: 2, 3: 2, 4: 4, 5: 4, 6: 8, 7: 2}  # 8U 8S 16U 16S 32S 32F 64F 16F (16BF: depth 16F plus a flag bit)
READ_PIXEL, READ_RESIZE, READ_YUV, READ_YUV_RESIZE = 0, 1, 2, 3
NV12, NV21, I420, YV12, P010, YUYV, UYVY, I444 = range(8)
WRITE_PIXEL_3D, WRITE_SPLIT, WRITE_T_SPLIT = 1, 2, 3


def type_cn(t):
    return ((t >> 3) & 63) + 1


def elem_bytes(t):
    return DEPTH_BYTES[t & 7]


def ceil_half(n):
    return (n + 1) // 2


# ---- interval sets --------------------------------------------------------------------------------------------------------------------
def normalise(intervals):
    """Sorted, disjoint, non-adjacent [lo, hi) intervals with the same union (empty ones dropped)."""
    out = []
    for lo, hi in sorted((int(a), int(b)) for a, b in intervals if b > a):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [(a, b) for a, b in out]


def intersects(a, b):
    """Do two normalised interval sets share a byte?"""
    i = j = 0
    while i < len(a) and j < len(b):
        if a[i][0] < b[j][1] and b[j][0] < a[i][1]:
            return True
        if a[i][1] <= b[j][1]:
            i += 1
        else:
            j += 1
    return False


def span(intervals):
    """[first byte, last byte + 1) of a non-empty normalised set."""
    return intervals[0][0], intervals[-1][1]


def spans_apart(a, b):
    return a[1] <= b[0] or b[1] <= a[0]


# ---- reads ----------------------------------------------------------------------------------------------------------------------------
def _is_yuv(rd):
    return rd.kind in (READ_YUV, READ_YUV_RESIZE)


def view_reads(rd, m):
    """The bytes ONE source view of the read stage may read: every sample of its width x height pixels, nothing else."""
    data, w, h, step = int(m.data), int(m.cols), int(m.rows), int(m.step)
    uv = int(getattr(m, "uv_offset", 0) or 0)
    if not _is_yuv(rd):
        row = w * type_cn(rd.src_type) * elem_bytes(rd.src_type)
        return normalise((data + y * step, data + y * step + row) for y in range(h))
    layout = getattr(rd, "yuv_layout", NV12)
    if layout in (YUYV, UYVY):  # one plane of 4-byte pixel pairs; a view of odd width reads its whole last pair
        return normalise((data + y * step, data + y * step + 4 * ceil_half(w)) for y in range(h))
    if layout == I444:  # the view's rows in the Y plane, and again uv_offset and 2 * uv_offset further (U, V)
        return normalise((data + k * uv + y * step, data + k * uv + y * step + w) for k in range(3) for y in range(h))
    es = 2 if layout == P010 else 1
    ivs = [(data + y * step, data + y * step + w * es) for y in range(h)]
    cbase = data + (uv if uv else h * step)  # 0 = the chroma plane directly below the view's `height` luma rows
    if layout in (NV12, NV21, P010):  # interleaved chroma: ceil(h / 2) rows of ceil(w / 2) (U, V) pairs, `step` apart
        ivs += [(cbase + r * step, cbase + r * step + 2 * ceil_half(w) * es) for r in range(ceil_half(h))]
    else:  # I420 / YV12: two (W/2) x (H/2) planes with rows of step / 2 bytes, the second directly behind the first
        cstep = step // 2
        for plane in (0, 1):
            first = cbase + plane * (h // 2) * cstep
            ivs += [(first + r * cstep, first + r * cstep + ceil_half(w)) for r in range(ceil_half(h))]
    return normalise(ivs)


def views(chain):
    """The views a chain reads: the first min(batch, used_planes) (planes behind them are background: nothing is read)."""
    rd = chain[0]
    return list(rd.mats)[:max(0, min(int(rd.batch), int(rd.used_planes)))]


def reads(chain):
    rd = chain[0]
    return normalise(iv for m in views(chain) for iv in view_reads(rd, m))


# ---- writes ---------------------------------------------------------------------------------------------------------------------------
def writes(chain):
    """The bytes the write stage stores: ALL `batch` planes (the ones behind used_planes receive the background)."""
    rd, wr = chain[0], chain[-1]
    batch, cn, esz = int(rd.batch), type_cn(wr.dst_type), elem_bytes(wr.dst_type)
    data, plane = int(wr.data), int(wr.width) * int(wr.height) * esz
    if wr.kind in (WRITE_SPLIT, WRITE_PIXEL_3D):  # NCHW / packed [plane][y][x]: dense, batch * cn planes' worth
        return normalise([(data, data + batch * cn * plane)])
    if wr.kind == WRITE_T_SPLIT:  # CNHW: channel k of image z at (k * N + z) planes, N = the tensor's image count
        n = max(int(wr.planes), batch)
        return normalise((data + k * n * plane, data + (k * n + batch) * plane) for k in range(cn))
    raise NotImplementedError("write kind %d has no dense extent" % wr.kind)


# ---- the two predicates ---------------------------------------------------------------------------------------------------------------
def exact_conflict(chains):
    w = [writes(c) for c in chains]
    r = [reads(c) for c in chains]
    for i in range(len(chains)):
        for j in range(len(chains)):
            if i != j and intersects(w[i], w[j]):
                return True
            if intersects(r[i], w[j]):  # j == i counts: a chain that reads its own target
                return True
    return False


def read_spans(chain):
    """The closed spans the host sees of a chain's reads: one per view -- or ONE for a device-table chain (its stated hull)."""
    rd = chain[0]
    per_view = [span(view_reads(rd, m)) for m in views(chain)]
    if getattr(rd, "table", None) is not None and per_view:
        return [(min(s[0] for s in per_view), max(s[1] for s in per_view))]
    return per_view


def clear(chains):
    targets = [span(writes(c)) for c in chains]
    for i in range(len(targets)):
        for j in range(i):
            if not spans_apart(targets[i], targets[j]):
                return False
    for c in chains:
        for s in read_spans(c):
            for t in targets:
                if not spans_apart(s, t):
                    return False
    return True


def classify(chains):
    if exact_conflict(chains):
        return "conflict"
    return "clear" if clear(chains) else "grey"


# ---- the slow way: one address per sample index (to check the sets above) ---------------------------------------------------------------
def slow_view_addresses(rd, m):
    """The same set as view_reads, built pixel by pixel from the sample addressing of the layout (tests/f64_model.yuv_taps)."""
    data, w, h, step = int(m.data), int(m.cols), int(m.rows), int(m.step)
    uv = int(getattr(m, "uv_offset", 0) or 0)
    out = set()
    layout = getattr(rd, "yuv_layout", NV12) if _is_yuv(rd) else None
    es = elem_bytes(rd.src_type)
    for y in range(h):
        for x in range(w):
            if layout is None:
                px = type_cn(rd.src_type) * es
                samples = [(data + y * step + x * px + b, 1) for b in range(px)]
            elif layout in (YUYV, UYVY):
                samples = [(data + y * step + 4 * (x // 2), 4)]  # the pixel's pair is read whole (header: odd widths too)
            elif layout == I444:
                samples = [(data + k * uv + y * step + x, 1) for k in range(3)]
            else:
                cbase = data + (uv if uv else h * step)
                samples = [(data + y * step + x * es, es)]
                if layout in (NV12, NV21, P010):
                    pair = cbase + (y // 2) * step + 2 * (x // 2) * es
                    samples += [(pair, es), (pair + es, es)]
                else:
                    first = cbase + (y // 2) * (step // 2) + x // 2
                    samples += [(first, 1), (first + (h // 2) * (step // 2), 1)]
            for addr, n in samples:
                out.update(range(addr, addr + n))
    return out
