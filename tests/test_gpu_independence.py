"""The chain-independence decision of cvgs_execute_many (and of a queue group) against the exact byte sets of tests/byte_model.py.

All chains of a group live in ONE arena -- a numpy byte buffer mirrored in one device tensor -- with sources and targets at seeded
offsets, so that a conflict is an ordinary byte overlap.  For every group the model says "conflict" (some chain writes a byte another
writes or any chain reads), "clear" (all view spans and target spans pairwise apart) or "grey" (neither: either answer is allowed).

THE DECISION (test_node_counts): the group is captured with tests/test_gpu_many._captured_kernel_nodes -- nothing is launched, the graph
is never replayed -- and  conflict => one kernel node per chain,  clear => exactly ONE node,  grey => no assertion.
THE MEANING (test_sequential_meaning): every deliberate placement and eight random groups per family are run through cvgs.executeMany
on the device arena and, chain after chain in order, through the CPU oracle on the host arena (packed 4:2:2 and planar 4:4:4, which the
oracle does not know: the composed values of tests/yuv422_cases.Expect / tests/yuv444_cases.Expect); the WHOLE arena is compared byte for
byte (NaN payloads as in tests/test_gpu_fuzz.py).  That holds fused and un-fused groups alike to the sequential meaning and shows that
no byte outside the targets moved.  Grey groups are executed too (their targets lie in bytes no chain reads).  A chain that reads its OWN
target is counted but not executed: one launch that reads what it writes has no defined result, sequential or not.
THE QUEUE (test_queue_groups): cvgs.Queue.submit_many_on exposes the group behind ONE gate; the K1 u8c3 groups are submitted that way
(no hybrid policy, so nothing may fall back to launches): conflict groups come back CVGS_ERR_UNSUPPORTED with the "must be independent"
text and nothing of them has run, clear groups are served and leave the sequential result.  (Queue.submit_many is n separate submits in
one call -- batches of separate submits overlap by the queue's contract -- and is not a group.)

Families the node count covers -- each shown capturable as one node by a control group at disjoint placement (label "control"):
  k1_u8c3, k1_u8c4        K1, host descriptors (the planes travel in the fused launch's kernel arguments)
  tab_u8, tab_u16, tab_f32 K1, device plane tables, the hull stated by the facade (plus: nothing stated => one node per chain whatever
                          the placement; vouched => one node).  The host sees ONE range of such a chain, so a target in the gap between
                          two of its crops is grey for it, not clear (byte_model.read_spans)
  nv12, nv21, p010, yuyv, uyvy, i444   the K4 family, host descriptors
  pw_3d, pw_split, pw_splitT            the fused pointwise tick (READ_PIXEL u8 into packed 3-D, split, splitT)
Not covered: I420 / YV12 (host descriptors of planar-chroma ticks are staged in a table, which a capture refuses: such a tick is captured
chain by chain even at disjoint placement, so a node count says nothing about the decision); their ranges are held to the model by
tests/test_hull_vs_byte_model.py.  bf16 targets add no placement of their own and are left to tests/test_gpu_bf16.py.

Placements every family meets on purpose (DELIBERATE; the model's class of each is asserted, from the model alone):
  before_gap / before_abut / overlap_first   a target that ends 32 bytes before a view's first byte / exactly at it / inside it
  after_abut / last_row_remainder / overlap_last   a target that begins exactly behind a view's last byte / 16 bytes further, inside the unused
                          remainder of a bottom crop's last row (round 4's defect) / on its last bytes
  crop_gap                inside the gap between two crops of one frame
  chroma_rows             (4:2:0) inside the chroma rows of a crop, behind its luma rows
  u_plane, v_plane        (I444) inside the U and the V plane of a view
  splitT_ranges           two splitT chains writing different image ranges of ONE CNHW tensor
  splitT_reach            a splitT target with planes > batch whose last channel run reaches into another chain's source
  own_target              a chain reading its own target
  unstated, vouched       (device tables) nothing stated, and vouched
"Overlap" is by one source element -- ONE byte for the 8-bit layouts; the 16-bit, fp32 and packed 4:2:2 sources are aligned to their
element / pixel pair, and targets are kept 16-byte aligned, so the smallest overlap there is 2 / 4 bytes.
Shapes: frames of at most 97 x 61, targets of (24, 16) or (8, 4), batch 1-6, groups of 2-4 chains of one shape."""
import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import byte_model as B
from tests import helpers as H
from tests import yuv422_cases as Y422
from tests import yuv444_cases as Y444

SLOT = 1 << 17                      # one chain's part of the arena: its default target at +256, its frame at +64 Ki (+ a shift below 16)
FRAME_AT, TARGET_AT = 1 << 16, 256
MAX_CHAINS = 4
ARENA = MAX_CHAINS * SLOT
FILL_SEED = 0x1DE9
N_COUNT_SEEDS, N_RUN_SEEDS = 32, 8

FAMILIES = {
    "k1_u8c3": dict(kind="k1", cn=3, depth=cvgs.DEPTH_8U, align=1), "k1_u8c4": dict(kind="k1", cn=4, depth=cvgs.DEPTH_8U, align=1),
    "tab_u8": dict(kind="k1", cn=3, depth=cvgs.DEPTH_8U, align=1, table=True), "tab_u16": dict(kind="k1", cn=3, depth=cvgs.DEPTH_16U, align=2, table=True, fmax=(60, 40)),
    "tab_f32": dict(kind="k1", cn=3, depth=cvgs.DEPTH_32F, align=4, table=True, fmax=(40, 30)),
    "nv12": dict(kind="420", layout=capi.YUV_NV12, align=2), "nv21": dict(kind="420", layout=capi.YUV_NV21, align=2), "p010": dict(kind="420", layout=capi.YUV_P010, align=2),
    "yuyv": dict(kind="422", layout=capi.YUV_YUYV, align=4), "uyvy": dict(kind="422", layout=capi.YUV_UYVY, align=4),
    "i444": dict(kind="444", layout=capi.YUV_I444, align=1),
    "pw_3d": dict(kind="pw", cn=3, write="3d", align=1), "pw_split": dict(kind="pw", cn=3, write="split", align=1), "pw_splitT": dict(kind="pw", cn=3, write="splitT", align=1),
}
# (align: what the source's address must be a multiple of -- 4:2:0 surfaces are kept even so that crops' uv_offset stays even)


class Chain:
    """One chain's geometry, in arena offsets."""

    def __init__(self, slot, fw, fh, step, rects, used=None, uv=0, write="split", planes=0, table_mode=None):
        self.frame, self.target = slot * SLOT + FRAME_AT, slot * SLOT + TARGET_AT
        self.fw, self.fh, self.step, self.uv, self.rects = fw, fh, step, uv, list(rects)
        self.used = len(self.rects) if used is None else used
        self.write, self.planes, self.table_mode = write, planes, table_mode


class Group:
    def __init__(self, family, dst, chains, label):
        self.family, self.dst, self.chains, self.label = family, dst, chains, label
        self.runnable = True

    def out_cn(self):
        return FAMILIES[self.family].get("cn", 3)

    def target_bytes(self, c):
        n = max(c.planes, len(c.rects)) if c.write == "splitT" else len(c.rects)
        return self.out_cn() * n * self.dst[0] * self.dst[1] * 4


# ---- chains from geometry --------------------------------------------------------------------------------------------------------------------
def build(g, c, base, table=None):
    """The iop list of chain c with the arena at address `base` (the host buffer, the device tensor, or 0 for offsets)."""
    fam = FAMILIES[g.family]
    kind, (dw, dh), n = fam["kind"], g.dst, len(c.rects)
    cn = g.out_cn()
    f = cvgs.make_type(cvgs.DEPTH_32F, cn)
    out = cvgs.GpuMat(n, cn * dw * dh, cvgs.CV_32FC1, base + c.target)
    if kind == "k1":
        frame = cvgs.GpuMat(c.fh, c.fw, cvgs.make_type(fam["depth"], cn), base + c.frame, c.step)
        ops = H.k1_chain(frame, c.rects, out, g.dst, cn, used=c.used, src_depth=fam["depth"], table=table)
    elif kind == "pw":
        u = cvgs.make_type(cvgs.DEPTH_8U, cn)
        frame = cvgs.GpuMat(c.fh, c.fw, u, base + c.frame, c.step)
        ops = [cvgs.ReadIOp(capi.READ_PIXEL, u, [frame.roi(*r) for r in c.rects], c.used), cvgs.convertTo(u, f, 0.3), cvgs.subtract(f, H.K1_SUB[cn]), cvgs.divide(f, H.K1_DIV[cn])]
        ops.append(cvgs.write(f, cvgs.GpuMat(n, dw * dh, f, base + c.target), g.dst) if c.write == "3d" else cvgs.split(f, out, g.dst))
    else:
        layout = fam["layout"]
        if kind == "420":
            luma = cvgs.GpuMat(c.fh, c.fw, cvgs.CV_16UC1 if layout == capi.YUV_P010 else cvgs.CV_8UC1, base + c.frame, c.step)
            mats = [luma.nv12_roi(*r) for r in c.rects]
        elif kind == "422":
            mats = [cvgs.GpuMat(c.fh, c.fw, Y422.CV_8UC2, base + c.frame, c.step).yuv422_roi(*r) for r in c.rects]
        else:
            surf = cvgs.GpuMat(c.fh, c.fw, cvgs.CV_8UC1, base + c.frame, c.step)
            surf.uv_offset = c.uv
            mats = [surf.yuv444_roi(*r) for r in c.rects]
        ops = [cvgs.read_nv12(mats, g.dst, capi.YUV_LIMITED, capi.BT709, False, layout=layout), cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f),
               cvgs.multiply(f, [0.3] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.divide(f, H.K1_DIV[3]), cvgs.split(f, out, g.dst)]
    if c.write == "splitT":
        ops[-1] = cvgs.splitT(f, base + c.target, dw, dh, c.planes)
    return ops


def model_chains(g, base=0):
    """The chains as the model reads them (device-table chains carry a table mark: the host sees one hull of them)."""
    return [build(g, c, base, table=1 if c.table_mode else None) for c in g.chains]


def classify(g):
    return B.classify(model_chains(g))


def expected_nodes(g, cls):
    """Kernel nodes of the captured call, or None where either answer is allowed."""
    modes = {c.table_mode for c in g.chains}
    if "unstated" in modes:
        return len(g.chains)  # nothing stated, nothing vouched: the chains keep their sequential meaning, whatever the placement
    if modes == {"vouched"}:
        return 1 if cls == "clear" else None  # (the caller's word replaces the source check; only clear groups are vouched for here)
    return {"conflict": len(g.chains), "clear": 1, "grey": None}[cls]


# ---- the generator ---------------------------------------------------------------------------------------------------------------------------
def _frame(family, rng, slot, n_rects, dst, small=False, write=None, planes=0):
    """A random frame of the family in `slot`, with n_rects views."""
    fam = FAMILIES[family]
    kind = fam["kind"]
    wmax, hmax = fam.get("fmax", (97, 61))
    fw, fh = int(rng.integers(max(dst[0], 24), wmax + 1)), int(rng.integers(max(dst[1], 20), hmax + 1))
    if small:
        fw, fh = 64, 48
    even = kind in ("420", "422")
    if even:
        fw &= ~1
    if kind == "420":
        fh &= ~1
    px = {"k1": None, "pw": 3, "420": 2 if fam.get("layout") == capi.YUV_P010 else 1, "422": 2, "444": 1}[kind]
    if px is None:
        px = fam["cn"] * {cvgs.DEPTH_8U: 1, cvgs.DEPTH_16U: 2, cvgs.DEPTH_32F: 4}[fam["depth"]]
    a = fam["align"]
    pad = int(rng.choice([0, 1, 5, 13, 40])) if not small else 40
    step = (fw * px + pad + (4 if kind == "422" else a) - 1) // (4 if kind == "422" else a) * (4 if kind == "422" else a)
    rects = []
    for _ in range(n_rects):
        if kind == "pw":
            w, h = dst
        else:
            w, h = int(rng.integers(4, max(5, fw // 2))), int(rng.integers(4, max(5, fh // 2)))
        x, y = int(rng.integers(0, fw - w + 1)), int(rng.integers(0, fh - h + 1))
        if kind == "420":
            x, y, w, h = x & ~1, y & ~1, w & ~1, h & ~1
        if kind == "422":
            x &= ~1
        rects.append((x, y, w, h))
    uv = (fh - 1) * step + fw + int(rng.choice([0, 1, 77])) if kind == "444" else 0
    write = write or fam.get("write", "split")
    if write == "splitT" and not planes:
        planes = n_rects
    return Chain(slot, fw, fh, step, rects, uv=uv, write=write, planes=planes,
                 table_mode="stated" if fam.get("table") else None)


def _hull(g, i):
    """[first byte, last byte + 1) of everything chain i reads, and its views' spans, in arena offsets."""
    ch = build(g, g.chains[i], 0)
    spans = [B.span(B.view_reads(ch[0], m)) for m in B.views(ch)]
    return min(s[0] for s in spans), max(s[1] for s in spans), spans


def _pin(g, a, b, anchor, delta, at_end=False):
    """Move chain b's target so that its first byte (at_end: the byte behind its last) lies `delta` bytes from `anchor`, a byte of chain a's
    geometry; chain a's frame is shifted by less than 16 bytes (a multiple of its alignment) so that the target stays 16-byte aligned."""
    al = FAMILIES[g.family]["align"]
    assert delta % al == 0 and anchor % al == 0
    shift = (-(anchor + delta)) % 16
    assert shift % al == 0
    g.chains[a].frame += shift
    point = anchor + shift + delta
    g.chains[b].target = point - (g.target_bytes(g.chains[b]) if at_end else 0)
    assert g.chains[b].target % 16 == 0 and 0 <= g.chains[b].target and g.chains[b].target + g.target_bytes(g.chains[b]) <= ARENA


def random_group(family, seed):
    fam = FAMILIES[family]
    rng = np.random.default_rng([sorted(FAMILIES).index(family), seed])
    n = int(rng.integers(2, MAX_CHAINS + 1))
    dst = [(24, 16), (8, 4)][int(rng.integers(2))]
    write, planes = None, 0
    batches = [int(rng.integers(1, 7)) for _ in range(n)]
    if fam.get("write") == "splitT" or (fam["kind"] != "pw" and rng.integers(4) == 0):
        write, planes = "splitT", max(batches) + int(rng.integers(0, 3))
    chains = [_frame(family, rng, i, batches[i], dst, write=write, planes=planes) for i in range(n)]
    if fam["kind"] in ("k1", "pw"):
        for c in chains:
            if rng.integers(3) == 0:
                c.used = int(rng.integers(1, len(c.rects) + 1))
    g = Group(family, dst, chains, "seed %d" % seed)
    mode = ["disjoint", "disjoint", "hit", "hit", "alias", "near"][int(rng.integers(6))]
    a, b = [int(v) for v in rng.choice(n, 2, replace=False)]
    size = g.target_bytes(chains[b])
    lo, hi, spans = _hull(g, a)
    if mode == "hit":  # somewhere over chain a's frame: mostly on a view, sometimes in a gap or in row padding
        chains[b].target = int(rng.integers(max(256, lo - size + 16), hi)) // 16 * 16
    elif mode == "alias":  # on chain a's target
        chains[b].target = max(256, chains[a].target + int(rng.integers(-size // 16 + 1, g.target_bytes(chains[a]) // 16)) * 16)
    elif mode == "near":  # close to chain a's reads, in front of them or behind
        gap = int(rng.integers(0, 5)) * 16
        chains[b].target = (lo - size - gap) // 16 * 16 if rng.integers(2) else (hi + gap + 15) // 16 * 16
    chains[b].target = min(max(chains[b].target, 256), ARENA - size - 256)
    g.label += " " + mode
    # a chain that reads its own target is met on purpose only (own_target): it cannot be executed
    g.runnable = not any(B.intersects(B.reads(ch), B.writes(ch)) for ch in model_chains(g))
    return g


def _pair(family, label, write=None, planes=0):
    """The two-chain group the deliberate placements start from: chain A (index 0) reads a top and a bottom crop at the frame's left edge,
    chain B (index 1) is the one whose target is moved."""
    rng = np.random.default_rng([77, sorted(FAMILIES).index(family)])
    dst = (8, 4)
    chains = [_frame(family, rng, i, 2, dst, small=True, write=write, planes=planes) for i in range(2)]
    w, h = dst if FAMILIES[family]["kind"] == "pw" else (16, 8)
    chains[0].rects = [(0, 0, w, h), (0, chains[0].fh - h, w, h)]
    return Group(family, dst, chains, label)


def deliberate(family):
    """[(group, the classes the model may give it)] -- every placement of the module docstring that exists for the family."""
    fam = FAMILIES[family]
    kind, al = fam["kind"], fam["align"]
    out = []

    def case(label, want, **kw):
        g = _pair(family, label, **kw)
        out.append((g, want))
        return g

    case("control", ("clear",))
    for label, delta, at_end, want in (("before_gap", -32, True, "clear"), ("before_abut", 0, True, "clear"), ("overlap_first", al, True, "conflict")):
        g = case(label, (want,))
        _pin(g, 0, 1, _hull(g, 0)[0], delta, at_end)
    for label, delta, want in (("after_abut", 0, "clear"), ("last_row_remainder", 16, "clear"), ("overlap_last", -al, "conflict")):
        g = case(label, (want,))
        _pin(g, 0, 1, _hull(g, 0)[1], delta)
    g = case("crop_gap", ("clear", "grey"))  # grey where a view's span reaches over the gap (its chroma rows / planes lie behind it), or for a table's one hull
    _pin(g, 0, 1, g.chains[0].frame + 12 * g.chains[0].step, 0)
    if kind == "420":
        g = case("chroma_rows", ("conflict",))
        _pin(g, 0, 1, g.chains[0].frame + (g.chains[0].fh + 1) * g.chains[0].step, 0)  # chroma row 1 of the top crop, behind every luma row
    if kind == "444":
        for k, label in ((1, "u_plane"), (2, "v_plane")):
            g = case(label, ("conflict",))
            _pin(g, 0, 1, g.chains[0].frame + k * g.chains[0].uv + 2 * g.chains[0].step, 0)
    if fam.get("write", "splitT") == "splitT":  # (the pointwise families write one kind each)
        plane = 8 * 4 * 4
        g = case("splitT_ranges", ("grey",), write="splitT", planes=4)
        g.chains[1].target = g.chains[0].target + 2 * plane  # images 2-3 of the tensor whose images 0-1 chain A writes
        g = case("splitT_reach", ("conflict",), write="splitT", planes=8)
        _pin(g, 0, 1, _hull(g, 0)[0], -(2 * 8 * plane + 64))  # A's first byte lies 64 bytes inside B's LAST channel run, behind batch * cn planes
    g = case("own_target", ("conflict",))
    g.chains[0].target = (_hull(g, 0)[0] + 15) // 16 * 16
    g.runnable = False
    if fam.get("table"):
        for mode in ("unstated", "vouched"):
            g = case(mode, ("clear",))
            for c in g.chains:
                c.table_mode = mode
    for g, _ in out:
        for c in g.chains:
            assert 0 <= c.target and c.target + g.target_bytes(c) <= ARENA and c.frame + 3 * (c.uv or 0) + (c.fh * 3 // 2 + 1) * c.step <= ARENA
    return out


def all_groups(family, n_seeds):
    return [g for g, _ in deliberate(family)] + [random_group(family, s) for s in range(n_seeds)]


# ---- conditions on the generator: from the model alone, no product call (and no GPU) ----------------------------------------------------------
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_generator_conditions(family):
    wanted = {"control", "before_gap", "before_abut", "overlap_first", "after_abut", "last_row_remainder", "overlap_last", "crop_gap", "own_target"}
    kind = FAMILIES[family]["kind"]
    wanted |= {"chroma_rows"} if kind == "420" else set()
    wanted |= {"u_plane", "v_plane"} if kind == "444" else set()
    wanted |= {"splitT_ranges", "splitT_reach"} if FAMILIES[family].get("write", "splitT") == "splitT" else set()
    wanted |= {"unstated", "vouched"} if FAMILIES[family].get("table") else set()
    seen = {}
    for g, want in deliberate(family):
        seen[g.label] = classify(g)
        assert seen[g.label] in want, "%s %s: the model says %s" % (family, g.label, seen[g.label])
    assert set(seen) == wanted
    if kind in ("k1", "pw", "422") and not FAMILIES[family].get("table"):
        assert seen["crop_gap"] == "clear"  # view by view, the gap between two crops belongs to nobody
    classes = [classify(random_group(family, s)) for s in range(N_COUNT_SEEDS)]
    n = len(classes)
    assert 4 * classes.count("conflict") >= n and 4 * classes.count("clear") >= n and 4 * classes.count("grey") <= n, \
        "%s: %d conflict, %d clear, %d grey of %d" % (family, classes.count("conflict"), classes.count("clear"), classes.count("grey"), n)
    for s in range(N_COUNT_SEEDS):  # shapes: the smallest that still reach the fused kernels (module docstring)
        g = random_group(family, s)
        assert 2 <= len(g.chains) <= 4 and g.dst in ((24, 16), (8, 4)) and all(1 <= len(c.rects) <= 6 and c.fw <= 97 and c.fh <= 61 for c in g.chains)
    for g in all_groups(family, N_COUNT_SEEDS):  # every byte a group touches lies inside the arena, 64 bytes and more from its ends
        for ch in model_chains(g):
            for lo, hi in B.reads(ch) + B.writes(ch):
                assert 64 <= lo and hi <= ARENA - 64, (family, g.label)


# ---- the GPU side ----------------------------------------------------------------------------------------------------------------------------
def _initial(family):
    """The arena's fill: seeded bytes; finite fp32 values for the fp32 sources (whatever such a view reads is then a finite number)."""
    if FAMILIES[family].get("depth") == cvgs.DEPTH_32F:
        return (H.random_u8((ARENA // 4,), FILL_SEED).astype(np.float32) * np.float32(0.75)).view(np.uint8).copy()
    return H.random_u8((ARENA,), FILL_SEED)


class Rig:
    """The arena on both sides, built once per test."""

    def __init__(self, family, device):
        import torch
        self.family, self.torch = family, torch
        self.initial = _initial(family)
        raw = np.zeros(ARENA + 256, np.uint8)
        off = (-raw.ctypes.data) % 256
        self.host = raw[off:off + ARENA]  # 256-byte aligned like the device allocation: the two sides agree on every alignment
        self.dev = torch.zeros(ARENA, dtype=torch.uint8, device=device)
        self.init_dev = torch.from_numpy(self.initial).to(device)
        self.keep = []

    def reset(self):
        self.host[:] = self.initial
        self.dev.copy_(self.init_dev)
        self.torch.cuda.synchronize()

    def lowered(self, g):
        """The group's chains on the device arena, lowered (device tables built from the same views and uploaded)."""
        out = []
        for c in g.chains:
            ops = build(g, c, self.dev.data_ptr())
            if c.table_mode:
                tab = self.torch.frombuffer(bytearray(cvgs.build_plane_table(ops[0])), dtype=self.torch.uint8).to(self.dev.device)
                self.keep.append(tab)
                ops = build(g, c, self.dev.data_ptr(), table=tab.data_ptr())
                if c.table_mode == "unstated":
                    ops[0].mats = None  # no host views at hand: the facade states nothing
                elif c.table_mode == "vouched":
                    ops[0].mats, ops[0].table_vouched = None, True
            out.append(cvgs.lower(ops))
        return out

    def reference(self, g, oracle):
        """The same chains one after another on the host arena."""
        kind = FAMILIES[g.family]["kind"]
        base = self.host.ctypes.data
        for c in g.chains:
            ops = build(g, c, base)
            for m in ops[0].mats:
                m.owner = self.host
            if kind == "422":
                surf = np.lib.stride_tricks.as_strided(self.host[c.frame:], (c.fh, c.step // 2, 2), (c.step, 2, 1))  # the whole pitch: every crop lies inside
                Y422.Expect(oracle, [surf], FAMILIES[g.family]["layout"]).run(ops)
            elif kind == "444":
                Y444.Expect(oracle, [_Surf444(self.host, c)]).run(ops)
            else:
                oracle.execute(cvgs.lower(ops))

    def compare(self, g, what):
        got = self.dev.cpu().numpy()
        ref = self.host.copy()
        for ch in model_chains(g):  # targets are fp32: NaN payloads may differ, everything else must be the same bits
            for lo, hi in B.writes(ch):
                a, b = got[lo:hi].view(np.float32), ref[lo:hi].view(np.float32)
                an, bn = np.isnan(a), np.isnan(b)
                assert np.array_equal(an, bn), what
                a[an], b[bn] = 0, 0
        H.assert_bit_exact(got, ref, what)


class _Surf444:
    """What yuv444_cases.Expect reads of a surface, taken from the arena as it is NOW (an earlier chain of the group may have written into it)."""

    def __init__(self, arena, c):
        self.buf, self.origin, self.w, self.h, self.step, self.uv = arena, c.frame, c.fw, c.fh, c.step, c.uv
        idx = c.frame + (np.arange(3)[:, None, None] * c.uv + np.arange(c.fh)[None, :, None] * c.step + np.arange(c.fw)[None, None, :])
        self.planes = tuple(np.ascontiguousarray(p) for p in arena[idx])


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_node_counts(family, device, lib):
    from tests.test_gpu_many import _captured_kernel_nodes
    rig = Rig(family, device)
    rig.reset()
    seen = {"conflict": 0, "clear": 0, "grey": 0}
    for g in all_groups(family, N_COUNT_SEEDS):
        cls = classify(g)
        seen[cls] += 1
        low = rig.lowered(g)
        nodes = _captured_kernel_nodes(lib, cvgs.pack_chains(low), len(low), device)
        print("%s %-28s %-8s %d chains -> %d nodes" % (family, g.label, cls, len(low), nodes))
        want = expected_nodes(g, cls)
        if g.label == "control":
            assert nodes == 1, "%s: the control group at disjoint placement does not capture as ONE node (%d): the family's tick is not capturable" % (family, nodes)
        if want is not None:
            assert nodes == want, "%s, %s: the model says %s, the call enqueued %d kernels for %d chains" % (family, g.label, cls, nodes, len(low))
    assert min(seen["conflict"], seen["clear"]) > 0
    assert (rig.dev.cpu().numpy() == rig.initial).all(), "a captured call ran"


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_sequential_meaning(family, device, lib, oracle):
    import torch
    rig = Rig(family, device)
    ran = 0
    for g in all_groups(family, N_RUN_SEEDS):
        if not g.runnable:
            continue
        rig.reset()
        low = rig.lowered(g)
        capi.check(lib.cvgs_execute_many(cvgs.pack_chains(low), len(low), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        rig.reference(g, oracle)
        rig.compare(g, "%s, %s (%s)" % (family, g.label, classify(g)))
        ran += 1
    assert ran >= N_RUN_SEEDS


@pytest.mark.gpu
def test_queue_groups(device, lib, oracle):
    """cvgs.Queue.submit_many_on: ONE gate for the group.  Conflict groups are refused whole, clear groups are served."""
    import torch
    family = "k1_u8c3"
    rig = Rig(family, device)
    q = cvgs.Queue(idle_us=5000.0)
    side = torch.cuda.Stream()
    refused = served = submitted = 0
    try:
        for g in all_groups(family, N_RUN_SEEDS):
            cls = classify(g)
            if cls == "grey":
                continue
            rig.reset()
            low = rig.lowered(g)
            ptrs = cvgs.Queue.chain_pointers(low)
            print("queue %-28s %s" % (g.label, cls))
            if cls == "conflict":
                with pytest.raises(capi.CvgsError) as e:
                    q.submit_many_on(side, ptrs, len(low), cvgs.Queue.MIN_GROUP(2))
                assert e.value.code == capi.ERR_UNSUPPORTED and "must be independent" in str(e.value), "%s: %s" % (g.label, e.value)
                torch.cuda.synchronize()
                assert (rig.dev.cpu().numpy() == rig.initial).all(), "%s: something of a refused group ran" % g.label
                assert q.stats()["submitted"] == submitted
                refused += 1
            else:
                t = q.submit_many_on(side, ptrs, len(low), cvgs.Queue.MIN_GROUP(2))  # (not deferred: the stream is held until the group is complete)
                side.synchronize()
                submitted += len(low)
                assert t != cvgs.Queue.TICKET_DIRECT and q.stats()["submitted"] == submitted
                rig.reference(g, oracle)
                rig.compare(g, "queue group, %s" % g.label)
                served += 1
        assert q.stats()["error"] == 0
    finally:
        q.destroy()
    assert refused >= 4 and served >= 4
