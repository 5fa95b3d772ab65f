"""The case grid of the ring model (tests/ring_model.py), shared by tests/test_ring_model_vs_oracle.py (CPU oracle) and
tests/test_gpu_circular_model.py (kernels).  A covering grid, not a full product: every case names the kernel instantiation or the branch
of cvgs_circular_update it is there for, and assert_preconditions() re-derives from the launch geometry of k_circular.hip that the shape
really reaches it (blocks = ceil(n / (256 * UNROLL)) capped at 8192 / jobs, stride = blocks * 256: the unrolled main loop AND the tail
loop of a copy kernel are both live in one launch iff (UNROLL - 1) * stride < n < UNROLL * stride).  Re-derive when that geometry changes.

Frames are seeded random u8 and distinct per update, so a wrong slot lands far outside any bound."""
import collections
import math

from cvgpuspeedup_amd import capi, cvgs
from tests import f64_model as F
from tests import helpers as H
from tests import ring_model as R

Case = collections.namedtuple("Case", "name handle mirrored order layout depth cn batch w h push")
# handle: "def" (default) | "dev" (CVGS_CIRCULAR_CAPTURABLE);  order: "nf" | "of";  layout: "std" | "tr" | "pk"
# depth: "32f" | "16f" | "16bf" | "8u" | "64f";  push: "px_msd" | "px_cast" | "px_mad" (per-pixel u8 pushes, one per program class) | "rs"
DEPTHS = {"32f": cvgs.CV_32F, "16f": cvgs.CV_16F, "16bf": capi.DEPTH_16BF, "8u": cvgs.CV_8U, "64f": cvgs.CV_64F}
ELEM_BYTES = {"32f": 4, "16f": 2, "16bf": 2, "8u": 1, "64f": 8}
RESIZE_SRC = (53, 31)  # (width, height) of the frames a resize push reads
MAX_COPY_JOBS = 64  # kMaxCopyJobs (cvgs_device.h): launch_circular_push declines more, launch_plane_copies takes them in chunks of it
MUL, SUB, DIV, ADD = [0.3, 0.31, 0.29, 0.5], [0.4, 0.45, 0.5, 0.1], [0.25, 0.22, 0.23, 0.2], [3.25, 1.5, 0.75, 2.0]


def pixel_type(case, twin=False):
    """the type of one pixel of a pushed frame (cn channels); twin: the fp32 twin of a CV_16BF case for the oracle, which has no bfloat16"""
    if case.depth == "16bf":
        return cvgs.make_type(cvgs.CV_32F, case.cn) if twin else cvgs.make_type(cvgs.CV_16F, case.cn) | capi.TYPE_FLAG_BF16
    return cvgs.make_type(DEPTHS[case.depth], case.cn)


def elem_type(case, twin=False):
    """the handle's element type: the pixel type for packed tensors, its one-channel type for planar ones"""
    t = pixel_type(case, twin)
    return t if case.layout == "pk" else (t & ~(63 << 3))


def color_planes(case):
    return 1 if case.layout == "pk" else case.cn


def plane_bytes(case):
    return ELEM_BYTES[case.depth] * (case.cn if case.layout == "pk" else 1) * case.w * case.h


def order_of(case):
    return cvgs.NewestFirst if case.order == "nf" else cvgs.OldestFirst


def mode_of(case):
    return cvgs.Transposed if case.layout == "tr" else cvgs.Standard


def write_kind(case):
    return {"std": capi.WRITE_TENSOR_SPLIT, "tr": capi.WRITE_TENSOR_T_SPLIT, "pk": capi.WRITE_PIXEL_3D}[case.layout]


def frame_shape(case):
    return (RESIZE_SRC[1], RESIZE_SRC[0], case.cn) if case.push == "rs" else (case.h, case.w, case.cn)


def frame(case, i):
    """the u8 frame of update i (seeded by the case's name: distinct per update and per case)"""
    seed = 1 + sum(ord(ch) * (k + 1) for k, ch in enumerate(case.name)) % 100_000
    return H.random_u8(frame_shape(case), seed=seed * 64 + i)


def chain(case, mat, write, twin=False):
    """the push chain over `mat` (device or host memory); twin: without the final conversion to bfloat16 (rounded by the caller)"""
    cn = case.cn
    u, f = cvgs.make_type(cvgs.CV_8U, cn), cvgs.make_type(cvgs.CV_32F, cn)
    if case.push == "rs":
        ops = [cvgs.resize(u, cvgs.INTER_LINEAR, mat, (case.w, case.h))]
    else:
        ops = [cvgs.ReadIOp(capi.READ_PIXEL, u, [mat], 1), cvgs.convertTo(u, f)]
    if case.push == "px_msd":
        ops += [cvgs.multiply(f, MUL[:cn]), cvgs.subtract(f, SUB[:cn]), cvgs.divide(f, DIV[:cn])]
    elif case.push != "px_cast":
        ops += [cvgs.multiply(f, MUL[:cn]), cvgs.add(f, ADD[:cn])]
    if case.depth != "32f" and not (twin and case.depth == "16bf"):
        ops.append(cvgs.convertTo(f, pixel_type(case)))
    return ops + [write]


def host_write(case, twin=False):
    return cvgs.WriteIOp(write_kind(case), pixel_type(case, twin), 16, case.w, case.h, 0, case.batch)


def model_frame(case, i):
    """f64_model's answer for the frame of update i: value and derived bound of every element, [1][H][W][C]"""
    a = frame(case, i)
    return F.evaluate(chain(case, cvgs.GpuMat.from_array(a, cvgs.make_type(cvgs.CV_8U, case.cn)), host_write(case)), [F.View(a)])


def ring(case):
    return R.Ring(case.batch, R.NEWEST_FIRST if case.order == "nf" else R.OLDEST_FIRST, case.layout, F.depth_of(pixel_type(case)), case.cn,
                  case.w, case.h)


# ---- which route an update takes, restated from cvgs_circular_update / launch_circular_push -------------------------------------------------
def route(case):
    """"push": the single-launch k_circular_push (DEV = capturable);  "stage": chain -> staging image, then k_circular_dev;
    "chain+copy": chain kernel, then k_plane_copy;  "chain": the chain kernel alone (default mirrored rings, BATCH 1)."""
    jobs = 0 if case.mirrored else (case.batch - 1) * color_planes(case)  # the copy jobs a push launch would carry
    push_ok = case.push != "rs" and case.depth in ("32f", "16f", "16bf") and plane_bytes(case) % 16 == 0 and jobs <= MAX_COPY_JOBS
    if case.handle == "dev":
        return "push" if push_ok else "stage"
    if case.mirrored or case.batch == 1:
        return "chain"
    return "push" if push_ok else "chain+copy"


def copy_jobs(case):
    cp, r = color_planes(case), route(case)
    if r == "stage":
        return 2 * cp if case.mirrored else (case.batch + 1) * cp
    if r == "chain":
        return 0
    return 0 if case.mirrored else (case.batch - 1) * cp


def copy_geometry(case):
    """(bytes per access, UNROLL, n accesses per plane, stride) of the copy part of the case's route"""
    pb, jobs = plane_bytes(case), copy_jobs(case)
    vec, unroll = (16, 8) if pb % 16 == 0 else ((4, 4) if pb % 4 == 0 else (1, 4))
    n = pb // vec
    blocks = max(1, min(math.ceil(n / (256 * unroll)), max(8192 // jobs, 1) if jobs else 1))
    return vec, unroll, n, blocks * 256


def main_and_tail_live(case):
    vec, unroll, n, stride = copy_geometry(case)
    return (unroll - 1) * stride < n < unroll * stride


def assert_preconditions(case):
    """what the case's NAME claims, derived from its shape"""
    tags = case.name.split("_")
    r = route(case)
    vec = copy_geometry(case)[0]
    assert (case.handle == "dev") == ("dev" in tags) and (case.handle == "def") == ("def" in tags), case
    assert not (case.mirrored and case.layout == "tr"), "mirrored rings exist in the Standard plane order only"
    for width in (16, 4, 1):
        if "copy%d" % width in tags:
            assert r in ("stage", "chain+copy") and copy_jobs(case) > 0 and vec == width, (case, r, vec)
            assert main_and_tail_live(case) or "tail" in tags, (case, copy_geometry(case))
    if "pushcopy16" in tags:
        assert r == "push" and vec == 16 and copy_jobs(case) > 0 and main_and_tail_live(case), (case, r, copy_geometry(case))
    if "push" in tags:
        assert r == "push" and plane_bytes(case) % 16 == 0, (case, r)
    for tag in ("stage", "chain"):
        if tag in tags:
            assert r == tag, (case, r)
    if "copy" in tags:
        assert r == "chain+copy", (case, r)
    if "packed" in tags:
        assert case.layout == "pk"


# ---- the grid -------------------------------------------------------------------------------------------------------------------------------
CASES = collections.OrderedDict()


def add(prefix, handle, mirrored, order, layout, depth, cn, batch, w, h, push):
    """{h}: the handle kind;  {r}: the route the update takes (push | stage | copy | chain), which assert_preconditions() holds the name to"""
    r = route(Case("", handle, mirrored, order, layout, depth, cn, batch, w, h, push))
    prefix = prefix.replace("{h}", handle).replace("{r}", "copy" if r == "chain+copy" else r)
    name = "%s_%s_%s_%s_%sc%d_b%d_%dx%d_%s" % (prefix, "mir" if mirrored else "ring", order, layout, depth, cn, batch, w, h, push)
    assert name not in CASES, name
    CASES[name] = Case(name, handle, mirrored, order, layout, depth, cn, batch, w, h, push)


for _h in ("def", "dev"):
    # every copy width, main and tail loops both live in one launch (k_plane_copy / the copy part of k_circular_push on default handles,
    # k_circular_dev / k_circular_push<DEV> on capturable ones)
    add("{h}_pushcopy16", _h, False, "nf", "std", "32f", 3, 3, 100, 80, "px_mad")     # n_vec 2000: lanes 0-207 unrolled, the rest in the tail
    add("{h}_copy16", _h, False, "of", "std", "32f", 3, 3, 100, 80, "rs")
    add("{h}_copy4", _h, False, "nf", "std", "32f", 3, 3, 37, 23, "px_mad")           # 3404 bytes, n = 851
    add("{h}_copy1", _h, False, "of", "std", "16f", 3, 3, 37, 23, "px_mad")           # 1702 bytes
    add("{h}_copy1", _h, False, "nf", "std", "16bf", 3, 3, 37, 23, "px_msd")
    add("{h}_copy1", _h, False, "of", "std", "8u", 3, 3, 37, 23, "px_mad")            # 851 bytes
    add("{h}_copy16_tail", _h, False, "nf", "std", "32f", 3, 3, 40, 24, "rs")         # the aligned small shape: n_vec 240, tail loop only
    # a resize push and 64F elements, each on an odd-sized and on an aligned plane (capturable: both force stage-then-shift)
    add("{h}_copy4_resize_odd", _h, False, "of", "std", "32f", 3, 3, 37, 23, "rs")
    add("{h}_copy4_e64_odd", _h, False, "nf", "std", "64f", 3, 3, 37, 23, "px_mad")   # 6808 bytes: 16 does not divide it, n = 1702
    add("{h}_copy16_tail_e64", _h, False, "of", "std", "64f", 3, 3, 40, 24, "px_mad")
    # the single-launch push: cn 1-4 with planar and with packed writes, each program class with fp32, fp16 and bf16 elements
    for _k, (_cn, _lay, _prog, _d) in enumerate([(1, "std", "px_msd", "16f"), (2, "std", "px_cast", "16f"), (3, "std", "px_mad", "16bf"), (4, "std", "px_msd", "32f"),
                                                 (1, "pk", "px_cast", "16bf"), (2, "pk", "px_mad", "32f"), (3, "pk", "px_msd", "16bf"), (4, "pk", "px_cast", "32f"),
                                                 (3, "std", "px_mad", "16f")]):
        add(("packed_push_{h}_c%d" if _lay == "pk" else "push_{h}_c%d") % _cn, _h, False, "nf" if _k % 2 else "of", _lay, _d, _cn, 3, 40, 24, _prog)
    # ring depth 1, 2, 5 on plain and mirrored rings, by a per-pixel push and by a resize push (capturable: push route and stage route, the
    # latter with its 2 * CP mirrored jobs and its job >= B * CP history jobs)
    for _b in (1, 2, 5):
        for _m in (False, True):
            add("depth_{r}_{h}", _h, _m, "nf" if _b != 2 else "of", "std", "32f", 3, _b, 40, 24, "px_msd")
            add("depth_{r}_{h}", _h, _m, "of" if _b != 2 else "nf", "std", "32f", 3, _b, 40, 24, "rs")
    # Transposed tensors (plain rings only), both orders
    for _o in ("nf", "of"):
        add("transposed_{r}_{h}", _h, False, _o, "tr", "32f", 3, 3, 40, 24, "px_msd")
        add("transposed_{r}_{h}", _h, False, _o, "tr", "16f", 2, 3, 37, 23, "rs")
    # packed tensors on the mirrored ring, and a packed odd-sized u8 tensor on the plain ring
    add("packed_{r}_{h}", _h, True, "of", "pk", "32f", 3, 3, 40, 24, "px_mad")
    add("packed_{r}_{h}", _h, True, "nf", "pk", "16f", 4, 2, 37, 23, "rs")
    add("packed_{h}_copy1", _h, False, "nf", "pk", "8u", 3, 3, 37, 23, "rs")          # 2553 bytes
    # either side of the push launch's 64 copy jobs, by a per-pixel push that is eligible in every other respect: BATCH 22 = 63 jobs (push),
    # BATCH 23 = 66 (capturable: stage-then-shift; default: the chain kernel, then copy launches of 64 + 2 jobs)
    add("jobs63_{r}_{h}", _h, False, "nf", "std", "32f", 3, 22, 40, 24, "px_msd")
    add("jobs66_{r}_{h}", _h, False, "of", "std", "32f", 3, 23, 40, 24, "px_msd")

BESIDE_THE_JOB_LIMIT = [n for n in CASES if n.startswith("jobs6")]  # on the GPU: subtests of one item (tests/test_gpu_circular_model.py)
assert len(CASES) <= 80 and len(BESIDE_THE_JOB_LIMIT) == 4, len(CASES)
