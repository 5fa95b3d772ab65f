"""The grid of tests/colour_cases.py without a GPU: every chain is one the product accepts, the dry run names the kernel the case expects (the
compile-time colour kernels of k_cvtcolor_u8.hip by default, an interpreted kernel under CHAIN_NO_THREAD_FUSION / CHAIN_FORCE_GENERIC and for
every ineligible neighbour), the grid holds what its docstring says -- asserted from the built chains, not from the cases' names --, and the CPU
oracle lies within the float64 model's bound (tests/f64_model.py) on every case it can run: channel permutations bit for bit, gray within
Result.check's own bound.  Two mutants of the model show that it is a real check.

Largest |oracle - model| / tolerance per family (1 = at the bound): permutations 0 (exact) at every depth; gray 0.50 on CV_8U and CV_16U (the
integer outputs' half step), 0.65 on CV_32F."""
import ctypes as C

import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import colour_cases as K
from tests import model_cases as MC

# What the grid must hold, restated here as literals (NOT taken from tests/colour_cases.py): deleting a width, a height, a layout, a gray order, an
# alpha or an ineligibility reason from the grid -- from its constants and its cases alike -- fails test_the_grid_covers_what_it_says.
WIDTHS = {K.U8: {16, 1008, 1024, 1040, 2064}, K.U16: {16, 1008, 1024, 1040, 2064}, K.F32: {4, 252, 256, 260, 516}}
HEIGHTS = {1, 3, 4, 5, 9}
NEIGHBOUR_BASE_WIDTH = {K.U8: 1040, K.U16: 1040, K.F32: 260}
GRAY_ORDERS = {((1, 0, 2), 3), ((0, 0, 0), 3), ((2, 0, 1), 3), ((3, 1, 0), 4), ((1, 2, 3), 4)}  # ((R, G, B) channel indices, channels in)
LAYOUTS = {"src_pitch": (True, False), "out_pitch": (False, True), "both_pitch": (True, True)}  # (source view pitched, output view pitched)
BATCHES = {"batch1": 1, "batch2": 2, "batch3": 3}
REASONS = {"width+1", "width-3", "src_base+4", "src_base+8", "src_step%16=8", "out_base+8", "out_pitch%16=8", "used<batch", "device_table"}
ALPHAS = {K.U8: {7.0, 0.0}, K.U16: {float(0x1234), float(0x00FF)}}
ALPHA_BITS_F32 = {0x80000000, int(np.float32(3.0e38).view(np.uint32)), 0x00000123}  # -0.0, 3.0e38, a subnormal
BAD_ALPHAS = {K.U8: {255.5, 300.0, -1.0, 65536.0}, K.U16: {255.5, -1.0, 65536.0}}  # (300 is a CV_16U value: that chain is eligible)
FAST = {(K.U8, "permute"): "pointwise16_u8_permute", (K.U8, "gray"): "pointwise16_u8_gray", (K.U16, "permute"): "pointwise16_u16_permute",
        (K.U16, "gray"): "pointwise16_u16_gray", (K.F32, "permute"): "pointwise4_f32_permute", (K.F32, "gray"): "pointwise4_f32_gray"}

_BUILT = {}


def built(name):
    """(backend, iops, views) of a case over host memory, built once"""
    if name not in _BUILT:
        B = MC.HostBackend()
        iops, views = K.CASES[name].build(B)
        _BUILT[name] = (B, iops, views)
    return _BUILT[name]


def facts(name):
    """what the eligibility predicate looks at, read from the built chain"""
    B, iops, _ = built(name)
    rd, st, wr = iops
    c = K.CASES[name]
    es = K.ES[c.depth]
    w, h = rd.mats[0].cols, rd.mats[0].rows
    ocn = capi.type_cn(wr.dst_type)
    pitch = wr.step if wr.kind == capi.WRITE_PIXEL_2D else w * ocn * es
    op, aux, operand = st.ops[0]
    lane = 16 if c.depth != K.F32 else 4
    return dict(w=w, h=h, batch=rd.batch, used=rd.used_planes, table=rd.table is not None, lane=lane, row=w * c.cn * es, orow=w * ocn * es, pitch=pitch,
                src_base=[m.data % 16 for m in rd.mats], src_step=[m.step for m in rd.mats], out_base=wr.data % 16, op=op, aux=aux, operand=operand,
                image_bytes=max(h * w * max(c.cn, ocn) * es, 1), write_kind=wr.kind)


def violated(name):
    """the reasons (colour_cases.REASONS and the operand ones) for which the chain of a case is not eligible"""
    f, c = facts(name), K.CASES[name]
    out = set()
    if f["w"] % f["lane"]:
        out.add("width")
    if any(b == 4 for b in f["src_base"]):
        out.add("src_base+4")
    if any(b == 8 for b in f["src_base"]):
        out.add("src_base+8")
    assert all(b in (0, 4, 8) for b in f["src_base"]) and f["out_base"] in (0, 8)
    if any(s % 16 for s in f["src_step"]):
        assert all(s % 16 == 8 for s in f["src_step"])
        out.add("src_step%16=8")
    if f["out_base"]:
        out.add("out_base+8")
    if f["pitch"] % 16:
        assert f["pitch"] % 16 == 8
        out.add("out_pitch%16=8")
    if f["used"] != f["batch"]:
        assert f["used"] == f["batch"] - 1
        out.add("used<batch")
    if f["table"]:
        out.add("device_table")
    if f["op"] in (capi.OP_ADD_ALPHA, capi.OP_DROP_ALPHA) and f["aux"] & 63 not in (K.ID3, K.SWAP3):
        out.add("selector")
    if f["op"] == capi.OP_GRAY and c.depth == K.F32 and f["aux"] & 63 not in (K.ID3, K.SWAP3):
        out.add("gray_order")
    if f["op"] == capi.OP_ADD_ALPHA and c.depth != K.F32:
        a = f["operand"][0]
        if not (0 <= a <= (255 if c.depth == K.U8 else 65535)) or a != int(a):
            out.add("alpha")
    return out


def reason_found(name):
    """the ineligibility reason of a case as the built chain shows it (None: eligible), the two width neighbours told apart by the width itself"""
    v = violated(name)
    assert len(v) <= 1, (name, v)
    if v == {"width"}:
        w, base = facts(name)["w"], NEIGHBOUR_BASE_WIDTH[K.CASES[name].depth]
        assert w in (base + 1, base - 3), (name, w)
        return "width+1" if w == base + 1 else "width-3"
    return next(iter(v), None)


def test_every_chain_validates_and_names_its_kernel(lib):
    for c in K.CASES.values():
        _, iops, _ = built(c.name)
        assert lib.cvgs_validate(C.byref(cvgs.lower(iops).desc)) == 0, c.name
        assert cvgs.kernel_name(*iops) == c.kernel, (c.name, cvgs.kernel_name(*iops))
        assert c.kernel.startswith(K.FAST_PREFIXES) == (c.reason is None), c.name
        for what, flags in K.FLAGS[1:]:
            got = cvgs.kernel_name(*iops, flags=flags)
            assert got == c.generic and not got.startswith(K.FAST_PREFIXES), (c.name, what, got)


def test_every_neighbour_differs_from_an_eligible_chain_in_one_thing():
    for c in K.CASES.values():
        want = set() if c.reason is None else {"width" if c.reason.startswith("width") else c.reason}
        assert violated(c.name) == want, (c.name, violated(c.name))
    for d in K.DEPTHS:  # the width neighbours: one more pixel, three fewer
        for t in ("permute", "gray"):
            ws = {c.reason: facts(c.name)["w"] for c in K.CASES.values() if c.depth == d and c.template == t and c.reason in ("width+1", "width-3")}
            base = NEIGHBOUR_BASE_WIDTH[d]
            assert ws == {"width+1": base + 1, "width-3": base - 3}, (d, t, ws)


def test_the_grid_covers_what_it_says():
    assert len(K.CASES) <= 250
    for c in K.CASES.values():
        f = facts(c.name)
        assert f["image_bytes"] < 100 * 1000 and (f["w"], f["h"]) == (c.w, c.h), c.name
    assert K.FAST == FAST
    for (d, t), kernel in FAST.items():
        mine = [c for c in K.CASES.values() if c.kernel == kernel]
        assert all(c.depth == d and c.template == t and c.reason is None for c in mine)
        assert {facts(c.name)["w"] for c in mine} == WIDTHS[d], kernel           # every width and every height on every fast kernel
        assert {facts(c.name)["h"] for c in mine} == HEIGHTS, kernel
        dense = [c for c in mine if c.layout == "dense"]                                   # ... and dense
        assert {facts(c.name)["w"] for c in dense} == WIDTHS[d] and {facts(c.name)["h"] for c in dense} == HEIGHTS, kernel
        for c in dense:
            f = facts(c.name)
            assert f["src_step"] == [f["row"]] and f["pitch"] == f["orow"] and f["write_kind"] == capi.WRITE_PIXEL_2D, c.name
        # the pitched layouts, on each template: a source view at a 16-byte-aligned x offset with a step beyond its row, an output view likewise
        for layout in list(LAYOUTS) + list(BATCHES):
            cs = [c for c in mine if c.layout == layout]
            assert cs, (kernel, layout)
            for c in cs:
                B, iops, _ = built(c.name)
                f = facts(c.name)
                src_pitched = all(s > f["row"] and s % 16 == 0 for s in f["src_step"]) and all(m.data % 256 >= 16 for m in iops[0].mats)
                out_pitched = f["pitch"] > f["orow"] and f["pitch"] % 16 == 0 and iops[2].data % 256 >= 16
                if layout in LAYOUTS:
                    assert (src_pitched, out_pitched) == LAYOUTS[layout], c.name
                    assert f["batch"] == 1 and f["write_kind"] == capi.WRITE_PIXEL_2D
                else:
                    assert f["batch"] == BATCHES[layout] and f["write_kind"] == capi.WRITE_PIXEL_3D and not f["table"], c.name
        codes = {built(c.name)[1][1].ops[0][:2] + (c.cn,) for c in mine}  # every cvtColor code of the template
        if t == "permute":
            want = {(capi.OP_REORDER, K.SWAP3, 3), (capi.OP_REORDER, K.SWAP3 | (3 << 6), 4)}
            want |= {(op, aux, cn) for op, cn in ((capi.OP_ADD_ALPHA, 3), (capi.OP_DROP_ALPHA, 4)) for aux in (K.ID3, K.SWAP3)}
        else:
            want = {(capi.OP_GRAY, aux, cn) for aux in (K.ID3, K.SWAP3) for cn in (3, 4)}
        assert codes >= want, (kernel, want - codes)
    for d in K.DEPTHS:
        n = K.DN[d]
        for t in ("permute", "gray"):
            reasons = {reason_found(c.name) for c in K.CASES.values() if c.depth == d and c.template == t}
            assert reasons >= REASONS, (n, t, REASONS - reasons)
        reasons = {reason_found(c.name) for c in K.CASES.values() if c.depth == d}
        assert "selector" in reasons and ("alpha" in reasons) == (d != K.F32) and ("gray_order" in reasons) == (d == K.F32), n
        sel = {built(c.name)[1][1].ops[0][0] for c in K.CASES.values() if c.depth == d and reason_found(c.name) == "selector"}
        assert sel == {capi.OP_ADD_ALPHA, capi.OP_DROP_ALPHA}, n
        grays = [c for c in K.CASES.values() if c.depth == d and facts(c.name)["op"] == capi.OP_GRAY and facts(c.name)["aux"] & 63 not in (K.ID3, K.SWAP3)]
        orders = {(tuple((facts(c.name)["aux"] >> (2 * k)) & 3 for k in range(3)), c.cn) for c in grays}
        assert orders == GRAY_ORDERS and all(c.gray_order is not None for c in grays), n
        for c in K.CASES.values():
            if c.depth == d and c.gray_order is not None:
                assert facts(c.name)["aux"] == K.gray_aux(c.gray_order)
                assert c.kernel == (K.FAST[(d, "gray")] if d != K.F32 else K.FALLBACK[d]), c.name  # (launch_gray's ORD == 0; launch_f32_colour4's mode < 0)
        alphas = {facts(c.name)["operand"][0] for c in K.CASES.values() if c.depth == d and c.reason is None and facts(c.name)["op"] == capi.OP_ADD_ALPHA}
        bad = {facts(c.name)["operand"][0] for c in K.CASES.values() if c.depth == d and reason_found(c.name) == "alpha"}
        if d == K.F32:
            assert {int(np.float32(a).view(np.uint32)) for a in alphas} >= ALPHA_BITS_F32 and not bad
        else:
            assert alphas >= ALPHAS[d] and bad == BAD_ALPHAS[d], n
    # sources hold what the fill rules ask for
    for c in K.CASES.values():
        a = built(c.name)[2][0].arr
        assert a.std() > 0 or not np.isfinite(a).all(), c.name
        if c.depth == K.U16:
            assert (a == 65535).any() and ((a >> 8) != (a & 255)).any(), c.name
        if c.depth == K.F32:
            special = np.isnan(a).any() and np.isinf(a).any() and (np.signbit(a) & (a == 0)).any() and (a == np.float32(3.0e38)).any()
            assert special == c.pure and (c.pure or np.isfinite(a).all()), c.name


def _oracle_run(oracle, c):
    B = MC.HostBackend()
    iops, views = c.build(B)
    oracle.execute(cvgs.lower(iops))
    got, moved = K.split_output(B.placed, B.result())
    assert moved.size == 0, "%s: the oracle wrote %d padding bytes" % (c.name, moved.size)
    return iops, views, got


@pytest.mark.parametrize("depth,template", K.FAMILIES, ids=[K.family_name(*f).replace(" ", "_") for f in K.FAMILIES])
def test_oracle_within_the_model_bound(oracle, depth, template):
    failed, worst, ran = [], 0.0, 0
    for c in K.CASES.values():
        if (c.depth, c.template) != (depth, template) or not c.oracle:
            continue
        iops, views, got = _oracle_run(oracle, c)
        ok, ratio, text = K.compare(c, K.model_of(c, iops, views), got)
        worst, ran = max(worst, ratio), ran + 1
        if not ok:
            failed.append("%s: %s" % (c.name, text))
    print("RATIO oracle %-12s %-40s %.4f" % (K.family_name(depth, template), "%d cases" % ran, worst))
    assert ran >= 20 and not failed, "%d of %d cases:\n%s" % (len(failed), ran, "\n".join(failed))


def _mutated(iops, aux=None, operand=None):
    op, a, o = iops[1].ops[0]
    return [iops[0], cvgs.PointwiseIOp(iops[1].in_type, iops[1].out_type, [(op, a if aux is None else aux(a), o if operand is None else operand(o))]), iops[2]]


def _exchange_r_b(aux):
    return (aux & ~0x33) | ((aux & 3) << 4) | ((aux >> 4) & 3)


@pytest.mark.parametrize("depth", K.DEPTHS, ids=[K.DN[d] for d in K.DEPTHS])
def test_a_model_with_r_and_b_exchanged_rejects_the_oracle(oracle, depth):
    """the model is a real check: `aux` with the first and the third selector exchanged throws cases of each depth and template outside the bound"""
    for template in ("permute", "gray"):
        caught = 0
        for c in K.cases_of(depth, template, True)[:8]:
            iops, views, got = _oracle_run(oracle, c)
            ok, _, _ = K.compare(c, K.model_of(c, _mutated(iops, aux=_exchange_r_b), views), got)
            caught += not ok
        assert caught >= 1, (K.DN[depth], template)


def test_a_model_with_the_alpha_bytes_swapped_rejects_the_oracle(oracle):
    """a CV_16U alpha with its two bytes exchanged (0x1234 -> 0x3412, 0x00FF -> 0xFF00): every such case falls outside; 65535 could not show it"""
    def swapped(o):
        return [float(((int(v) & 255) << 8) | (int(v) >> 8)) for v in o]
    cs = [c for c in K.CASES.values() if c.depth == K.U16 and c.reason is None and facts(c.name)["op"] == capi.OP_ADD_ALPHA]
    caught = {}
    for c in cs:
        iops, views, got = _oracle_run(oracle, c)
        caught[facts(c.name)["operand"][0]] = not K.compare(c, K.model_of(c, _mutated(iops, operand=swapped), views), got)[0]
    assert caught[float(0x1234)] and caught[float(0x00FF)] and not caught[65535.0], caught
