"""GPU parity for the bfloat16 hand-off tensors (CV_16BF): every output bit-exact against the CPU oracle's fp32 TWIN (the same chain
with the final CV_16BF replaced by CV_32F), rounded on the host to nearest even (tests/test_bf16_types.py: rne_bf16, pinned against
torch).  The oracle knows nothing of bf16: a bf16 SOURCE is widened exactly on the host and handed to it as fp32."""
import numpy as np
import pytest

from cvgpuspeedup_amd import capi, cvgs
from tests import helpers as H
from tests.test_bf16_types import _same_bits, rne_bf16, special_values, widen_bf16

pytestmark = pytest.mark.gpu

GUARD = 4096


def _run(build, out_shape, bf):
    """build(wrap, wrap_out, out, bf) -> iops.  bf=True: on the GPU, with CV_16BF outputs held as uint16; bf=False: on the oracle
    (the fp32 twin).  GPU outputs sit between canary bands that must come back untouched."""
    import torch
    from oracle import oracle_binding as ob
    keep, outs = [], []

    def wrap(a, cvt):
        if bf:
            t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            keep.append(t)
            return cvgs.GpuMat.from_tensor(t, cvt)
        keep.append(a)
        return cvgs.GpuMat.from_array(a, cvt)

    def wrap_out(a, cvt):
        if bf:
            big = torch.full((a.nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            t = big[GUARD:GUARD + a.nbytes].view(torch.from_numpy(a).dtype).view(a.shape)
            t.zero_()
            outs.append((big, t))
            return cvgs.GpuMat.from_tensor(t, cvt)
        outs.append((None, a))
        return cvgs.GpuMat.from_array(a, cvt)

    out = np.zeros(out_shape, np.uint16 if bf else np.float32)
    iops = build(wrap, wrap_out, out, bf)
    if bf:
        cvgs.executeOperations(torch.cuda.current_stream(), *iops)
        torch.cuda.synchronize()
        res = []
        for big, t in outs:
            g = big.cpu().numpy()
            assert (g[:GUARD] == 0xA5).all() and (g[-GUARD:] == 0xA5).all(), "store outside the output"
            res.append(t.cpu().numpy())
        return res, iops
    ob.execute(cvgs.lower(iops))
    return [a for _, a in outs], iops


def _check(build, out_shape, what):
    gpu, iops = _run(build, out_shape, True)
    ref, _ = _run(build, out_shape, False)
    for g, r in zip(gpu, ref):
        want = rne_bf16(r)
        assert _same_bits(g, want), "%s: %d of %d elements differ" % (what, int((g != want).sum()), g.size)
    return gpu, ref, iops


def T(bf, cn):
    """the hand-off type: CV_16BFCn on the GPU, CV_32FCn for the oracle twin"""
    return (cvgs.make_type(capi.DEPTH_16F, cn) | capi.TYPE_FLAG_BF16) if bf else cvgs.make_type(capi.DEPTH_32F, cn)


def _f16_twin_name(iops_bf):
    """cvgs_kernel_name of the same chain with CV_16F in place of every CV_16BF"""
    import copy
    twin = []
    for op in iops_bf:
        o = copy.copy(op)
        for attr in ("dst_type", "out_type", "in_type", "src_type"):
            if hasattr(o, attr) and isinstance(getattr(o, attr), int):
                setattr(o, attr, getattr(o, attr) & ~capi.TYPE_FLAG_BF16)
        if hasattr(o, "ops"):
            o.ops = [(c, (a & ~capi.TYPE_FLAG_BF16) if c in (capi.OP_CAST, capi.OP_CAST_TRUNC) else a, v) for c, a, v in o.ops]
        twin.append(o)
    return cvgs.kernel_name(*twin)


def _assert_twin_name(iops_bf):
    name, f16 = cvgs.kernel_name(*iops_bf), _f16_twin_name(iops_bf)
    assert "f16" in f16 and name == f16.replace("f16", "bf16"), (name, f16)


def _k1_ops(cn, swap, bf):
    f = cvgs.make_type(cvgs.CV_32F, cn)
    ops = [cvgs.cvtColor(cvgs.COLOR_RGB2BGR if cn == 3 else cvgs.COLOR_RGBA2BGRA, f)] if swap else []
    ops += [cvgs.multiply(f, [0.3] * cn), cvgs.subtract(f, H.K1_SUB[cn]), cvgs.divide(f, H.K1_DIV[cn])]
    return ops + ([cvgs.convertTo(f, T(True, cn))] if bf else [])


@pytest.mark.parametrize("cn,swap,transposed", [(3, True, False), (4, True, False), (3, False, True), (4, False, False)])
def test_k1_bf16_output(cn, swap, transposed):
    src = H.random_u8((500, 700, cn), 40 + cn)
    crops = H.random_crops(13, 700, 500, seed=9 + cn, wmin=1, wmax=600, hmin=1, hmax=450)
    dst, n, used = (64, 128), 13, 11
    u = cvgs.make_type(cvgs.CV_8U, cn)

    def build(wrap, wrap_out, out, bf):
        frame = wrap(src, u)
        rd = cvgs.resize(u, cvgs.INTER_LINEAR, [frame.roi(*c) for c in crops], dst, used, [17.0, 99.5, 3.0, 200.0][:cn])
        o = wrap_out(out, T(bf, 1))
        wr = cvgs.splitT(T(bf, cn), o.data, dst[0], dst[1], n, keep=o) if transposed else cvgs.split(T(bf, cn), o, dst)
        return [rd] + _k1_ops(cn, swap, bf) + [wr]

    _, ref, iops = _check(build, (n, cn * 64 * 128), "K1 bf16 C%d" % cn)
    assert np.isfinite(ref[0]).all() and ref[0].std() > 1.0
    _assert_twin_name(iops)


def test_k1_bf16_preserve_ar_and_table():
    """PRESERVE_AR padding + 70 planes (more than the kernel-argument block holds), bf16 output; the interpreted and canonical programs."""
    src = H.random_u8((300, 400, 3), 3)
    n = 70
    crops = H.random_crops(n, 400, 300, seed=5, wmin=2, wmax=200, hmin=2, hmax=280)
    dst = (48, 40)
    f = cvgs.CV_32FC3
    progs = {"ref": lambda bf: _k1_ops(3, True, bf),
             "canon": lambda bf: [cvgs.multiply(f, [1 / 255.0] * 3), cvgs.subtract(f, [0.485, 0.456, 0.406]), cvgs.divide(f, [0.229, 0.224, 0.225]),
                                  cvgs.add(f, [0.5] * 3)] + ([cvgs.convertTo(f, T(True, 3))] if bf else []),
             "interp": lambda bf: [cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f), cvgs.multiply(f, [0.5] * 3)] +
                                  ([cvgs.convertTo(f, T(True, 3))] if bf else [])}
    for name, prog in progs.items():
        def build(wrap, wrap_out, out, bf):
            frame = wrap(src, cvgs.CV_8UC3)
            rd = cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [frame.roi(*c) for c in crops], dst, n, [128.0, 64.0, 32.0], cvgs.PRESERVE_AR)
            return [rd] + prog(bf) + [cvgs.split(T(bf, 3), wrap_out(out, T(bf, 1)), dst)]

        _, _, iops = _check(build, (n, 3 * 48 * 40), "K1 bf16 PRESERVE_AR, 70 planes, %s program" % name)
        _assert_twin_name(iops)


def test_bf16_conversion_special_values():
    """convertTo<CV_32F, CV_16BF> on every tie / overflow / subnormal class (interpreted and K1-adjacent pointwise paths), and back."""
    vals = special_values()
    n = (vals.size // 128) * 128
    src = np.concatenate([vals[:n], vals[-128:]]).reshape(-1, 128, 1).copy()

    def build(wrap, wrap_out, out, bf):
        return [cvgs.ReadIOp(capi.READ_PIXEL, cvgs.CV_32FC1, [wrap(src, cvgs.CV_32FC1)], 1)] + \
               ([cvgs.convertTo(cvgs.CV_32FC1, T(True, 1))] if bf else []) + [cvgs.write(T(bf, 1), wrap_out(out, T(bf, 1)))]

    gpu, _, _ = _check(build, src.shape, "fp32 -> bf16")
    bsrc = gpu[0].copy()

    def back(wrap, wrap_out, out, bf):  # the oracle reads the exact widening of the bf16 source
        a = bsrc if bf else widen_bf16(bsrc)
        st = T(bf, 1)
        return [cvgs.ReadIOp(capi.READ_PIXEL, st, [wrap(a, st)], 1)] + ([cvgs.convertTo(st, cvgs.CV_32FC1)] if bf else []) + \
               [cvgs.multiply(cvgs.CV_32FC1, [3.0]), cvgs.convertTo(cvgs.CV_32FC1, T(True, 1)) if bf else cvgs.multiply(cvgs.CV_32FC1, [1.0]),
                cvgs.write(T(bf, 1), wrap_out(out, T(bf, 1)))]

    _check(back, src.shape, "bf16 source -> fp32 * 3 -> bf16")


@pytest.mark.parametrize("src_depth,cn", [("8U", 3), ("16U", 4), ("16S", 1), ("32S", 2)])
def test_pointwise_to_bf16(src_depth, cn):
    from tests import kat_runner as K
    from tests.test_gpu_chains import _random_src
    a = _random_src((45, 67, cn), src_depth, 21)
    st = cvgs.make_type(K.CV_DEPTH[src_depth], cn)
    srcs = [(a, (45, 67, cn))]
    if src_depth == "8U":
        srcs.append((_random_src((9, 555, cn), src_depth, 22), (9, 555, cn)))  # wide rows
    for arr, shape in srcs:
        def packed(wrap, wrap_out, out, bf):
            return [cvgs.ReadIOp(capi.READ_PIXEL, st, [wrap(arr, st)], 1), cvgs.convertTo(st, T(bf, cn), 1.0 / 255.0, -0.25),
                    cvgs.write(T(bf, cn), wrap_out(out, T(bf, cn)))]

        _, _, iops = _check(packed, shape, "pointwise %s -> bf16 packed %s" % (src_depth, shape))
        if src_depth == "8U":  # (u8 sources: the thread-fused pointwise kernel, as for fp16)
            _assert_twin_name(iops)
    if cn > 1:
        def planar(wrap, wrap_out, out, bf):
            o = wrap_out(out, T(bf, 1))
            return [cvgs.ReadIOp(capi.READ_PIXEL, st, [wrap(a, st)], 1), cvgs.convertTo(st, T(bf, cn), 1.0 / 255.0, -0.25),
                    cvgs.split_tensor(T(bf, cn), o.data, 67, 45, 1, keep=o)]

        _, _, iops = _check(planar, (1, cn * 45 * 67), "pointwise %s -> bf16 planar" % src_depth)
        if src_depth == "8U":
            _assert_twin_name(iops)


def test_64f_and_16f_to_bf16_and_back():
    src = (H.random_u8((8, 8, 3), seed=3).astype(np.float32) / 7.0)

    def via64(wrap, wrap_out, out, bf):
        f, d = cvgs.CV_32FC3, cvgs.CV_64FC3
        return [cvgs.ReadIOp(capi.READ_PIXEL, f, [wrap(src, f)], 1), cvgs.convertTo(f, d), cvgs.multiply(d, [1.0 / 3.0, 0.1, 7.0]),
                cvgs.add(d, [1e-3, 2.5, -4.0]), cvgs.convertTo(d, T(bf, 3)), cvgs.write(T(bf, 3), wrap_out(out, T(bf, 3)))]

    _check(via64, (8, 8, 3), "64F -> bf16")
    half = src.astype(np.float16)

    def via16(wrap, wrap_out, out, bf):  # fp16 -> bf16 -> fp16 (the oracle: fp16 -> fp32, rounded on the host)
        h = cvgs.CV_16FC3
        ops = [cvgs.convertTo(h, T(True, 3)), cvgs.convertTo(T(True, 3), cvgs.CV_32FC3)] if bf else [cvgs.convertTo(h, cvgs.CV_32FC3)]
        return [cvgs.ReadIOp(capi.READ_PIXEL, h, [wrap(half, h)], 1)] + ops + [cvgs.multiply(cvgs.CV_32FC3, [1.0])] + \
               ([cvgs.convertTo(cvgs.CV_32FC3, T(True, 3))] if bf else []) + [cvgs.write(T(bf, 3), wrap_out(out, T(bf, 3)))]

    _check(via16, (8, 8, 3), "fp16 -> bf16 -> fp32 -> bf16")


def test_bf16_sources_resize_and_warp():
    """CV_16BF images as resize and warp sources (taps widened exactly), fp32 outputs bit-exact vs the oracle on the widened image."""
    import torch
    from oracle import oracle_binding as ob
    bsrc = rne_bf16(H.random_u8((40, 50, 3), seed=8).astype(np.float32) / 3.0)
    s = torch.cuda.current_stream()
    t = torch.from_numpy(bsrc).cuda().view(torch.bfloat16)
    for kind in ("resize", "warp"):
        def read(m, st):
            if kind == "resize":
                return cvgs.resize(st, cvgs.INTER_LINEAR, [m.roi(3, 2, 40, 30)] * 2, (17, 23), 2)
            return cvgs.warp(cvgs.WARP_AFFINE, st, [m] * 2, [[[0.7, 0.1, 2.0], [-0.05, 0.8, 1.5]]] * 2, (31, 19))

        w, h = (17, 23) if kind == "resize" else (31, 19)
        o = torch.zeros((2, 3 * w * h), dtype=torch.float32, device="cuda")
        cvgs.executeOperations(s, read(cvgs.GpuMat.from_tensor(t, cvgs.CV_16BFC3), cvgs.CV_16BFC3),
                               cvgs.split(cvgs.CV_32FC3, cvgs.GpuMat.from_tensor(o, cvgs.CV_32FC1), (w, h)))
        torch.cuda.synchronize()
        wide = widen_bf16(bsrc)
        ref = np.zeros((2, 3 * w * h), np.float32)
        ob.execute(cvgs.lower([read(cvgs.GpuMat.from_array(wide, cvgs.CV_32FC3), cvgs.CV_32FC3),
                               cvgs.split(cvgs.CV_32FC3, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), (w, h))]))
        H.assert_bit_exact(o.cpu().numpy(), ref, "bf16 %s source" % kind)


def test_circular_tensor_bf16(oracle):
    """CircularTensor with CV_16BFC1 elements, in default, capturable and mirrored form: ordering and content vs the oracle's fp32 twin."""
    import torch
    from tests.test_gpu_circular_nv12 import _read_device
    W, H_, B = 80, 46, 4
    f = cvgs.CV_32FC3
    s = torch.cuda.current_stream()
    for flags in ({}, {"capturable": True}, {"mirrored": True}):
        ct = cvgs.CircularTensor(cvgs.CV_8UC3, cvgs.CV_16BFC1, 3, B, cvgs.NewestFirst, cvgs.Standard, W, H_, **flags)
        oc = oracle.OracleCircular(W, H_, cvgs.CV_32FC1, 3, B, cvgs.NewestFirst, cvgs.Standard)
        for i in range(2 * B + 1):
            frame = H.random_u8((H_, W, 3), seed=300 + i)
            frame_t = torch.from_numpy(frame).cuda()
            pw = [cvgs.convertTo(cvgs.CV_8UC3, f), cvgs.multiply(f, [1.0 / 255.0] * 3), cvgs.subtract(f, [0.485, 0.456, 0.406]),
                  cvgs.divide(f, [0.229, 0.224, 0.225])]
            ct.update(s, cvgs.GpuMat.from_tensor(frame_t, cvgs.CV_8UC3), *pw, cvgs.convertTo(f, cvgs.CV_16BFC3), ct.write_split(cvgs.CV_16BFC3))
            oc.update(cvgs.lower([cvgs.ReadIOp(capi.READ_PIXEL, cvgs.CV_8UC3, [cvgs.GpuMat.from_array(frame, cvgs.CV_8UC3)], 1),
                                  *pw, cvgs.WriteIOp(capi.WRITE_TENSOR_SPLIT, f, 16, W, H_, 0, B)]))
            torch.cuda.synchronize()
            got = _read_device(ct.data(), ct.nbytes()).view(np.uint16)
            assert _same_bits(got, rne_bf16(oc.array(np.float32))), "bf16 circular update %d (%s)" % (i, flags)
        assert ct.nbytes() == B * 3 * W * H_ * 2
        ct.release()


def test_warp_and_nv12_bf16_tensors(oracle):
    """bf16 NCHW from N warped faces and from crops of 4:2:0 surfaces in every layout."""
    import torch
    from tests.test_gpu_circular_nv12 import _nv12
    f = cvgs.CV_32FC3
    src = H.random_u8((300, 400, 3), 77)
    n, dst = 5, (112, 112)
    ms = [[[0.4 + 0.1 * i, 0.05 * i, -10.0 * i], [-0.03 * i, 0.5, 7.0]] for i in range(n)]

    def build(wrap, wrap_out, out, bf):
        img = wrap(src, cvgs.CV_8UC3)
        return [cvgs.warp(cvgs.WARP_AFFINE, cvgs.CV_8UC3, [img] * n, ms, dst)] + _k1_ops(3, False, bf) + \
               [cvgs.split(T(bf, 3), wrap_out(out, T(bf, 1)), dst)]

    _, _, iops = _check(build, (n, 3 * dst[0] * dst[1]), "warp -> bf16 NCHW")
    _assert_twin_name(iops)
    w, hh, d2 = 640, 360, (64, 128)
    for layout in (capi.YUV_NV12, capi.YUV_NV21, capi.YUV_P010, capi.YUV_I420, capi.YUV_YV12):
        p010 = layout == capi.YUV_P010
        buf = _nv12(w, hh, 99)
        if p010:
            buf = (buf.astype(np.uint16) << 8) | 0x80
        planar_chroma = layout in (capi.YUV_I420, capi.YUV_YV12)
        rects = [(0, 0, 640, 360)] if planar_chroma else [(0, 0, 640, 360), (10, 20, 100, 200), (300, 100, 64, 128), (2, 2, 8, 8)]
        st = cvgs.CV_16UC1 if p010 else cvgs.CV_8UC1

        def build2(wrap, wrap_out, out, bf):
            m = wrap(buf, st)
            luma = cvgs.GpuMat(hh, w, st, m.data, m.step, owner=m.owner)
            rois = [luma.nv12_roi(*r) if r != (0, 0, 640, 360) else luma for r in rects]
            return [cvgs.read_nv12(rois, d2, capi.YUV_FULL, capi.BT601, False, layout), cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f),
                    cvgs.multiply(f, [0.3 / (4.0 if p010 else 1.0)] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.divide(f, H.K1_DIV[3])] + \
                   ([cvgs.convertTo(f, T(True, 3))] if bf else []) + [cvgs.split(T(bf, 3), wrap_out(out, T(bf, 1)), d2)]

        _, _, iops = _check(build2, (len(rects), 3 * d2[0] * d2[1]), "4:2:0 layout %d -> bf16 NCHW" % layout)
        if layout in (capi.YUV_NV12, capi.YUV_NV21):  # (the fast K4 family serves the interleaved layouts; the others: the interpreted kernel)
            _assert_twin_name(iops)


def test_queue_refuses_bf16():
    import torch
    t = torch.zeros((100, 120, 3), dtype=torch.uint8, device="cuda")
    o = torch.zeros((2, 3 * 32 * 16), dtype=torch.int16, device="cuda")
    frame = cvgs.GpuMat.from_tensor(t, cvgs.CV_8UC3)
    ops = [cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [frame.roi(0, 0, 50, 40), frame.roi(10, 10, 60, 60)], (32, 16), 2)] + \
          _k1_ops(3, True, True) + [cvgs.split(cvgs.CV_16BFC3, cvgs.GpuMat.from_tensor(o, cvgs.CV_16BFC1), (32, 16))]
    q = cvgs.Queue()
    try:
        with pytest.raises(capi.CvgsError, match="bf16"):
            q.submit(*ops)
    finally:
        q.destroy()
    assert not o.any()  # nothing was written (an fp16 store would have been)


def test_k1_bf16_ticks():
    """cvgs_execute_many: 4 cameras' bf16 K1 chains in ONE launch (host descriptors and device tables), each bit-exact vs its fp32 twin."""
    import torch
    from oracle import oracle_binding as ob
    dst, n = (64, 128), 12
    frames = [H.random_u8((360, 480, 3), seed=70 + i) for i in range(4)]
    crops = [H.random_crops(n, 480, 360, seed=80 + i, wmin=4, wmax=300, hmin=4, hmax=300) for i in range(4)]
    refs = []
    for fr, cr in zip(frames, crops):
        ref = np.zeros((n, 3 * 64 * 128), np.float32)
        m = cvgs.GpuMat.from_array(fr, cvgs.CV_8UC3)
        ob.execute(cvgs.lower([cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [m.roi(*c) for c in cr], dst, n)] + _k1_ops(3, True, False) +
                              [cvgs.split(cvgs.CV_32FC3, cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), dst)]))
        refs.append(rne_bf16(ref))
    ts = [torch.from_numpy(fr).cuda() for fr in frames]
    keep = []
    for table in (False, True):
        outs = [torch.zeros((n, 3 * 64 * 128), dtype=torch.int16, device="cuda") for _ in range(4)]
        chains = []
        for t, cr, o in zip(ts, crops, outs):
            m = cvgs.GpuMat.from_tensor(t, cvgs.CV_8UC3)
            rd = cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [m.roi(*c) for c in cr], dst, n)
            if table:  # a resident device plane table (cvgs_plane_table_build)
                tab = torch.frombuffer(bytearray(cvgs.build_plane_table(rd)), dtype=torch.uint8).cuda()
                keep.append(tab)
                rd.table = tab.data_ptr()
            chains.append([rd] + _k1_ops(3, True, True) + [cvgs.split(cvgs.CV_16BFC3, cvgs.GpuMat.from_tensor(o, cvgs.CV_16BFC1), dst)])
        held = cvgs.executeMany(torch.cuda.current_stream(), chains)
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            assert _same_bits(o.cpu().numpy().view(np.uint16), refs[i]), "tick camera %d (table %s)" % (i, table)
        del held


@pytest.mark.parametrize("cn", [3, 4])
def test_k1_bf16_packed_pixels(cn):
    """K1 into packed PIXEL_3D bf16 pixels (the pair stores and, for C3, the tail element), headline and canonical programs."""
    src = H.random_u8((300, 400, cn), 60 + cn)
    crops = H.random_crops(9, 400, 300, seed=61 + cn, wmin=2, wmax=300, hmin=2, hmax=280)
    dst, n = (37, 29), 9
    u, f = cvgs.make_type(cvgs.CV_8U, cn), cvgs.make_type(cvgs.CV_32F, cn)
    for name, prog in (("ref", lambda bf: _k1_ops(cn, True, bf)),
                       ("canon", lambda bf: [cvgs.multiply(f, [1 / 255.0] * cn), cvgs.add(f, [0.25] * cn)] + ([cvgs.convertTo(f, T(True, cn))] if bf else []))):
        def build(wrap, wrap_out, out, bf):
            frame = wrap(src, u)
            rd = cvgs.resize(u, cvgs.INTER_LINEAR, [frame.roi(*c) for c in crops], dst, n)
            return [rd] + prog(bf) + [cvgs.write(T(bf, cn), wrap_out(out, T(bf, cn)), dst)]

        _, _, iops = _check(build, (n, dst[0] * dst[1] * cn), "K1 bf16 packed C%d, %s program" % (cn, name))
        _assert_twin_name(iops)


def test_k1_bf16_mirrors():
    """K1 with cvgs_write_desc.mirrors and a bf16 tensor: every mirror receives the same bytes as the primary tensor, which is bit-exact."""
    import torch
    src = H.random_u8((400, 600, 3), 91)
    crops = H.random_crops(24, 600, 400, seed=92, wmin=4, wmax=300, hmin=4, hmax=300)
    dst, n = (64, 128), 24
    mirrors = [torch.zeros((n, 3 * 64 * 128), dtype=torch.int16, device="cuda") for _ in range(3)]

    def build(wrap, wrap_out, out, bf):
        frame = wrap(src, cvgs.CV_8UC3)
        wr = cvgs.split(T(bf, 3), wrap_out(out, T(bf, 1)), dst)
        if bf:
            wr.mirrored_to([m.data_ptr() for m in mirrors])
        return [cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [frame.roi(*c) for c in crops], dst, n)] + _k1_ops(3, True, bf) + [wr]

    gpu, _, iops = _check(build, (n, 3 * 64 * 128), "K1 bf16 mirrored")
    _assert_twin_name(iops)
    for i, m in enumerate(mirrors):
        assert np.array_equal(m.cpu().numpy().view(np.uint16), gpu[0]), "mirror %d" % i


def test_k1_bf16_special_values_fast_path():
    """The K1 bf16 store (not only the interpreted kernel's) on the overflow boundary, fp32 subnormals and values that round into bf16
    subnormals: a u8 ramp resized at its own size and scaled into each range, bit-exact vs the rounded fp32 twin."""
    u = cvgs.CV_8UC3
    src = (np.arange(256 * 64, dtype=np.uint32) % 256).astype(np.uint8).reshape(64, 256, 1).repeat(3, axis=2).copy()
    for sc in (3.3895314e38 / 255.0, 3.4028235e38 / 254.0, 1.1754944e-38 / 255.0, 9.1835e-41 / 255.0, 2.0 ** -133, 1.0 / 3.0):
        def build(wrap, wrap_out, out, bf):
            f = cvgs.CV_32FC3
            rd = cvgs.resize(u, cvgs.INTER_LINEAR, [wrap(src, u)], (256, 64), 1)
            return [rd, cvgs.multiply(f, [sc, -sc, sc * 1.0000001])] + ([cvgs.convertTo(f, T(True, 3))] if bf else []) + \
                   [cvgs.split(T(bf, 3), wrap_out(out, T(bf, 1)), (256, 64))]

        _, _, iops = _check(build, (1, 3 * 256 * 64), "K1 bf16 store, scale %g" % sc)
        _assert_twin_name(iops)


def test_bf16_ticks_graph_replay():
    """cvgs_execute_many of 4 cameras' bf16 chains, K1 (device tables) and K4 (NV12 surfaces): one captured kernel node each, replayed from a
    HIP graph, bit-exact vs the fp32 twins."""
    import torch
    from oracle import oracle_binding as ob
    from tests.test_gpu_circular_nv12 import _nv12
    from tests.test_gpu_many import _captured_kernel_nodes
    f = cvgs.CV_32FC3
    keep = []
    for kind in ("k1", "k4"):
        n, dst = 8, (64, 128)
        chains, outs, refs = [], [], []
        for i in range(4):
            if kind == "k1":
                fr = H.random_u8((300, 400, 3), seed=120 + i)
                cr = H.random_crops(n, 400, 300, seed=130 + i, wmin=4, wmax=300, hmin=4, hmax=280)
                mk = lambda m, o, bf, cr=cr: ([cvgs.resize(cvgs.CV_8UC3, cvgs.INTER_LINEAR, [m.roi(*c) for c in cr], dst, n)] + _k1_ops(3, True, bf) +
                                              [cvgs.split(T(bf, 3), o, dst)])
                st = cvgs.CV_8UC3
            else:
                fr = _nv12(640, 360, 140 + i)
                rects = [(0, 0, 640, 360), (10, 20, 100, 200), (300, 100, 64, 128), (2, 2, 64, 64)] * 2

                def mk(m, o, bf, rects=rects):
                    luma = cvgs.GpuMat(360, 640, cvgs.CV_8UC1, m.data, m.step, owner=m.owner)
                    rois = [luma.nv12_roi(*r) for r in rects]
                    return [cvgs.read_nv12(rois, dst, capi.YUV_FULL, capi.BT601, False), cvgs.cvtColor(cvgs.COLOR_RGB2BGR, f),
                            cvgs.multiply(f, [0.3] * 3), cvgs.subtract(f, H.K1_SUB[3]), cvgs.divide(f, H.K1_DIV[3])] + \
                           ([cvgs.convertTo(f, T(True, 3))] if bf else []) + [cvgs.split(T(bf, 3), o, dst)]
                st = cvgs.CV_8UC1
            ref = np.zeros((n, 3 * 64 * 128), np.float32)
            ob.execute(cvgs.lower(mk(cvgs.GpuMat.from_array(fr, st), cvgs.GpuMat.from_array(ref, cvgs.CV_32FC1), False)))
            refs.append(rne_bf16(ref))
            t = torch.from_numpy(fr).cuda()
            o = torch.zeros((n, 3 * 64 * 128), dtype=torch.int16, device="cuda")
            ops = mk(cvgs.GpuMat.from_tensor(t, st), cvgs.GpuMat.from_tensor(o, cvgs.CV_16BFC1), True)
            if kind == "k1":
                tab = torch.frombuffer(bytearray(cvgs.build_plane_table(ops[0])), dtype=torch.uint8).cuda()
                ops[0].table = tab.data_ptr()
                keep.append(tab)
            keep += [t, ops]
            chains.append(ops)
            outs.append(o)
        name = cvgs.kernel_name(*chains[0])
        assert name.endswith("_bf16"), name
        lowered = [cvgs.lower(c) for c in chains]
        packed = cvgs.pack_chains(lowered)
        lib = capi.load_library()
        assert _captured_kernel_nodes(lib, packed, 4, None) == 1, "%s: one fused launch" % kind
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            capi.check(lib.cvgs_execute_many(packed, 4, s.cuda_stream))
        torch.cuda.synchronize()
        for o in outs:
            o.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            capi.check(lib.cvgs_execute_many(packed, 4, s.cuda_stream))
        torch.cuda.synchronize()
        assert not any(o.any() for o in outs)  # captured, not run
        g.replay()
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            assert _same_bits(o.cpu().numpy().view(np.uint16), refs[i]), "%s tick camera %d from the graph" % (kind, i)
        keep += [packed, lowered, g]
