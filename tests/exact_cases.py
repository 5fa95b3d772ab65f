"""The case grid of the exact model (tests/exact_model.py), shared by tests/test_exact_model_vs_oracle.py (CPU oracle) and the GPU file
tests/test_zzzzzzzzzz_gpu_exact_model.py (kernels).  A case is a function of a backend B that builds the chain on B's memory and returns
(iops, arrays): the iop list and one source array per plane the read uses -- the SAME numpy data the chain reads.

Inputs are small: a few rows of 131 pixels or fewer (131 is no multiple of 4 or 64: the thread-fused kernels stay on their edge code), each
a fixed EDGE LIST for its depth followed by seeded random values (float types: random bit patterns -- NaNs, infinities and subnormals occur --,
moderate values and k + 0.5 ties).  Every convertTo the grid builds carries `convert = (alpha, beta)`, what was ASKED for, which the model
evaluates from convertTo's definition.

REFUSED lists the chains cvgs_validate refuses, by name, with the expected error text; no cast pair is among them."""
import numpy as np

from cvgpuspeedup_amd import capi, cvgs
from tests import exact_model as E

D8U, D8S, D16U, D16S, D32S, D32F, D64F, D16F, D16BF = (cvgs.CV_8U, cvgs.CV_8S, cvgs.CV_16U, cvgs.CV_16S, cvgs.CV_32S, cvgs.CV_32F, cvgs.CV_64F,
                                                       cvgs.CV_16F, capi.DEPTH_16BF)
DEPTHS = [D8U, D8S, D16U, D16S, D32S, D32F, D64F, D16F, D16BF]
INT_DEPTHS = [D8U, D8S, D16U, D16S, D32S]
NAMES = {D8U: "8u", D8S: "8s", D16U: "16u", D16S: "16s", D32S: "32s", D32F: "32f", D64F: "64f", D16F: "16f", D16BF: "16bf"}
W, ROWS = 131, 3


def T(depth, cn):
    return (cvgs.make_type(cvgs.CV_16F, cn) | capi.TYPE_FLAG_BF16) if depth == D16BF else cvgs.make_type(depth, cn)


# ---- backends ---------------------------------------------------------------------------------------------------------------------------
class HostBackend:
    """Chains over numpy memory, for the CPU oracle."""
    device = False

    def __init__(self):
        self.outs = []

    def src(self, arr, cv_type):
        a = np.ascontiguousarray(arr)
        return cvgs.GpuMat.from_array(a, cv_type)

    def out(self, shape, cv_type):
        a = np.zeros(shape, E.NP_DTYPE[E.depth_of(cv_type)])
        self.outs.append(a)
        return cvgs.GpuMat.from_array(a, cv_type)

    def results(self):
        return list(self.outs)


class DeviceBackend:
    """Chains over device memory; every output sits between canary bands that must come back untouched."""
    device = True
    GUARD = 4096

    def __init__(self):
        self.keep, self.outs = [], []

    @staticmethod
    def _torchable(a):
        return a.view(np.int16) if a.dtype == np.uint16 else a

    def src(self, arr, cv_type):
        import torch
        a = np.ascontiguousarray(arr)
        t = torch.from_numpy(self._torchable(a)).cuda()
        self.keep.append(t)
        return cvgs.GpuMat(a.shape[0], a.shape[1], cv_type, t.data_ptr(), a.strides[0], owner=t)

    def out(self, shape, cv_type):
        import torch
        a = np.zeros(shape, E.NP_DTYPE[E.depth_of(cv_type)])
        big = torch.full((a.nbytes + 2 * self.GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        big[self.GUARD:self.GUARD + a.nbytes].zero_()
        self.outs.append((big, a))
        return cvgs.GpuMat(shape[0], shape[1], cv_type, big.data_ptr() + self.GUARD, a.strides[0], owner=big)

    def results(self):
        res = []
        for big, a in self.outs:
            g = big.cpu().numpy()
            assert (g[:self.GUARD] == 0xA5).all() and (g[-self.GUARD:] == 0xA5).all(), "store outside the output"
            res.append(g[self.GUARD:-self.GUARD].view(a.dtype).reshape(a.shape))
        return res


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
_INT_EDGES = [0, 1, -1, 2, -2, 126, 127, 128, 129, -127, -128, -129, 254, 255, 256, 257, 32766, 32767, 32768, 32769, -32767, -32768, -32769, 65534,
              65535, 65536, 65537, 2 ** 31 - 1, 2 ** 31 - 2, -2 ** 31, -2 ** 31 + 1, 2 ** 24 + 1, 2 ** 24 + 3, -2 ** 24 - 1, -2 ** 24 - 3,
              2 ** 24 + 65537,          # float takes it to the bfloat16 tie 2^24 + 2^16, which then goes to even: 2^24; one rounding gives 2^24 + 2^17
              2047, 2048, 2049, 2050, 2051, 65503, 65504, 65519, 65520, 65521, 2147483520, 2147483584, -2147483584, 7, -7, 100, -100, 3, -3,
              # CV_32S values that are NaN / infinity patterns of a float: a lane operation that quiets a signalling NaN changes an integer
              0x7F800000, 0x7F800001, 0x7FC00000, 0xFF800001 - 2 ** 32, 0xFFC00000 - 2 ** 32, 0xFF800000 - 2 ** 32, 0x00000001, 0x00800000, 0x80000001 - 2 ** 32]

_TIES = [0.5, 1.5, 2.5, 3.5, 126.5, 127.5, 128.5, 129.5, 254.5, 255.5, 256.5, 32766.5, 32767.5, 32768.5, 32769.5, 65534.5, 65535.5, 65536.5]
_F32_EDGES = ([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.49999997, -0.49999997, 0.50000006, 0.3, -0.3, 0.9999999, -0.9999999]
              + _TIES + [-t for t in _TIES] +
              [2147483520.0, 2147483648.0, -2147483648.0, -2147483904.0, 4e9, -4e9, 1e9, -1e9, 7e4, -7e4, 300.2, -300.7, 16777216.0, 16777218.0,
               65504.0, 65519.9, 65520.0, 65519.996, 65536.0, 2049.0, 2051.0, 2049.0002, 2050.9998, 2048.0, 2050.0,           # binary16: overflow tie, ties
               1.00390625, 1.01171875, 1.0039063, 1.0117187, 3.3895314e38, 3.4e38, -3.4e38, 3e38,                                    # bfloat16: ties, overflow
               5.9604645e-08, 2.9802322e-08, 2.9802326e-08, 8.940697e-08, 6.1035156e-05, 6.097555e-05, 6.0e-05, 1e-8, -6e-8,            # binary16 subnormals
               1e-40, -1e-40, 1.4e-45, 1.1754942e-38, 1.17549435e-38])                                                                    # float subnormals
_F32_EDGE_BITS = [0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F800001, 0x7FC00001, 0xFF800001, 0xFFFFFFFF, 0x00000001, 0x80000001, 0x007FFFFF]
_F64_EDGES = [2147483647.4, 2147483647.5, 2147483647.0, -2147483648.5, -2147483648.4, -2147483649.0, 2147483648.0, 65519.9, 65519.99999, 65520.0,
              2049.0000001,             # rounds to 2050 directly, to 2048 through float (2049, a tie)
              2050.9999999, 1.0000000596, 1.00000005960464478, 1.0 + 2.0 ** -8 + 1e-10,  # bfloat16: up directly, to 1 through float
              0.1, 1.0 / 3.0, -0.1, 1e300, -1e300, 1e-300, 1e-310, -1e-310, 4.9e-324, -4.9e-324, 2.2250738585072014e-308,
              16777217.0, 16777219.0, -16777217.0, 16777217.000001, 2.0 ** -150, 2.0 ** -150 * 1.0000001, 2.0 ** -149 * 1.5, 1e-46, 3.4028235677973366e38,
              3.40282356779733e38, 3.4028234e38, 255.49999999999997, 255.50000000000003, -0.49999999999999994, 0.49999999999999994, 4294967296.0, 1e19, -1e19]
_F16_EDGES = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 126.5, 127.5, 128.5, -127.5, -128.5, -129.5, 254.5, 255.5,
              256.5, 0.2998, -0.2998, 0.4998, 32752.0, 32768.0, -32768.0, -32784.0, 65504.0, -65504.0, 2048.0, 2049.0, 2050.0, 5.96e-8, 1.2e-7, 6.1e-5,
              6.104e-5, 1.00390625, 1.01171875, 1.0009765625, 255.875, 1023.5, 1024.5]
_BF16_EDGE_BITS = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x7F81, 0xFFC1, 0x0001, 0x8001, 0x007F, 0x0080, 0x3F00, 0xBF00, 0x3FC0, 0xBFC0, 0x4020, 0xC020,
                   0x3F80, 0xBF80, 0x42FF, 0x4300, 0x4301, 0xC300, 0xC301, 0x437E, 0x437F, 0x4380, 0x46FF, 0x4700, 0xC700, 0xC701, 0x477F, 0x4780, 0x4EFF,
                   0x4F00, 0xCF00, 0xCF01, 0x7F7F, 0xFF7F, 0x3380, 0x3300, 0x3340, 0x3880, 0x387F, 0x4500, 0x3E99, 0x3EFF]


def edge_list(depth):
    if depth in INT_DEPTHS:
        lo, hi = E.INT_RANGE[depth]
        return np.array(sorted({v for v in _INT_EDGES if lo <= v <= hi} | {lo, lo + 1, hi, hi - 1}), np.int64).astype(E.NP_DTYPE[depth])
    with np.errstate(all="ignore"):
        if depth == D32F:
            return np.concatenate([np.array(_F32_EDGES, np.float64).astype(np.float32), np.array(_F32_EDGE_BITS, np.uint32).view(np.float32)])
        if depth == D64F:
            f = np.concatenate([np.array(_F32_EDGES, np.float64).astype(np.float32), np.array(_F32_EDGE_BITS, np.uint32).view(np.float32)]).astype(np.float64)
            return np.concatenate([f, np.array(_F64_EDGES, np.float64), np.array([0x7FF0000000000001, 0xFFF8000000000001, 0x000FFFFFFFFFFFFF], np.uint64).view(np.float64)])
        if depth == D16F:
            return np.concatenate([np.array(_F16_EDGES, np.float64).astype(np.float16), np.array([0x0001, 0x8001, 0x03FF, 0x0400, 0x7BFF, 0x7C01, 0xFE00], np.uint16).view(np.float16)])
    return np.array(_BF16_EDGE_BITS, np.uint16)


def source(depth, cn, seed, rows=ROWS, w=W):
    """(rows, w, cn) of `depth`: the edge list, then seeded random values."""
    n = rows * w * cn
    rng = np.random.default_rng(1000 + seed)
    dt = E.NP_DTYPE[depth]
    if depth in INT_DEPTHS:
        lo, hi = E.INT_RANGE[depth]
        a = rng.integers(lo, hi, n, dtype=np.int64, endpoint=True).astype(dt)
        a[1::5] = (rng.integers(-300, 300, a[1::5].size)).clip(lo, hi).astype(dt)  # small values: products and quotients that do not all saturate
    elif depth in (D16F, D16BF):
        a = rng.integers(0, 65535, n, dtype=np.int64, endpoint=True).astype(np.uint16).view(dt)
    else:
        bits = np.uint32 if depth == D32F else np.uint64
        a = rng.integers(0, np.iinfo(bits).max, n, dtype=bits, endpoint=True).view(dt).copy()
        with np.errstate(all="ignore"):
            a[1::3] = rng.uniform(-70000.0, 70000.0, a[1::3].size).astype(dt)
            a[2::3] = (rng.integers(-70000, 70000, a[2::3].size) + 0.5).astype(dt)
            a[5::9] = rng.uniform(-300.0, 300.0, a[5::9].size).astype(dt)
    e = edge_list(depth)
    assert e.size <= n, (e.size, n)
    a[:e.size] = e
    return a.reshape(rows, w, cn)


# ---- builders ---------------------------------------------------------------------------------------------------------------------------
def convert(in_type, out_type, alpha=None, beta=None):
    """cvgs.convertTo that remembers what was asked for: the model evaluates it from convertTo's definition, not from the lowered stages."""
    op = cvgs.convertTo(in_type, out_type, alpha, beta)
    op.convert = (alpha, beta)
    return op


def move(opcode, in_type, out_type, aux, alpha=None):
    return cvgs.PointwiseIOp(in_type, out_type, [(opcode, aux, [alpha] * 4 if alpha is not None else None)])


PAD = 3  # elements of padding behind every row of a pitched 2D output


def chain_case(depth, cn, stages, seed, write="packed2d", batch=1, used=None, background=None, rows=ROWS, w=W):
    """READ_PIXEL of `batch` planes (rows x w x cn of `depth`) -> stages(cn) -> write.  write: packed2d (pitched, PAD elements wider than the
    image: the padding must come back zero) | split (split_tensor) | splitT | batch2d (write_batch, one pitched image per plane) | packed3d."""
    def build(B):
        st = T(depth, cn)
        ops = stages(cn)
        ot = ops[-1].out_type if ops else st
        ocn = capi.type_cn(ot)
        o1 = T(E.depth_of(ot), 1)
        arrays = [source(depth, cn, seed + 17 * z, rows, w) for z in range(batch)]
        n_used = batch if used is None else used
        mats = [B.src(a, st) for a in arrays]
        rd = cvgs.ReadIOp(capi.READ_PIXEL, st, mats, n_used, background=background)
        if write == "packed2d":
            assert batch == 1
            wr = cvgs.write(ot, B.out((rows, w + PAD, ocn), ot).roi(0, 0, w, rows))
        elif write == "batch2d":
            wr = cvgs.write_batch(ot, [B.out((rows, w + PAD, ocn), ot).roi(0, 0, w, rows) for _ in range(batch)])
        elif write == "packed3d":
            wr = cvgs.write(ot, B.out((batch, w * rows, ocn), ot), (w, rows))
        elif write == "split":
            o = B.out((batch, ocn * w * rows), o1)
            wr = cvgs.split_tensor(ot, o.data, w, rows, batch, keep=o)
        else:
            assert write == "splitT", write
            o = B.out((batch, ocn * w * rows), o1)
            wr = cvgs.splitT(ot, o.data, w, rows, batch, keep=o)
        return [rd] + ops + [wr], arrays[:n_used]
    build.write, build.batch, build.rows, build.w = write, batch, rows, w
    return build


def written(build, results, shape):
    """The backend's output arrays as [plane][y][x][c]; the padding of pitched outputs must have stayed zero."""
    n, h, w, c = shape
    if build.write in ("packed2d", "batch2d"):
        assert len(results) == n
        for r in results:
            assert not r[:, w:].any(), "store into the padding of a pitched output"
        return np.stack([r[:, :w] for r in results])
    kind = {"packed3d": E.WRITE_PIXEL_3D, "split": E.WRITE_TENSOR_SPLIT, "splitT": E.WRITE_TENSOR_T_SPLIT}[build.write]
    return E.logical(results[0], shape, kind)


def has_64f(iops):
    if E.depth_of(iops[0].src_type) == D64F or E.depth_of(iops[-1].dst_type) == D64F:
        return True
    return any(E.depth_of(i.in_type) == D64F or E.depth_of(i.out_type) == D64F or any(o[0] in (E.OP_CAST, E.OP_CAST_TRUNC) and o[1] == D64F for o in i.ops)
               for i in iops[1:-1])


def has_bf16(iops):
    return any(capi.type_is_bf16(t) for t in [iops[0].src_type, iops[-1].dst_type] + [i.out_type for i in iops[1:-1]])


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------
CASES = {}   # name -> (group, build)


def add(name, group, build):
    assert name not in CASES, name
    CASES[name] = (group, build)


# cast matrix: 9 x 9 depth pairs, rounding (convertTo) and truncating (cast); one channel for every pair, three for one pair per source depth
C3_PARTNER = {D8U: D32F, D8S: D16U, D16U: D8U, D16S: D8S, D32S: D32F, D32F: D32S, D64F: D16F, D16F: D64F, D16BF: D16S}
for _s in DEPTHS:
    for _d in DEPTHS:
        for _cn in ((1, 3) if C3_PARTNER[_s] == _d else (1,)):
            add("cast_%s_%s_round_c%d" % (NAMES[_s], NAMES[_d], _cn), "cast " + NAMES[_s],
                chain_case(_s, _cn, (lambda s, d: lambda cn: [convert(T(s, cn), T(d, cn))])(_s, _d), seed=_s * 16 + (_d & 15)))
            add("cast_%s_%s_trunc_c%d" % (NAMES[_s], NAMES[_d], _cn), "cast " + NAMES[_s],
                chain_case(_s, _cn, (lambda s, d: lambda cn: [cvgs.cast(T(s, cn), T(d, cn))])(_s, _d), seed=_s * 16 + (_d & 15)))

# integer arithmetic: every integer depth, 1 / 3 / 4 channels, chains of 1 to 3 stages, then a cast to another integer depth and to CV_32F
INT_TAIL = {D8U: D8S, D8S: D16U, D16U: D16S, D16S: D8U, D32S: D16U}


def _int_chain(depth, k, tail):
    hi = E.INT_RANGE[depth][1]

    def stages(cn):
        t = T(depth, cn)
        ch = [[cvgs.multiply(t, [2.9, 3, -0.9, -1][:cn])],
              [cvgs.add(t, [-100.5, 100, 7.7, 0][:cn]), cvgs.divide(t, [3, 0, -2, 5.5][:cn])],
              [cvgs.subtract(t, [hi, 1, -2, 1e12][:cn]), cvgs.multiply(t, [-2, 2e9, 0, 9][:cn]), cvgs.add(t, [1, -1e12, 1, -0.0][:cn])],
              [cvgs.divide(t, [-7, 1e12, 255, -1][:cn])]][k]
        return ch + [convert(t, T(tail, cn))]
    return stages


for _s in INT_DEPTHS:
    for _cn in (1, 3, 4):
        for _k in range(4):
            for _tail in (INT_TAIL[_s], D32F):
                add("int_%s_c%d_chain%d_to_%s" % (NAMES[_s], _cn, _k, NAMES[_tail]), "int " + NAMES[_s],
                    chain_case(_s, _cn, _int_chain(_s, _k, _tail), seed=300 + _s * 8 + _cn))

# CV_64F chains: convertTo<I, 64F>(alpha, beta); +, -, x, / with scalars no float holds (0.1, 1/3, 1e-310), division by +-0; CV_32F stages in front
# of and behind a CV_64F stage; written as CV_64F and after a second cast
F64_SCALARS = {"add": [0.1, 1.0 / 3.0, 1e-310, -0.1], "sub": [0.1, 1.0 / 3.0, 1e-310, -1e300], "mul": [0.1, 1.0 / 3.0, 1e-310, -0.0],
               "div": [0.1, 0.0, -0.0, 1.0 / 3.0]}
F64_OPS = {"add": cvgs.add, "sub": cvgs.subtract, "mul": cvgs.multiply, "div": cvgs.divide}


def _f64_chain(src, kind, out, trunc_out):
    def stages(cn):
        st, d = T(src, cn), T(D64F, cn)
        if kind == "cvt":
            ops = [convert(st, d, 0.1, -1.0 / 3.0)]
        elif kind == "mixed":  # CV_32F arithmetic in front of and behind a CV_64F stage: one IEEE float operation per stage
            f = T(D32F, cn)
            ops = ([convert(st, f)] if src != D32F else []) + [cvgs.multiply(f, [0.1, 3.3, 1e-30, -7.7][:cn]), convert(f, d), cvgs.add(d, [1.0 / 3.0, 0.1, 1e-310, 1e300][:cn]),
                                                                convert(d, f), cvgs.divide(f, [3.0, 0.1, -0.0, 1e-30][:cn])]
            if out == D32F:
                return ops
            return ops + [cvgs.cast(f, T(out, cn)) if trunc_out else convert(f, T(out, cn))]
        else:
            ops = ([convert(st, d)] if src != D64F else []) + [F64_OPS[kind](d, F64_SCALARS[kind][:cn])]
        if out == D64F:
            return ops
        return ops + [cvgs.cast(d, T(out, cn)) if trunc_out else convert(d, T(out, cn))]
    return stages


F64_KINDS = ["cvt", "add", "sub", "mul", "div", "mixed"]
for _s in (D8U, D32S, D32F, D64F):
    for _ki, _k in enumerate(F64_KINDS):
        for _o in (D64F, D32F, D16F, D16BF, D8U, D16S, D32S):
            _cn = 1 if _k == "cvt" else 4
            add("f64_%s_%s_to_%s" % (NAMES[_s], _k, NAMES[_o]), "f64 " + NAMES[_s],
                chain_case(_s, _cn, _f64_chain(_s, _k, _o, trunc_out=(_ki % 2 == 1 and _o in INT_DEPTHS)), seed=500 + _s * 8 + _ki, rows=2))

# channel moves on every depth: ADD_ALPHA (swapping), a 4-channel REORDER, DROP_ALPHA -- alpha values every depth holds exactly
_SWAP3, _ID3, _ROT4 = 2 | (1 << 2) | (0 << 4), 0 | (1 << 2) | (2 << 4), 3 | (0 << 2) | (1 << 4) | (2 << 6)
for _s in DEPTHS:
    add("moves_%s" % NAMES[_s], "structure",
        chain_case(_s, 3, (lambda s: lambda cn: [move(capi.OP_ADD_ALPHA, T(s, 3), T(s, 4), _SWAP3, 77.0 if s in INT_DEPTHS else 0.5),
                                                  move(capi.OP_REORDER, T(s, 4), T(s, 4), _ROT4), move(capi.OP_DROP_ALPHA, T(s, 4), T(s, 3), _ID3),
                                                  move(capi.OP_REORDER, T(s, 3), T(s, 3), _SWAP3)])(_s), seed=700 + (_s & 15), rows=2))


def _u8_f32(cn):
    return [convert(T(D8U, cn), T(D32F, cn), 1.0 / 255.0, -0.25)]


def _f32_f64(cn):
    return [convert(T(D32F, cn), T(D64F, cn)), cvgs.add(T(D64F, cn), [0.1, 1.0 / 3.0, -1e-310][:cn])]


def _s16_arith(cn):
    return [cvgs.multiply(T(D16S, cn), [3, -2.5, 100][:cn]), cvgs.subtract(T(D16S, cn), [-7, 32767, 1][:cn])]


# write kinds on a batch of 3: tensors (NCHW, CNHW) and one pitched image per plane; a thread-fused chain, a CV_64F chain, integer arithmetic
for _nm, _d, _st in (("u8_f32", D8U, _u8_f32), ("f32_f64", D32F, _f32_f64), ("s16_arith", D16S, _s16_arith)):
    for _wk in ("split", "splitT", "batch2d"):
        add("write_%s_%s" % (_wk, _nm), "structure", chain_case(_d, 3, _st, seed=800, write=_wk, batch=3, rows=2))
# default-value planes (used = 2 of 3): one per source class.  Integer-typed reads take integral, in-range default values (what a non-integral one means
# for an integer read is defined nowhere); float-typed reads take non-integral ones
add("used_16u", "structure", chain_case(D16U, 3, lambda cn: [cvgs.multiply(T(D16U, cn), [2, 1, 300]), convert(T(D16U, cn), T(D8U, cn))], seed=810,
                                        write="packed3d", batch=3, used=2, background=[7.0, 200.0, 65535.0], rows=2))
add("used_32s", "structure", chain_case(D32S, 1, lambda cn: [cvgs.add(T(D32S, cn), [5]), convert(T(D32S, cn), T(D32F, cn))], seed=811,
                                        write="split", batch=3, used=2, background=[-16777217.0], rows=2))
add("used_32f", "structure", chain_case(D32F, 3, lambda cn: [cvgs.multiply(T(D32F, cn), [0.1, 3.0, -1.0]), convert(T(D32F, cn), T(D16S, cn))], seed=812,
                                        write="splitT", batch=3, used=2, background=[17.25, -0.3, 99.5], rows=2))
add("used_16f", "structure", chain_case(D16F, 3, lambda cn: [convert(T(D16F, cn), T(D32F, cn))], seed=813,
                                        write="packed3d", batch=3, used=2, background=[0.1, -2049.0, 65520.0], rows=2))
add("used_64f", "structure", chain_case(D64F, 3, lambda cn: [cvgs.multiply(T(D64F, cn), [0.1, 1.0 / 3.0, 3.0])], seed=814,
                                        write="batch2d", batch=3, used=2, background=[0.1, -0.3, 1e-40], rows=2))
# nine planes and more: past the 8 inline planes of the interpreted kernels (generic_inline64; CV_64F chains: the staged table)
add("batch9_s16_arith", "structure", chain_case(D16S, 3, _s16_arith, seed=820, write="splitT", batch=9, rows=2, w=67))
add("batch9_f32_f64", "structure", chain_case(D32F, 3, _f32_f64, seed=821, write="split", batch=9, rows=2, w=67))
add("batch10_u8_f32_used7", "structure", chain_case(D8U, 3, _u8_f32, seed=822, write="split", batch=10, used=7, background=[3.0, 250.0, 0.0], rows=2, w=67))

GROUPS = sorted({g for g, _ in CASES.values()})


def names_of(group):
    return sorted(n for n, (g, _) in CASES.items() if g == group)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _refused_arith(depth, fn):
    def build(B):
        t = T(depth, 3)
        a = source(depth, 3, 900, rows=2)
        return [cvgs.ReadIOp(capi.READ_PIXEL, t, [B.src(a, t)], 1), fn(t, [2.0, 3.0, 4.0]), cvgs.write(t, B.out((2, W, 3), t))], [a]
    return build


REFUSED = {}  # name -> (build, expected error text): chains cvgs_validate refuses.  No cast pair is among them.
for _nm, _fn in F64_OPS.items():
    REFUSED["%s_on_16f" % _nm] = (_refused_arith(D16F, _fn), "arithmetic stages on CV_16F values (convertTo CV_32F first)")
    REFUSED["%s_on_16bf" % _nm] = (_refused_arith(D16BF, _fn), "arithmetic stages on CV_16BF (bf16) values (convertTo CV_32F first)")
