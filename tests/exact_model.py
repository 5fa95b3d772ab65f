"""An EXACT restatement of the chains tests/f64_model.py leaves out: every cast between the nine depths, arithmetic on integer-typed values,
CV_64F arithmetic and the CV_32F stages around it, channel moves on any depth, default-value planes.  None of these operations needs an error
bound -- IEEE single / double operations, cv::saturate_cast, static_cast truncation and saturating 64-bit integer arithmetic are reproducible to
the bit in numpy -- so the comparison is EQUALITY (differs(): integers byte for byte, floats bit for bit with any NaN equal to any NaN; the sign
of zero counts).

Written from the definitions and NOT from oracle/cvgs_oracle.c or the kernels.  It imports numpy and nothing else: the iop objects the tests
build are read by attribute only, the numeric codes are those of the public C header (include/cvgs_hip.h).

evaluate(iops, arrays) -> ndarray in the output's own dtype (CV_16F: float16, CV_16BF: uint16 bit patterns), logical order [plane][y][x][c].
`arrays`: one (H, W, C) array per READ plane in the source's own dtype (CV_16BF: uint16 bit patterns); READ_PIXEL reads only.

How a value is carried between stages: integer depths as int64, CV_32F / CV_16F / CV_16BF as the float32 they equal, CV_64F as float64.

A pointwise iop that carries an attribute `convert = (alpha, beta)` (tests/exact_cases.py sets it on every convertTo it builds) is evaluated
from convertTo's DEFINITION -- alpha and beta narrowed to float, cast to the intermediate type, one multiply, one add, cast to the output
type -- and not from the stages the facade lowered it to; every other iop is evaluated stage by stage.

Every defining choice is a named switch (SPEC) that defaults to the specification; tests/test_exact_model_vs_oracle.py flips each one and shows
that the oracle then differs from the model somewhere on the grid of tests/exact_cases.py."""
import numpy as np

# include/cvgs_hip.h
DEPTH_8U, DEPTH_8S, DEPTH_16U, DEPTH_16S, DEPTH_32S, DEPTH_32F, DEPTH_64F, DEPTH_16F = range(8)
FLAG_BF16 = 0x1000
DEPTH_16BF = DEPTH_16F | FLAG_BF16
READ_PIXEL = 0
(OP_NOP, OP_CAST, OP_MUL, OP_ADD, OP_SUB, OP_DIV, OP_REORDER, OP_ADD_ALPHA, OP_DROP_ALPHA, OP_GRAY, OP_CAST_TRUNC) = range(11)
WRITE_PIXEL_2D, WRITE_PIXEL_3D, WRITE_TENSOR_SPLIT, WRITE_TENSOR_T_SPLIT, WRITE_SPLIT_2D, WRITE_PIXEL_2D_BATCH = range(6)

INT_RANGE = {DEPTH_8U: (0, 255), DEPTH_8S: (-128, 127), DEPTH_16U: (0, 65535), DEPTH_16S: (-32768, 32767), DEPTH_32S: (-2 ** 31, 2 ** 31 - 1)}
NP_DTYPE = {DEPTH_8U: np.uint8, DEPTH_8S: np.int8, DEPTH_16U: np.uint16, DEPTH_16S: np.int16, DEPTH_32S: np.int32, DEPTH_32F: np.float32,
            DEPTH_64F: np.float64, DEPTH_16F: np.float16, DEPTH_16BF: np.uint16}
FLOAT_FORMAT = {DEPTH_32F: (24, -126, 127), DEPTH_16F: (11, -14, 15), DEPTH_16BF: (8, -126, 127)}  # precision bits, min normal exponent, max exponent
SMALL_FLOATS = (DEPTH_16F, DEPTH_16BF)

# Every defining choice; False = the specification.
SPEC = {
    "half_rounds_once": False,            # to CV_16F / CV_16BF in ONE rounding from the source value instead of through float
    "float_rounds_toward_zero": False,    # conversions to CV_32F / CV_16F / CV_16BF truncate instead of rounding to nearest even
    "subnormals_flushed": False,          # a subnormal result of a conversion to a float type becomes a zero of its sign
    "zero_sign_dropped": False,           # a conversion between float types turns -0 into +0
    "nan_to_int_is_min": False,           # NaN -> the integer type's minimum instead of 0
    "convert_truncates": False,           # convertTo's float -> integer step truncates instead of rounding to nearest even
    "cast_rounds": False,                 # fk::Cast's float -> integer step rounds to nearest even instead of truncating
    "s32_overflow_is_min": False,         # float -> CV_32S out of range gives INT32_MIN (the x86 'indefinite') instead of the clamp
    "int_to_int_wraps": False,            # integer -> narrower integer wraps modulo 2^n instead of clamping
    "alpha_beta_as_double": False,        # convertTo's alpha and beta are not narrowed to float
    "convert_in_double": False,           # convertTo's multiply and add are carried in double although the intermediate is CV_32F
    "f64_scalar_narrowed": False,         # the scalar of a CV_64F arithmetic stage is narrowed to float
    "f32_stage_in_double": False,         # CV_32F arithmetic stages are carried in double (no rounding to float after each stage)
    "int_scalar_rounds": False,           # integer arithmetic: the scalar is rounded to nearest instead of truncated toward zero
    "int_scalar_unclamped": False,        # integer arithmetic: the scalar is not clamped to the pixel type
    "int_arith_in_32_bits": False,        # integer arithmetic: the operation wraps at 32 bits instead of running in int64
    "int_div_floors": False,              # integer division rounds toward minus infinity instead of toward zero
    "int_div_by_zero_is_max": False,      # x / 0 = the type's maximum instead of 0
    "int_result_wraps": False,            # integer arithmetic: the result wraps into the type instead of saturating
    "background_skips_chain": False,      # a default-value plane is cast straight to the output type: the arithmetic stages are skipped
    "background_as_double": False,        # the default value is taken as a double (the descriptor's field is a float)
}


def switches(**flipped):
    s = dict(SPEC)
    for k, v in flipped.items():
        if k not in s:
            raise KeyError(k)
        s[k] = v
    return s


# ---- types ----------------------------------------------------------------------------------------------------------------------------
def type_cn(t):
    return ((t >> 3) & 63) + 1


def depth_of(t):
    return DEPTH_16BF if (t & 7) == DEPTH_16F and (t & FLAG_BF16) else (t & 7)


def is_int(depth):
    return depth in INT_RANGE


def widen(arr, depth):
    """Source samples as the carried representation, exactly."""
    a = np.asarray(arr)
    if depth == DEPTH_16BF:
        return (a.astype(np.uint32) << 16).view(np.float32)
    if is_int(depth):
        return a.astype(np.int64)
    if depth == DEPTH_16F:
        return a.astype(np.float32)
    return a.astype(NP_DTYPE[depth])


def narrow(x, depth):
    """The carried representation as the output's own dtype (exact: x holds values of that type)."""
    if depth == DEPTH_16BF:
        return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)
    with np.errstate(all="ignore"):
        return np.asarray(x).astype(NP_DTYPE[depth])


# ---- float formats ----------------------------------------------------------------------------------------------------------------------
def round_to_format(x, depth, sw=SPEC):
    """x (float64, exact) as the nearest value of the float format of `depth` (float64 holding it): round to nearest even, overflow to
    infinity, subnormals kept, NaN / infinities / signed zeros kept (IEEE 754)."""
    p, emin, emax = FLOAT_FORMAT[depth]
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        finite = np.isfinite(x) & (ax > 0)
        _, e = np.frexp(np.where(finite, ax, 1.0))        # ax = m * 2^e, 0.5 <= m < 1
        e = np.maximum(e - 1, emin)                        # exponent of the leading bit, held at the subnormal range's
        q = np.ldexp(1.0, (e - (p - 1)).astype(np.int64))  # one unit in the last place
        t = x / q                                          # exact: q is a power of two and |t| < 2^p (or x is subnormal for float64 too)
        r = (np.trunc(t) if sw["float_rounds_toward_zero"] else np.rint(t)) * q  # np.rint: ties to even
        big = (2.0 - 2.0 ** (1 - p)) * 2.0 ** emax
        over = np.copysign(big if sw["float_rounds_toward_zero"] else np.inf, x)
        r = np.where(np.abs(r) > big, over, r)
        if sw["subnormals_flushed"]:
            r = np.where(np.abs(r) < 2.0 ** emin, np.copysign(0.0, x), r)
        r = np.where(finite, r, x)
        if sw["zero_sign_dropped"]:
            r = np.where(r == 0, 0.0, r)
    return r


def to_f32(x, src, sw=SPEC):
    """A carried value of depth `src` as CV_32F (float32)."""
    if src in (DEPTH_32F,) + SMALL_FLOATS:
        return np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        return round_to_format(np.asarray(x).astype(np.float64), DEPTH_32F, sw).astype(np.float32)  # |int32| < 2^53: exact in float64


# ---- stages -----------------------------------------------------------------------------------------------------------------------------
def cast(x, src, dst, truncating, sw=SPEC):
    if src == dst:
        return x
    if dst == DEPTH_64F:  # every other type widens exactly
        r = np.asarray(x).astype(np.float64)
        return np.where(r == 0, 0.0, r) if (sw["zero_sign_dropped"] and not is_int(src)) else r
    if dst == DEPTH_32F:
        if src in SMALL_FLOATS:
            return np.where(x == 0, np.float32(0), x) if sw["zero_sign_dropped"] else x
        return to_f32(x, src, sw)
    if dst in SMALL_FLOATS:
        if sw["half_rounds_once"] and src not in SMALL_FLOATS:
            v = np.asarray(x).astype(np.float64)
        else:
            v = to_f32(x, src, sw).astype(np.float64)  # first to float, then one more rounding: the double rounding is the definition
        return round_to_format(v, dst, sw).astype(np.float32)
    lo, hi = INT_RANGE[dst]
    if is_int(src):
        if sw["int_to_int_wraps"]:
            return (x - lo) % (hi - lo + 1) + lo
        return np.clip(x, lo, hi)
    with np.errstate(all="ignore"):
        v = np.asarray(x).astype(np.float64)
        nan = np.isnan(v)
        v = np.where(nan, 0.0, v)
        trunc = (truncating and not sw["cast_rounds"]) or (not truncating and sw["convert_truncates"])
        r = np.trunc(v) if trunc else np.rint(v)  # np.rint: ties to even
        out = np.clip(r, lo, hi).astype(np.int64)
        if sw["s32_overflow_is_min"] and dst == DEPTH_32S:
            out = np.where((r < lo) | (r > hi), lo, out)
        if sw["nan_to_int_is_min"]:
            out = np.where(nan, lo, out)
    return out


def _float_op(opcode, a, b):
    with np.errstate(all="ignore"):
        if opcode == OP_MUL:
            return a * b
        if opcode == OP_ADD:
            return a + b
        if opcode == OP_SUB:
            return a - b
        return a / b


def int_scalar(operand, depth, sw=SPEC):
    lo, hi = INT_RANGE[depth]
    s = np.asarray(operand, np.float64)
    s = np.where(np.isnan(s), 0.0, s)
    s = np.rint(s) if sw["int_scalar_rounds"] else np.trunc(s)
    if not sw["int_scalar_unclamped"]:
        s = np.clip(s, lo, hi)
    return np.clip(s, -2.0 ** 62, 2.0 ** 62).astype(np.int64)


def _wrap(v, bits):
    return ((v + (1 << (bits - 1))) % (1 << bits)) - (1 << (bits - 1))


def int_arith(opcode, a, operand, depth, sw=SPEC):
    lo, hi = INT_RANGE[depth]
    b = int_scalar(operand, depth, sw)
    if opcode == OP_MUL:
        r = a * b
    elif opcode == OP_ADD:
        r = a + b
    elif opcode == OP_SUB:
        r = a - b
    else:
        safe = np.where(b == 0, 1, b)
        if sw["int_div_floors"]:
            q = a // safe
        else:
            q = np.sign(a) * np.sign(safe) * (np.abs(a) // np.abs(safe))  # toward zero
        r = np.where(b == 0, hi if sw["int_div_by_zero_is_max"] else 0, q)
    if sw["int_arith_in_32_bits"]:
        r = _wrap(r, 32)
    if sw["int_result_wraps"]:
        return (r - lo) % (hi - lo + 1) + lo
    return np.clip(r, lo, hi)


def arithmetic(x, depth, opcode, operand, sw=SPEC):
    cn = x.shape[-1]
    operand = list(operand)[:cn]
    if depth in SMALL_FLOATS:
        raise ValueError("arithmetic on CV_16F / CV_16BF values is refused by cvgs_validate (tests/exact_cases.REFUSED)")
    if is_int(depth):
        return int_arith(opcode, x, operand, depth, sw)
    if depth == DEPTH_64F:
        s = np.asarray(operand, np.float64)  # the scalar as the double it was given
        if sw["f64_scalar_narrowed"]:
            s = s.astype(np.float32).astype(np.float64)
        return _float_op(opcode, np.asarray(x, np.float64), s)
    with np.errstate(all="ignore"):
        s = np.asarray(operand, np.float64).astype(np.float32)  # the scalar narrowed double -> float, part of the definition
    if sw["f32_stage_in_double"]:
        return _float_op(opcode, np.asarray(x).astype(np.float64), s.astype(np.float64))
    return _float_op(opcode, np.asarray(x).astype(np.float32), s)  # one IEEE float operation


def _reorder(x, aux, n):
    return x[..., [(aux >> (2 * c)) & 3 for c in range(n)]]


def apply_op(x, depth, opcode, aux, operand, sw=SPEC):
    """-> (x, depth)"""
    if opcode == OP_NOP:
        return x, depth
    if opcode in (OP_CAST, OP_CAST_TRUNC):
        dst = aux
        if dst not in NP_DTYPE:
            raise ValueError("bad destination depth %r" % (aux,))
        return cast(x, depth, dst, opcode == OP_CAST_TRUNC, sw), dst
    if opcode in (OP_MUL, OP_ADD, OP_SUB, OP_DIV):
        return arithmetic(x, depth, opcode, operand, sw), depth
    if opcode == OP_REORDER:
        return _reorder(x, aux, x.shape[-1]), depth
    if opcode == OP_DROP_ALPHA:
        return _reorder(x, aux, 3), depth
    if opcode == OP_ADD_ALPHA:  # the grid uses alpha values every depth holds exactly
        y = _reorder(x, aux, 3)
        a = np.float32(operand[0])
        a = np.int64(a) if is_int(depth) else (np.float64(a) if depth == DEPTH_64F else a)
        return np.concatenate([y, np.full(y.shape[:-1] + (1,), a, y.dtype)], -1), depth
    raise NotImplementedError("opcode %r: the exact model holds casts, arithmetic and channel moves (GRAY: tests/f64_model.py)" % (opcode,))


def convert_to(x, src, dst, alpha, beta, sw=SPEC):
    """cvGS::convertTo<I, O>(alpha, beta) from its definition."""
    mid = dst if dst in (DEPTH_32F, DEPTH_64F) else DEPTH_32F  # integer and 16-bit float outputs are computed in float
    with np.errstate(all="ignore"):
        a = np.float64(alpha) if sw["alpha_beta_as_double"] else np.float64(np.float32(alpha))
        b = None if beta is None else (np.float64(beta) if sw["alpha_beta_as_double"] else np.float64(np.float32(beta)))
        v = cast(x, src, mid, False, sw)
        if mid == DEPTH_64F or sw["convert_in_double"] or sw["f32_stage_in_double"]:
            v = np.asarray(v).astype(np.float64) * a
            if b is not None:
                v = v + b
        else:
            v = np.asarray(v).astype(np.float32) * np.float32(a)
            if b is not None:
                v = v + np.float32(b)
    return cast(v, mid, dst, False, sw), dst


def background(rd, depth, cn, shape, sw=SPEC):
    with np.errstate(all="ignore"):
        bg = np.asarray(list(rd.background)[:cn], np.float64)
        if not sw["background_as_double"]:
            bg = bg.astype(np.float32).astype(np.float64)  # the descriptor's field is a float
    if is_int(depth):
        assert np.all(bg == np.rint(bg)) and np.all(bg >= INT_RANGE[depth][0]) and np.all(bg <= INT_RANGE[depth][1]), \
            "a non-integral or out-of-range default value of an integer-typed read is not defined"
        v = bg.astype(np.int64)
    elif depth == DEPTH_64F:
        v = bg
    elif depth == DEPTH_32F:
        v = bg.astype(np.float32)
    else:
        v = round_to_format(bg, depth, sw).astype(np.float32)
    return np.broadcast_to(v, shape + (cn,)).copy()


def run_chain(x, depth, stages, sw=SPEC, casts_only=False):
    for iop in stages:
        conv = getattr(iop, "convert", None)
        if conv is not None and conv[0] is not None and not casts_only:
            assert depth_of(iop.in_type) == depth, (iop.in_type, depth)
            x, depth = convert_to(x, depth, depth_of(iop.out_type), conv[0], conv[1], sw)
            continue
        for opcode, aux, operand in iop.ops:
            if casts_only and opcode in (OP_MUL, OP_ADD, OP_SUB, OP_DIV):
                continue
            x, depth = apply_op(x, depth, opcode, aux, operand, sw)
    return x, depth


def evaluate(iops, arrays, sw=SPEC):
    """iops: [read, pointwise..., write] as the tests build them; arrays: one (H, W, C) array per plane the read uses."""
    rd, wr = iops[0], iops[-1]
    if rd.kind != READ_PIXEL:
        raise NotImplementedError("the exact model holds READ_PIXEL reads (resize, YUV and warp reads: tests/f64_model.py)")
    depth, cn = depth_of(rd.src_type), type_cn(rd.src_type)
    n, used = rd.batch, min(rd.used_planes, rd.batch)
    h, w = np.asarray(arrays[0]).shape[:2]
    outs = []
    with np.errstate(all="ignore"):  # overflow to infinity, division by zero and NaN operands are values here, not events
        for z in range(n):
            if z < used:
                x = widen(np.asarray(arrays[z]).reshape(h, w, cn), depth)
                x, d = run_chain(x, depth, iops[1:-1], sw)
            else:  # the default value, then the whole chain
                x = background(rd, depth, cn, (h, w), sw)
                x, d = run_chain(x, depth, iops[1:-1], sw, casts_only=sw["background_skips_chain"])
            outs.append(x)
    assert d == depth_of(wr.dst_type) and outs[0].shape[-1] == type_cn(wr.dst_type), "the chain's output type is not the write's"
    return narrow(np.stack(outs), d)


# ---- comparison -------------------------------------------------------------------------------------------------------------------------
def logical(got, shape, write_kind):
    """A written output (memory order of the write kind) as [plane][y][x][c]: packed pixels, NCHW (split), CNHW (splitT)."""
    n, h, w, c = shape
    got = np.asarray(got)
    if write_kind == WRITE_TENSOR_SPLIT:
        return got.reshape(n, c, h, w).transpose(0, 2, 3, 1)
    if write_kind == WRITE_TENSOR_T_SPLIT:
        return got.reshape(c, n, h, w).transpose(1, 2, 3, 0)
    return got.reshape(n, h, w, c)


def differs(got, want, depth):
    """bool per element: integers byte for byte; floats bit for bit (the sign of zero counts), any NaN equal to any NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if is_int(depth):
        return got != want
    if depth == DEPTH_16BF:
        fg, fw = widen(got, depth), widen(want, depth)
        return (got != want) & ~(np.isnan(fg) & np.isnan(fw))
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (got.view(bits) != want.view(bits)) & ~(np.isnan(got) & np.isnan(want))
