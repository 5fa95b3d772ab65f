"""What cvgs_circular_update refuses, as a table: handle kind x defect -> error code and the message text of cvgs_api.cpp, character for
character.  The validation block's ORDER is part of the behaviour (the first refusal that fires is the one a caller reads), so some rows
carry two defects and name the text of the earlier check.  After every refusal the handle's updates() is what it was, and at the end of a
handle's rows the whole tensor at data() is still zero: no row launches a kernel.

Handles are 32 x 16, BATCH 3.  Every row goes through the C ABI (capi) with a chain lowered by the facade: the facade itself raises for
none of these defects.  The default and mirrored forms of the frame-size refusal are in tests/test_gpu_advice_r1.py, the refusal of a
stream capture on a default handle in tests/test_gpu_circular_nv12.py.

This module holds the table (ROWS) and its runner; it defines NO test item of its own.  The GPU suite's list of tests is kept from growing
(tests/test_gpu_area.py says how): the item, with a subtest per handle, is in tests/test_zz_gpu_ring.py, collected behind every existing
item."""
import collections
import ctypes as C

from cvgpuspeedup_amd import capi, cvgs

W, H_, B = 32, 16, 3
U3, U4, F3, F4 = cvgs.CV_8UC3, cvgs.make_type(cvgs.CV_8U, 4), cvgs.CV_32FC3, cvgs.make_type(cvgs.CV_32F, 4)
H3 = cvgs.make_type(cvgs.CV_16F, 3)
BF3 = H3 | capi.TYPE_FLAG_BF16

# the texts, copied from cvgpuspeedup_amd/csrc/cvgs_api.cpp
AREA = "CircularTensor::update: INTER_AREA reads (CVGS_READ_RESIZE_AREA) are served by cvgs_execute / cvgs_execute_many only"
NV12 = "CircularTensor::update: NV12 / NV21 surface writes (CVGS_WRITE_NV12) are served by cvgs_execute / cvgs_execute_many only"
TABLE = "CircularTensor::update: warp reads over a device table are not served (host descriptors)"
BATCH = "CircularTensor::update pushes one frame: batch must be 1"
KIND = "CircularTensor needs a TensorSplit / TensorTSplit / TensorWrite stage"
TRANSPOSED = "Transposed CircularTensors need TensorTSplit (and only they)"
PACKED = "packed write needs COLOR_PLANES == 1 and the tensor's element type"
SPLIT = "split write does not match the tensor's planes / element type"
MIRRORS = "mirrors cannot be combined with a CircularTensor update"
SIZE = "the frame produced by the read stage differs from the CircularTensor's plane size"
INVALID, UNSUPPORTED = capi.ERR_INVALID, capi.ERR_UNSUPPORTED

# the handle variants: (element type, COLOR_PLANES, colour-plane mode)
VARIANTS = {
    "planar": (cvgs.CV_32FC1, 3, cvgs.Standard),
    "transposed": (cvgs.CV_32FC1, 3, cvgs.Transposed),
    "packed": (F3, 1, cvgs.Standard),
    "f16": (cvgs.make_type(cvgs.CV_16F, 1), 3, cvgs.Standard),
    "bf16": (cvgs.make_type(cvgs.CV_16F, 1) | capi.TYPE_FLAG_BF16, 3, cvgs.Standard),
}


class Env:
    """device memory the chains point at (no row reads or writes it) and the handle under test"""

    def __init__(self, ct):
        self.ct, self._t, self._held = ct, {}, []

    def zeros(self, *shape, dtype=None):
        torch = _torch()
        self._held.append(torch.zeros(shape, dtype=dtype or torch.uint8, device="cuda:0"))  # (held until the handle's rows are done)
        return self._held[-1]

    def mat(self, w=W, h=H_, cv_type=U3):
        key = (w, h, cv_type)
        if key not in self._t:
            self._t[key] = self.zeros(h, w, cvgs.type_cn(cv_type))
        return cvgs.GpuMat.from_tensor(self._t[key], cv_type)

    def pixel(self, w=W, h=H_, cv_type=U3, batch=1):
        return cvgs.ReadIOp(capi.READ_PIXEL, cv_type, [self.mat(w, h, cv_type)] * batch, batch)

    def to_f3(self):
        return cvgs.convertTo(U3, F3)


# ---- the defects: each builds the IOp list of one refused update ------------------------------------------------------------------------------
def area_read(e):
    return [cvgs.resize(U3, cvgs.INTER_AREA, e.mat(100, 100), (W, H_)), e.ct.write_split(F3)]


def nv12_write(e, read=None):
    surface = e.zeros(H_ + H_ // 2, W)
    return [read or e.pixel(), *([] if read else [e.to_f3()]), cvgs.write_nv12(cvgs.GpuMat(H_, W, cvgs.CV_8UC1, surface.data_ptr(), W, owner=surface))]


def area_read_and_nv12_write(e):
    return nv12_write(e, cvgs.resize(U3, cvgs.INTER_AREA, e.mat(100, 100), (W, H_)))


def device_table_warp(e):
    return [cvgs.warp_table(cvgs.WARP_AFFINE, e.mat(100, 100), e.zeros(1, 64), 1, (W, H_)), e.ct.write_split(F3)]


def batch_two(e):
    return [e.pixel(batch=2), e.to_f3(), e.ct.write_split(F3)]


def pixel_2d_write(e, batch=1):
    out = e.zeros(H_, W, 3, dtype=_torch().float32)
    return [e.pixel(batch=batch), e.to_f3(), cvgs.write(F3, cvgs.GpuMat.from_tensor(out, F3))]


def batch_two_and_pixel_2d_write(e):
    return pixel_2d_write(e, batch=2)


def tensor_split(e):  # (the defect on a Transposed handle)
    return [e.pixel(), e.to_f3(), e.ct.write_split(F3)]


def tensor_t_split(e):  # (the defect on a Standard handle)
    return [e.pixel(), e.to_f3(), e.ct.write_splitT(F3)]


def t_split_of_four_channels(e):  # two defects on a Standard 3-plane handle: the Transposed check comes first
    return [e.pixel(cv_type=U4), cvgs.convertTo(U4, F4), e.ct.write_splitT(F4)]


def packed_write(e):  # (the defect on a 3-plane handle)
    return [e.pixel(), e.to_f3(), e.ct.write_packed(F3)]


def packed_write_of_fp16(e):  # (into a packed fp32 handle)
    return [e.pixel(), cvgs.convertTo(U3, H3), e.ct.write_packed(H3)]


def split_of_four_channels(e):
    return [e.pixel(cv_type=U4), cvgs.convertTo(U4, F4), e.ct.write_split(F4)]


def split_of_fp16(e):
    return [e.pixel(), e.to_f3(), cvgs.convertTo(F3, H3), e.ct.write_split(H3)]


def split_of_bf16(e):
    return [e.pixel(), e.to_f3(), cvgs.convertTo(F3, BF3), e.ct.write_split(BF3)]


def one_mirror(e):
    return [e.pixel(), e.to_f3(), e.ct.write_split(F3).mirrored_to([4096])]


def pixel_2d_write_with_a_mirror(e):  # two defects: the write kind is judged before the mirrors
    ops = pixel_2d_write(e)
    ops[-1].mirrored_to([4096])
    return ops


def frame_of(w, h, resized):
    def defect(e):
        if resized:
            return [cvgs.resize(U3, cvgs.INTER_LINEAR, e.mat(100, 100), (w, h)), e.ct.write_split(F3)]
        return [e.pixel(w, h), e.to_f3(), e.ct.write_split(F3)]
    defect.__name__ = "%s_frame_of_%dx%d" % ("resized" if resized else "per_pixel", w, h)
    return defect


def _torch():
    import torch
    return torch


Row = collections.namedtuple("Row", "kind variant defect code text null_handle")
ROWS = []


def row(kind, variant, defect, code, text, null_handle=False):
    ROWS.append(Row(kind, variant, defect, code, text, null_handle))


for _kind in ("default", "mirrored", "capturable"):
    row(_kind, "planar", area_read, UNSUPPORTED, AREA)
    row(_kind, "planar", nv12_write, UNSUPPORTED, NV12)
    row(_kind, "planar", device_table_warp, UNSUPPORTED, TABLE)
    row(_kind, "planar", batch_two, INVALID, BATCH)
    row(_kind, "planar", pixel_2d_write, INVALID, KIND)
    row(_kind, "planar", tensor_t_split, INVALID, TRANSPOSED)
    row(_kind, "planar", packed_write, INVALID, PACKED)
    row(_kind, "planar", split_of_four_channels, INVALID, SPLIT)
    row(_kind, "planar", one_mirror, INVALID, MIRRORS)
    row(_kind, "packed", packed_write_of_fp16, INVALID, PACKED)
    # two defects: the earlier check's text wins
    row(_kind, "planar", batch_two_and_pixel_2d_write, INVALID, BATCH)
    row(_kind, "planar", area_read, UNSUPPORTED, AREA, null_handle=True)
    row(_kind, "planar", area_read_and_nv12_write, UNSUPPORTED, AREA)
    row(_kind, "planar", t_split_of_four_channels, INVALID, TRANSPOSED)
    row(_kind, "planar", pixel_2d_write_with_a_mirror, INVALID, KIND)
for _kind in ("default", "capturable"):  # (mirrored rings exist in the Standard plane order only)
    row(_kind, "transposed", tensor_split, INVALID, TRANSPOSED)
for _kind, _variant, _defect in (("default", "bf16", split_of_fp16), ("capturable", "bf16", split_of_fp16), ("mirrored", "f16", split_of_bf16),
                                 ("capturable", "f16", split_of_bf16)):
    row(_kind, _variant, _defect, INVALID, SPLIT)
for _w, _h in ((W + 8, H_), (W, H_ + 2), (W // 2, H_ // 2)):  # a capturable handle lowers for its push attempt first: that is where these fire
    row("capturable", "planar", frame_of(_w, _h, resized=False), INVALID, SIZE)
    row("capturable", "planar", frame_of(_w, _h, resized=True), INVALID, SIZE)

HANDLES = sorted(set((r.kind, r.variant) for r in ROWS))


def _read_device(ptr, nbytes):
    torch = _torch()
    t = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), C.c_size_t(nbytes), 3) == 0
    return t.cpu().numpy()


def check_the_table_covers_what_it_is_there_for():
    texts = set(r.text for r in ROWS)
    assert texts == {AREA, NV12, TABLE, BATCH, KIND, TRANSPOSED, PACKED, SPLIT, MIRRORS, SIZE}
    for kind in ("default", "mirrored", "capturable"):
        assert {AREA, NV12, TABLE, BATCH, KIND, TRANSPOSED, PACKED, SPLIT, MIRRORS} <= set(r.text for r in ROWS if r.kind == kind), kind
    assert len(ROWS) == len(set((r.kind, r.variant, r.defect.__name__, r.null_handle) for r in ROWS))


def refused_updates_say_why_and_leave_the_handle_alone(lib, kind, variant):
    torch = _torch()
    elem, planes, mode = VARIANTS[variant]
    ct = cvgs.CircularTensor(U3, elem, planes, B, cvgs.NewestFirst, mode, W, H_, mirrored=kind == "mirrored", capturable=kind == "capturable")
    stream = cvgs.stream_handle(torch.cuda.current_stream())
    try:
        env = Env(ct)
        rows = [r for r in ROWS if (r.kind, r.variant) == (kind, variant)]
        assert rows
        for r in rows:
            low = cvgs.lower(r.defect(env))
            rc = lib.cvgs_circular_update(None if r.null_handle else ct.handle, C.byref(low.desc), stream)
            got = lib.cvgs_last_error().decode()
            assert (rc, got) == (r.code, r.text), (r.defect.__name__, rc, got)
            assert ct.updates() == 0, r.defect.__name__
        torch.cuda.synchronize()
        assert not _read_device(ct.data(), ct.nbytes()).any()
    finally:
        ct.release()


def run_all(device, lib, subtests):
    """The table's own coverage, then every handle's rows as a subtest of ONE item.  Only a mismatch (AssertionError) lets the item go on to
    its next handle: whatever else ends one -- a HIP error at a synchronisation, say -- ends the item."""
    check_the_table_covers_what_it_is_there_for()
    stopped = []
    for kind, variant in HANDLES:
        with subtests.test(handle="%s-%s" % (kind, variant)):
            assert not stopped, "not started: an earlier handle ended with %s" % stopped[0]
            try:
                refused_updates_say_why_and_leave_the_handle_alone(lib, kind, variant)
            except AssertionError:
                raise
            except BaseException as e:
                stopped.append(repr(e)[:300])
                raise
