"""An independent model of the CircularTensor ring: a Python list of pushed frames, the function expected(k) -> [slot] -> frame index or
None, and the three memory layouts.  Written from the reference's documented semantics (the ones test_circular_tensor_reference_kat
quotes: tests/batchread/test_circularbatchread_x_write3D.cu) and NOT from oracle/cvgs_oracle.c or the product's slot arithmetic:

  * after k updates, slot z of a NewestFirst tensor holds the frame of age z (age 0 = the frame pushed last);
  * slot z of an OldestFirst tensor holds the frame of age BATCH - 1 - z;
  * a slot whose frame was never pushed holds zero BYTES.

There is no modulo, no ring index and no history buffer here: the frame of age a after k updates is frames[k - 1 - a].  A mirrored ring
and a capturable handle are ways of storing the same tensor, so the model has no notion of either.

Layouts of the tensor at data() (H rows, W columns, C channels per frame, B slots):
  "std"  planar Standard    [B][C][H][W]
  "tr"   planar Transposed  [C][B][H][W]
  "pk"   packed             [B][H][W][C]

The VALUE of a frame is not this module's business: push() takes any object with check(got[1][H][W][C] as float64) -> (ok, ratio), which the
tests obtain from f64_model.evaluate on the push chain, so every tolerance is that model's derived bound.  Numpy only; nothing here imports
oracle/ or the product package.

Every defining choice is a named switch (SPEC) that defaults to the specification; tests/test_ring_model_vs_oracle.py flips each one and
shows that the oracle then falls outside the model on a named case."""
import numpy as np

from tests import f64_model as F

NEWEST_FIRST, OLDEST_FIRST = 0, 1  # include/cvgs_hip.h: cvgs_circular_order

# False = the specification.
SPEC = {
    "age_reversed": False,                 # NewestFirst read as OldestFirst and the reverse
    "transposed_as_standard": False,       # a Transposed tensor laid out as a Standard one
    "unwritten_holds_first_frame": False,  # slots whose frame was never pushed show the first frame instead of zero bytes
    "newest_slot_off_by_one": False,       # the newest frame lands one slot further on (every age moved by one, cyclically)
}

NP_OF_DEPTH = {F.DEPTH_8U: np.uint8, F.DEPTH_32F: np.float32, F.DEPTH_16F: np.float16, F.DEPTH_16BF: np.uint16, F.DEPTH_64F: np.float64}
BITS_OF_SIZE = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def switches(**flipped):
    s = dict(SPEC)
    for k, v in flipped.items():
        if k not in s:
            raise KeyError(k)
        s[k] = v
    return s


def expected(k, batch, order, sw=SPEC):
    """[slot] -> index of the frame it shows after k updates (frames are numbered 0, 1, ... in push order), or None: never pushed."""
    newest_first = (order == NEWEST_FIRST) != bool(sw["age_reversed"])
    out = []
    for z in range(batch):
        age = z if newest_first else batch - 1 - z
        if sw["newest_slot_off_by_one"]:
            age = (age - 1) % batch
        idx = k - 1 - age
        if idx < 0:
            idx = 0 if (sw["unwritten_holds_first_frame"] and k > 0) else None
        out.append(idx)
    return out


class Ring:
    def __init__(self, batch, order, layout, depth, cn, width, height):
        assert layout in ("std", "tr", "pk") and order in (NEWEST_FIRST, OLDEST_FIRST)
        self.batch, self.order, self.layout, self.depth, self.cn, self.w, self.h = batch, order, layout, depth, cn, width, height
        self.frames = []

    def push(self, frame):
        self.frames.append(frame)

    def nbytes(self):
        return self.batch * self.cn * self.h * self.w * np.dtype(NP_OF_DEPTH[self.depth]).itemsize

    def slots(self, elems, sw=SPEC):
        """The tensor's elements (flat, memory order) as one [H][W][C] array per slot."""
        B, C, H, W = self.batch, self.cn, self.h, self.w
        layout = "std" if (self.layout == "tr" and sw["transposed_as_standard"]) else self.layout
        if layout == "std":
            a = elems.reshape(B, C, H, W).transpose(0, 2, 3, 1)
        elif layout == "tr":
            a = elems.reshape(C, B, H, W).transpose(1, 2, 3, 0)
        else:
            a = elems.reshape(B, H, W, C)
        return [a[z] for z in range(B)]

    def check(self, raw, sw=SPEC):
        """raw: the whole tensor as bytes (uint8, nbytes()) after len(frames) updates.  Every element of every slot is compared.
        Returns (bad, ratio, where): the number of elements outside the model, the worst |got - model| / tolerance over the slots that
        show a frame, and a description of the first slot that failed (or None)."""
        raw = np.ascontiguousarray(raw).reshape(-1)
        assert raw.dtype == np.uint8 and raw.size == self.nbytes(), (raw.dtype, raw.size, self.nbytes())
        dt = np.dtype(NP_OF_DEPTH[self.depth])
        elems = raw.view(dt)
        bits = raw.view(BITS_OF_SIZE[dt.itemsize])
        want = expected(len(self.frames), self.batch, self.order, sw)
        bad, worst, where = 0, 0.0, None
        for z, (idx, got, gbits) in enumerate(zip(want, self.slots(elems, sw), self.slots(bits, sw))):
            if idx is None:
                n = int(np.count_nonzero(gbits))
                what = "slot %d must hold zero bytes: %d elements are not" % (z, n)
            else:
                ok, ratio = self.frames[idx].check(F.widen(got, self.depth)[None])
                n = int(ok.size - np.count_nonzero(ok))
                r = float(np.nanmax(ratio))
                worst = max(worst, r)
                what = "slot %d must show frame %d: %d of %d elements outside the bound (worst ratio %.3g)" % (z, idx, n, ok.size, r)
            if n and where is None:
                where = "after %d updates, %s" % (len(self.frames), what)
            bad += n
        return bad, worst, where
