"""One child of tests/test_gpu_k1_rows.py: python -m tests.k1_rows_worker <outdir> with CVGS_K1_RPW = 1, 2 or 4 in the environment (the
library reads the hook once per process).  Builds every case of tests/k1_rows_cases.py on device memory, every output between canary
bands, records the kernel name with its "@rN", runs the chain and writes the outputs' bytes into <outdir>/k1_rows_rpw<N>.npz.
`--names <outdir>`: kernel names only, over host memory -- no GPU (tests/test_k1_rows_cases.py)."""
import ctypes as C
import os
import sys

import numpy as np

from cvgpuspeedup_amd import cvgs
from tests import circular_cases as CC
from tests import k1_rows_cases as K
from tests import model_cases as MC


def case_names(case, backend):
    """[kernel name] of a case's chains, built on `backend()`"""
    if case.kind == "circular":  # (--names only, no handle without a GPU: the push chain over host memory; main() asks for the real update chains)
        a = CC.frame(case.build, 0)
        B = backend()
        return [cvgs.kernel_name(*CC.chain(case.build, B.src(a, cvgs.make_type(cvgs.CV_8U, case.build.cn)), CC.host_write(case.build)))]
    return [cvgs.kernel_name(*b(backend())[0]) for _, b in (K.chains_of(case))]


def names_only(outdir, setting):
    rec = {"kernel::" + c.name: np.array(case_names(c, lambda: MC.HostBackend(bf16_twin=False))) for c in K.CASES.values()}
    np.savez(os.path.join(outdir, "k1_rows_names_rpw%s.npz" % setting), **rec)


def run_circular(case, torch):
    """(kernel names, the ordered tensor's bytes).  A CircularTensor update has no name call of its own: the name is asked for the chain
    that is handed to update() -- the same device source, the same stages, the handle's own write stage -- with the write pointed at the
    handle's tensor, which is what cvgs_circular_update does with it.  (The ring slot it adds as the second target is no input of the
    rows-per-wave choice.)"""
    cc = case.build
    u8, pt = cvgs.make_type(cvgs.CV_8U, cc.cn), CC.pixel_type(cc)
    frames = [torch.from_numpy(CC.frame(cc, i)).cuda() for i in range(K.CIRCULAR_UPDATES)]
    ct = cvgs.CircularTensor(u8, CC.elem_type(cc), CC.color_planes(cc), cc.batch, CC.order_of(cc), CC.mode_of(cc), cc.w, cc.h)
    names = []
    for t in frames:
        ops = CC.chain(cc, cvgs.GpuMat.from_tensor(t, u8), ct.write_split(pt))
        onto_tensor = ct.write_split(pt)
        onto_tensor.data = ct.data()
        names.append(cvgs.kernel_name(*ops[:-1], onto_tensor))
        ct.update(torch.cuda.current_stream(), *ops)
    torch.cuda.synchronize()
    assert ct.updates() == K.CIRCULAR_UPDATES
    out = torch.empty(ct.nbytes(), dtype=torch.uint8, device="cuda")
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(out.data_ptr()), C.c_void_p(ct.data()), C.c_size_t(ct.nbytes()), 3) == 0
    got = out.cpu().numpy()
    ct.release()
    return names, got


def main(outdir, setting):
    import torch
    assert torch.cuda.is_available(), "the worker needs a GPU"
    rec = {}
    stream = torch.cuda.current_stream()
    for case in K.CASES.values():
        if case.kind == "circular":
            names, got = run_circular(case, torch)
            rec["kernel::" + case.name], rec["out::%s::0" % case.name] = np.array(names), got
            continue
        built = []
        for _, b in K.chains_of(case):
            B = MC.DeviceBackend()
            iops, _ = b(B)
            built.append((B, iops))
        rec["kernel::" + case.name] = np.array([cvgs.kernel_name(*iops) for _, iops in built])
        if case.kind == "tick":
            keep = cvgs.executeMany(stream, [iops for _, iops in built])
        else:
            keep = cvgs.executeOperations(stream, *built[0][1])
        torch.cuda.synchronize()
        del keep
        for i, (B, _) in enumerate(built):
            rec["out::%s::%d" % (case.name, i)] = np.ascontiguousarray(B.result()).reshape(-1).view(np.uint8)  # (result() asserts the canary bands)
    np.savez(os.path.join(outdir, "k1_rows_rpw%s.npz" % setting), **rec)
    print("k1_rows_worker: %d cases under CVGS_K1_RPW=%s" % (len(K.CASES), setting), flush=True)


if __name__ == "__main__":
    setting = os.environ.get("CVGS_K1_RPW", "unset")
    if sys.argv[1] == "--names":
        names_only(sys.argv[2], setting)
    else:
        main(sys.argv[1], setting)
