"""Diagnostic: dump results computed with the library SRBD_LIB points at, or compare two such dumps bit
for bit (exit status 1 when an array differs).

    SRBD_LIB=ab/libsrbd_mpc_old.so python scripts/bitcmp.py dump gpurun_out/old.npz
    python scripts/bitcmp.py dump gpurun_out/new.npz
    python scripts/bitcmp.py cmp gpurun_out/old.npz gpurun_out/new.npz

`dump`: the fused step's solution (N = 10, 20; standing and randomized gait; K = 1, 10, 20).
`dump-backward`: the gradients and status words of the C entries srbd_pdipm_backward and srbd_mpc_backward,
called through _native.lib() and not through solver.py, so that the library alone decides what runs: the
workloads of tests/_backward_cases.py (N = 1, 2, 3, 10, 32, both gaits, K = 5, both seeds, B = 16), the
adjoint once more with one entry of one env's A_val changed (NaN rows, status 8), and B = 67 at N = 3
(the grid tail).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dump(path):
    import torch
    from biped_pympc_amd import solver
    from biped_pympc_amd.utils.synthetic import make_workload
    out = {}
    for N in (10, 20):
        for gait in (False, True):
            wl = make_workload(512, N, seed=900 + N + gait, random_gait=gait)
            ins = [torch.from_numpy(a).cuda() for a in wl.inputs]
            for K in (1, 10, 20):
                res = solver.mpc_solve(ins, N, K, 1.0)
                torch.cuda.synchronize()
                for k, name in enumerate(("x", "s", "z", "y", "res", "mu")):
                    out[f"N{N}_g{int(gait)}_K{K}_{name}"] = res[k].cpu().numpy()
    np.savez(path, **out)


def dump_backward(path):
    import torch
    from biped_pympc_amd import _native
    from biped_pympc_amd.layout import Dims
    from tests import _backward_cases as C
    L = _native.lib()
    K = 5
    out = {"_build_id": np.array(_native.build_id())}

    def ptrs(ts):
        return _native.ptr_array([t.data_ptr() if t is not None else 0 for t in ts])

    def run(tag, N, ins, qp, it, g):
        """Both entries on one batch; qp in the solver's input order, every tensor on the device."""
        B, d = g.shape[0], Dims(N)
        stream = torch.cuda.current_stream().cuda_stream
        grads = [torch.full((B, w), 7.0, dtype=torch.float64, device="cuda") for w in d.former_out_nnz]
        st = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        rc = L.srbd_pdipm_backward(N, B, ptrs(qp + it), g.data_ptr(), ptrs(grads), st.data_ptr(), stream)
        _native.check(rc, "srbd_pdipm_backward")
        if ins is not None:
            in_grads = [torch.full((B, w), 7.0, dtype=torch.float64, device="cuda") for w in d.former_in_nnz]
            ws = torch.empty(L.srbd_mpc_backward_workspace_doubles(N, B), dtype=torch.float64, device="cuda")
            st2 = torch.full((B,), -1, dtype=torch.int32, device="cuda")
            rc = L.srbd_mpc_backward(N, B, ptrs(ins), ptrs(it), g.data_ptr(), ws.data_ptr(), ptrs(in_grads),
                                     st2.data_ptr(), stream)
            _native.check(rc, "srbd_mpc_backward")
        torch.cuda.synchronize()
        for o, t in enumerate(grads):
            out[f"{tag}_adjoint_{C.NAMES[o]}"] = t.cpu().numpy()
        out[f"{tag}_adjoint_status"] = st.cpu().numpy()
        if ins is not None:
            for i, t in enumerate(in_grads):
                out[f"{tag}_mpc_in{i:02d}"] = t.cpu().numpy()
            out[f"{tag}_mpc_status"] = st2.cpu().numpy()

    def cuda(arrs, idx=None):
        return [torch.from_numpy(np.ascontiguousarray(a if idx is None else a[idx])).cuda() for a in arrs]

    for N in C.HORIZONS:
        for gait in C.GAITS:
            ins_np, qp_np = C.workload(N, gait)
            it_np = C.iterate(N, gait, K)
            for k, g_np in enumerate(C.seeds(N)):
                tag = f"N{N}_{gait}_K{K}_seed{k}"
                run(tag, N, cuda(ins_np), cuda(qp_np), cuda(it_np), cuda([g_np])[0])
                bad = [a.copy() for a in qp_np]  # one env whose QP is not stage-invariant
                bad[2][5, -1] += 1.0  # the last stage's u block against stage 0's (N = 1 has one stage: no NaN)
                run(tag + "_badA", N, None, cuda(bad), cuda(it_np), cuda([g_np])[0])
                if N == 3:
                    idx = np.arange(67) % C.BATCH
                    run(tag + "_B67", N, cuda(ins_np, idx), cuda(qp_np, idx), cuda(it_np, idx), cuda([g_np], idx)[0])
    n8 = sum(int((v == _native.STATUS_UNSUPPORTED).sum()) for k, v in out.items() if k.endswith("_status"))
    nan = sum(int(np.isnan(v).any(axis=1).sum()) for k, v in out.items() if "_adjoint_grad" in k)
    print(f"{len(out) - 1} arrays from build {_native.build_id()}: {n8} status words are 8, {nan} rows hold NaN")
    np.savez(path, **out)


def cmp(a, b):
    A, B = np.load(a), np.load(b)
    worst, differ = 0.0, 0
    for k in A.files:
        if k not in B.files:
            continue
        x, y = A[k], B[k]
        if k.startswith("_"):  # a note (the build id), not a result
            print(f"{k}: {x} / {y}")
            continue
        same = x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        if not same:
            differ += 1
            d = float(np.nanmax(np.abs(x - y)) / max(np.nanmax(np.abs(x)), 1e-300)) if x.shape == y.shape else np.inf
            worst = max(worst, d)
            print(f"{k}: differs, max rel {d:.3e}")
    n = len([k for k in A.files if not k.startswith("_")])
    missing = sorted(set(A.files) ^ set(B.files))
    if missing:
        print(f"only in one dump: {missing}")
    print(f"{n} arrays, {differ} differ, worst rel diff {worst:.3e}" + (" (bit-identical)" if not differ and not missing else ""))
    return 1 if differ or missing else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif sys.argv[1] == "dump-backward":
        dump_backward(sys.argv[2])
    else:
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
