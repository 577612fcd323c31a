"""The balancing step of LQG-balanced truncation on the device against the same step in NumPy / SciPy on the host, at
cfg2 (N = 58, the benchmark's B and C^T), with the factors the two ms='hamiltonian-sweep' RADI solves return.  Not a
pass/fail gate: the JSON lines it prints (and writes with --out) are the record behind DESIGN.md section 3e.

  solves      the two Riccati solves (regulator, filter), device-resident factors, per-shift cache cleared before each;
  device      lqgbt.balance_factors on the two DeviceFactors (B, C^T uploaded inside the call), T_l / T_r left on the
              device; its parts from one more call of each: the host SVD alone (ricadi_host_lqg_balance on the
              downloaded S) and the rest;
  host        the fetch of both factors over PCIe, then S = Zc^T (M Zf), LAPACK's SVD, T_l, T_r, the four projected
              matrices in NumPy / SciPy (threads as the environment sets them).

Timings: one warm-up call of each, then the two alternate for --trials rounds; median and best of the host clock around
calls that end synchronised.  The line "compare" also carries the distance of the two paths' sigma.

python tools/lqgbt_compare.py [--N 58] [--trials 7] [--tol 1e-10] [--out profiles/lqgbt_cfg2.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=58)
    ap.add_argument("--nu", type=float, default=0.05)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sadptprj_riclyap_adi.lin_alg_utils as lau
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    from optconpy_amd import _lib, backend, lqgbt, problems as pb

    pr = pb.ricc_problem(args.N, args.nu, NU=4, NY=4, alphau=1e-2)
    mct = lau.app_prj_via_sadpnt(amat=pr.M, jmat=pr.J, rhsv=pr.mc_mat.T, transposedprj=True)
    tb = lau.apply_invsqrt_fromright(pr.rmat, pr.b_mat, output="dense")
    Ct = np.ascontiguousarray(lau.apply_invsqrt_fromright(pr.y_masmat, mct, output="dense"))
    B = np.ascontiguousarray(lau.app_prj_via_sadpnt(amat=pr.M, jmat=pr.J, rhsv=np.asarray(tb), transposedprj=True))
    A, M = (-pr.A - pr.Nc).tocsr(), pr.M.tocsr()
    d = dict(ms="hamiltonian-sweep", device_resident=True)
    lines = []

    def emit(rec):
        rec.update(N=args.N, nv=int(M.shape[0]))
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    def solve(transposed):
        backend.context().clear_cache()
        b, w = (Ct, B) if transposed else (B, Ct)
        return pru.proj_alg_ric_radi(mmat=M, amat=A, jmat=pr.J, bmat=b, wmat=w, transposed=transposed, radi_dict=d)

    # ---- the two solves (the filter solve last: it leaves (A, M) resident, the orientation the balancing step needs)
    for name, tr in (("regulator", False), ("filter", True)):
        solve(tr)                                                   # warm-up
    ts = {"regulator": [], "filter": []}
    fac = {}
    for _ in range(max(3, args.trials // 2)):
        for name, tr in (("regulator", False), ("filter", True)):
            out, ms = timed(lambda: solve(tr))
            ts[name].append(ms)
            fac[name] = out
    for name in ts:
        emit(dict(path="solve-" + name, ms_median=statistics.median(ts[name]), ms_best=min(ts[name]),
                  ms_all=[round(v, 2) for v in ts[name]], cols=fac[name]["zfac"].shape[1],
                  radi_steps=fac[name]["radi_steps"], shift_solves=fac[name]["shift_solves"]))
    zc, zf = fac["regulator"]["zfac"], fac["filter"]["zfac"]

    # ---- the balancing step
    def device():
        return lqgbt.balance_factors(M, A, pr.J, zc, zf, B, Ct.T, tol=args.tol)

    def host():
        zch, zfh = zc.numpy(), zf.numpy()                           # the fetch is part of the host path
        S = zch.T @ (M @ zfh)
        U, sig, Vt = np.linalg.svd(S, full_matrices=False)
        r = min(int(np.count_nonzero(sig > args.tol * sig[0])), lqgbt.MAX_ORDER)
        sq = 1.0 / np.sqrt(sig[:r])
        tl, trr = zch @ (U[:, :r] * sq), zfh @ (Vt[:r].T * sq)
        return dict(hsv=sig, order=r, tl=tl, tr=trr, ar=tl.T @ (A @ trr), er=tl.T @ (M @ trr), br=tl.T @ B,
                    cr=Ct.T @ trr)

    def host_fetch():
        return zc.numpy(), zf.numpy()

    device(), host()                                                # warm-up
    td, th, tf = [], [], []
    for _ in range(args.trials):
        od, ms = timed(device)
        td.append(ms)
        oh, ms = timed(host)
        th.append(ms)
        _, ms = timed(host_fetch)
        tf.append(ms)
    # the device path's host SVD alone, on the S the host path forms
    S = zc.numpy().T @ (M @ zf.numpy())
    tj = []
    for _ in range(3):
        t0 = time.perf_counter()
        _lib.host_lqg_balance(S, args.tol, lqgbt.MAX_ORDER)
        tj.append(1e3 * (time.perf_counter() - t0))
    emit(dict(path="balance-device", ms_median=statistics.median(td), ms_best=min(td), ms_all=[round(v, 2) for v in td],
              order=int(od["order"]), kc=zc.shape[1], kf=zf.shape[1], host_jacobi_svd_ms=statistics.median(tj),
              rest_ms=statistics.median(td) - statistics.median(tj)))
    emit(dict(path="balance-host", ms_median=statistics.median(th), ms_best=min(th), ms_all=[round(v, 2) for v in th],
              order=int(oh["order"]), fetch_ms=statistics.median(tf), threads=os.environ.get("OMP_NUM_THREADS")))
    k = int(np.count_nonzero(oh["hsv"] >= 1e-6 * oh["hsv"][0]))
    emit(dict(path="compare", device_ms=statistics.median(td), host_ms=statistics.median(th),
              solves_ms=statistics.median(ts["regulator"]) + statistics.median(ts["filter"]),
              faster="device" if statistics.median(td) < statistics.median(th) else "host",
              sigma_distance=float(np.max(np.abs(od["hsv"][:k] - oh["hsv"][:k]) / oh["hsv"][:k])), tol=args.tol,
              trials=args.trials))
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
