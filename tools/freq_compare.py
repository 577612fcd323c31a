"""The frequency response on the device (lqgbt.freq_response: saddle solves at the complex shifts -i w) against SciPy's
complex sparse LU on the same host, same matrices, one job -- and the two records behind DESIGN.md section 3f that no
test asserts.  Not a pass/fail gate: the JSON lines it prints (and writes with --out) are the record.

  iterations  alpha = -i w, w = logspace(-1, 4, 16), mc = 8 random complex columns in ONE lockstep batch, against the
              real ``shift_solve_batch_dev`` at the sixteen proxy shifts with 16 real columns on the same context: the
              yardstick (same preconditioner setups, same panel width in doubles);
  product     the complex tiled product, 16 groups of mc = 8, per call (host clock around ``--reps`` calls, each ending
              synchronised) beside the real product of the same 16 x 16 real columns called the same way, and the
              real batched launch alone from the library's timing entry (device events, no synchronise per launch;
              the kernel form it took is recorded);
  response    ``freq_response`` at ``--nfreq`` frequencies logspace(-1, 4) with the benchmark's B and C, against
              ``scipy.sparse.linalg.splu`` of the complex saddle matrix per frequency (factorise, solve for the columns
              of B, C V).  One warm-up of each, then the two alternate for ``--trials`` rounds; medians of the host clock
              around calls that end synchronised.  The host path runs ``--host-freqs`` of the frequencies per round
              (evenly spaced; its time is linear in their number) and both are reported per frequency.

python tools/freq_compare.py [--N 58] [--nfreq 64] [--trials 3] [--host-freqs 16] [--out profiles/freq_response_cfg2.json]"""
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
    ap.add_argument("--nfreq", type=int, default=64)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--host-freqs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip-response", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import scipy.sparse as sps
    import scipy.sparse.linalg as spla
    import torch
    import sadptprj_riclyap_adi.lin_alg_utils as lau
    from optconpy_amd import _lib, backend, lqgbt, problems as pb

    pr = pb.ricc_problem(args.N, args.nu, NU=4, NY=4, alphau=1e-2)
    mct = lau.app_prj_via_sadpnt(amat=pr.M, jmat=pr.J, rhsv=pr.mc_mat.T, transposedprj=True)
    tb = lau.apply_invsqrt_fromright(pr.rmat, pr.b_mat, output="dense")
    Ct = np.ascontiguousarray(lau.apply_invsqrt_fromright(pr.y_masmat, mct, output="dense"))
    B = np.ascontiguousarray(lau.app_prj_via_sadpnt(amat=pr.M, jmat=pr.J, rhsv=np.asarray(tb), transposedprj=True))
    Cm = np.ascontiguousarray(Ct.T)
    A, M, J = (-pr.A - pr.Nc).tocsr(), pr.M.tocsr(), pr.J.tocsr()
    nv, np_ = M.shape[0], J.shape[0]
    lines = []

    def emit(rec):
        rec.update(N=args.N, nv=int(nv), n=int(nv + np_))
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    ctx = backend.context_for(A, M, J)            # (cal A, cal E) = (A, M): freq_response's orientation
    ctx.set_lowrank(None, None)
    rng = np.random.default_rng(0)

    # ---- iterations: complex solve against the real solve at the proxy shifts
    om16 = np.logspace(-1.0, 4.0, 16)
    Rc = torch.from_numpy(rng.standard_normal((nv, 8)) + 1j * rng.standard_normal((nv, 8))).to("cuda:0")
    (X, its_c, rr_c), ms_c = timed(lambda: ctx.shift_solve_cplx_batch_dev(-1j * om16, Rc, strict=False))
    (X, its_c, rr_c), ms_c = timed(lambda: ctx.shift_solve_cplx_batch_dev(-1j * om16, Rc, strict=False))
    del X
    prox = np.array([_lib.host_cplx_proxy(-1j * w) for w in om16])
    Rr = torch.from_numpy(rng.standard_normal((nv, 16))).to("cuda:0")
    Xr = torch.empty((16, nv + np_, 16), dtype=torch.float64, device="cuda:0")
    ctx.set_recycle(0)

    def real_solve():
        return ctx.shift_solve_batch_dev(prox, np.ones(16), Rr.data_ptr(), 0, 16, Xr.data_ptr(), strict=False)

    real_solve()
    (its_r, rr_r), ms_r = timed(real_solve)
    emit(dict(path="iterations", omegas=om16.tolist(), proxies=prox.tolist(), cplx_iters=list(its_c),
              real_iters=list(its_r), ratio=[round(a / max(b, 1), 2) for a, b in zip(its_c, its_r)],
              cplx_worst_relres=float(rr_c.max()), real_worst_relres=float(rr_r.max()),
              cplx_not_converged=[float(w) for w, r in zip(om16, rr_c.max(axis=1)) if r > 1e-10],
              cplx_ms=ms_c, real_ms=ms_r, restart=30, mc=8, real_columns=16))
    del Xr

    # ---- product: per call, and the real multi-shift launch alone
    n = nv + np_
    Xc = torch.from_numpy(rng.standard_normal((16, n, 8)) + 1j * rng.standard_normal((16, n, 8))).to("cuda:0")
    Yc = torch.zeros_like(Xc)
    Xre = torch.view_as_real(Xc).reshape(16, n, 16).contiguous()
    Yre = torch.zeros_like(Xre)
    al = -1j * om16

    def cplx_calls():
        for _ in range(args.reps):
            ctx.op_apply_cplx_batch_dev(al, Xc, Y_t=Yc)

    def real_calls():
        for _ in range(args.reps):
            ctx.op_apply_batch_dev(prox, np.ones(16), Xre.data_ptr(), n * 16, 16, Yre.data_ptr(), n * 16)

    _, var = ctx.op_apply_cplx_batch_dev(al, Xc, Y_t=Yc)
    cplx_calls(), real_calls()
    tc, tr = [], []
    for _ in range(5):
        tc.append(timed(cplx_calls)[1] / args.reps)
        tr.append(timed(real_calls)[1] / args.reps)
    ms_launch = ctx.time_spmm_batch_dev(prox, np.ones(16), Xre.data_ptr(), 16, Yre.data_ptr(), 200)
    emit(dict(path="product", cplx_form=var, cplx_ms_per_call=statistics.median(tc), real_ms_per_call=statistics.median(tr),
              real_launch_ms=float(ms_launch), real_launch_form=int(ctx.setup_info()["k1_variant"]), groups=16,
              real_columns=16, reps=args.reps))
    del Xc, Yc, Xre, Yre

    # ---- response: device against SciPy's complex LU
    if not args.skip_response:
        om = np.logspace(-1.0, 4.0, args.nfreq)
        sub = om[np.linspace(0, om.size - 1, min(args.host_freqs, om.size)).round().astype(int)]
        K = sps.bmat([[A, J.T], [J, None]], format="csc").astype(np.complex128)
        E0 = sps.bmat([[M, None], [None, sps.csc_matrix((np_, np_))]], format="csc").astype(np.complex128)
        rhs = np.vstack([-B, np.zeros((np_, B.shape[1]))]).astype(np.complex128)

        def device(freqs=om):
            return lqgbt.freq_response(M, A, J, B, Cm, freqs, info=True)

        def host(freqs=sub):
            return np.stack([Cm @ spla.splu((K - 1j * w * E0).tocsc()).solve(rhs)[:nv] for w in freqs])

        device(om[:16]), host(sub[:2])                              # warm-up
        td, th = [], []
        for _ in range(args.trials):
            (Gd, info), ms = timed(device)
            td.append(ms / om.size)
            Gh, ms = timed(host)
            th.append(ms / sub.size)
        Gs = device(sub)[0]
        dist = float(max(np.linalg.norm(Gs[k] - Gh[k]) / np.linalg.norm(Gh[k]) for k in range(sub.size)))
        emit(dict(path="response", nfreq=int(om.size), host_freqs=int(sub.size), nu=int(B.shape[1]), ny=int(Cm.shape[0]),
                  device_ms_per_freq=statistics.median(td), host_ms_per_freq=statistics.median(th),
                  device_ms_all=[round(v, 2) for v in td], host_ms_all=[round(v, 2) for v in th],
                  faster="device" if statistics.median(td) < statistics.median(th) else "host",
                  iters_min=int(info["iters"].min()), iters_max=int(info["iters"].max()),
                  worst_relres=float(info["relres"].max()), rel_distance_device_host=dist, trials=args.trials,
                  threads=os.environ.get("OMP_NUM_THREADS")))
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
