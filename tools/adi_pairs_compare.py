"""Real shifts against complex-conjugate shift pairs in the low-rank Lyapunov ADI at cfg2's operator (N = 58, the
benchmark's W), step form, through the drop-in: ``solve_proj_lyap_stein`` with ``ms='auto'`` and with
``ms='auto-complex'``.  Per variant: the shift list, steps, shift solves, GMRES iterations,
pair statistics, the factored residual and wall-clock -- one warm-up call of each, then the variants alternate for
--trials rounds, median and best of the host clock around calls that end with the factor on the host.  The per-shift
cache is cleared before every call: shift generation and setup are part of the call, for both variants alike.

Not a pass/fail gate: the JSON lines it prints (one per variant, then a summary) are the record behind the table of
DESIGN.md 3g.  With --out every line is also appended to that file as soon as it is known.

python tools/adi_pairs_compare.py [--N 58] [--trials 5] [--num-shifts 8] [--out profiles/adi_pairs_cfg2.json]"""
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
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--num-shifts", type=int, default=8)
    ap.add_argument("--max-steps", type=int, default=200)
    ap.add_argument("--newz-reltol", type=float, default=1e-8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import sadptprj_riclyap_adi.lin_alg_utils as lau
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    from optconpy_amd import backend, problems as pb

    pr = pb.ricc_problem(args.N, args.nu, NU=4, NY=4, alphau=1e-2)
    mct = lau.app_prj_via_sadpnt(amat=pr.M, jmat=pr.J, rhsv=pr.mc_mat.T, transposedprj=True)
    trct = lau.apply_invsqrt_fromright(pr.y_masmat, mct, output="dense")
    F = (-pr.A - pr.Nc).tocsr()
    ctx = backend.context_for(F.T.tocsr(), pr.M.T.tocsr(), pr.J)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").close()

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")

    def variant(ms):
        def run():
            ctx.clear_cache()
            d = dict(ms=ms, sweep_width=1, adi_max_steps=args.max_steps, adi_newZ_reltol=args.newz_reltol,
                     num_shifts=args.num_shifts, check_lyap_res=True)
            out = pru.solve_proj_lyap_stein(amat=F, mmat=pr.M, jmat=pr.J, wmat=trct, adi_dict=d)
            pi = out.get("pair_info", [0, 0, 0, 0])
            return dict(ms=ms, shifts=[[float(np.real(p)), float(np.imag(p))] for p in out["ms"]],
                        candidates=out["shift_info"]["candidates"], steps=out["adi_steps"],
                        shift_solves=out["shift_solves"], gmres_iters=out["gmres_iters"], pairs=pi[0],
                        pair_lockstep_iters=pi[1], pair_missed=pi[3], nonconverged=out["gmres_nonconverged"],
                        stopped_by=out["adi_stopped_by"], cols=out["zfac"].shape[1], rel_newZ=out["adi_rel_newZ"],
                        lyap_res=out["lyap_res"], res_fro=out["res_fro"])
        return run

    variants = [("auto", variant("auto")), ("auto-complex", variant("auto-complex"))]
    rec, times = {}, {name: [] for name, _ in variants}
    for name, fn in variants:                         # warm-up: every shape the timed calls use
        t0 = time.perf_counter()
        rec[name] = fn()
        rec[name]["ms_warmup"] = 1e3 * (time.perf_counter() - t0)
        emit(dict(rec[name], path="warm-up", N=args.N, n=pr.NV + pr.NP))
    for _ in range(args.trials):
        for name, fn in variants:
            t0 = time.perf_counter()
            fn()
            times[name].append(1e3 * (time.perf_counter() - t0))
    for name, _ in variants:
        rec[name].update(path="timed", N=args.N, n=pr.NV + pr.NP, ms_median=statistics.median(times[name]),
                         ms_best=min(times[name]), ms_all=[round(t, 2) for t in times[name]], trials=args.trials)
        emit(rec[name])
    a, c = rec["auto"], rec["auto-complex"]
    emit(dict(path="summary", auto_steps=a["steps"], complex_steps=c["steps"], auto_solves=a["shift_solves"],
              complex_solves=c["shift_solves"], auto_gmres_iters=a["gmres_iters"], complex_gmres_iters=c["gmres_iters"],
              auto_ms=a["ms_median"], complex_ms=c["ms_median"],
              faster="auto-complex" if c["ms_median"] < a["ms_median"] else "auto",
              ratio=max(a["ms_median"], c["ms_median"]) / min(a["ms_median"], c["ms_median"])))


if __name__ == "__main__":
    main()
