#!/usr/bin/env python
"""The cfg4-dre sweep of bench.py (same generator calls) once with Newton-ADI and once with ``ric_solver='radi'``
(``ms='hamiltonian-dominant'``) in one job, after one warm-up sweep of each.

Writes one JSON line per variant to profiles/dre_radi_cfg4.jsonl: seconds per sweep, per time step the Riccati solve's
seconds, steps, shift solves, GMRES iterations and the width of W, RADI's fallbacks, and the relative distance of every
time's gain and w from the other variant's.

    python tools/dre_compare.py --nts 2 [--N 106] [--nu 0.0025] [--radi-max-steps 200] [--out profiles/dre_radi_cfg4.jsonl]

With ``--radi-sweep-width W`` a third variant runs beside the two: ``ms='hamiltonian-sweep'`` at that width (DESIGN.md
3d-4; the cap of a step is min(W, 128 // columns of W, ...): 2 at 58 columns); its line carries the sweeps and the solves
of every sweep per time step, and every variant's distances are to Newton-ADI (Newton-ADI's to RADI).  ``--append``
adds the lines to ``--out`` instead of replacing it:

    python tools/dre_compare.py --nts 2 --radi-sweep-width 8 --append --out profiles/dre_radi_sweep_cfg4.jsonl

``radi_max_steps`` bounds the factor the RADI call reserves (radi_max_steps x columns of W x NV doubles: 8.3 GB at 58
columns, NV = 89 042 and 200 steps; the cfg4-dre steps need up to 143); the line reports the steps the runs needed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nts", type=int, default=2, choices=[2, 3])
    ap.add_argument("--N", type=int, default=106)
    ap.add_argument("--nu", type=float, default=0.15 / 60.0)
    ap.add_argument("--shifts", type=int, default=64)
    ap.add_argument("--radi-max-steps", type=int, default=200)
    ap.add_argument("--radi-res-reltol", type=float, default=1e-10)
    ap.add_argument("--radi-sweep-width", type=int, default=0)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "dre_radi_cfg4.jsonl"))
    args = ap.parse_args()

    import sadptprj_riclyap_adi.lin_alg_utils as lau
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    from optconpy_amd import backend, problems as pb
    from optconpy_amd.dae_ric import MemoryStore, solve_flow_daeric

    # the problem of bench.py --workload cfg4-dre
    nu, Nts = args.nu, args.nts
    pr = pb.ricc_problem(args.N, nu, NU=4, NY=4, alphau=1e-2)
    mct = lau.app_prj_via_sadpnt(amat=pr.M, jmat=pr.J, rhsv=pr.mc_mat.T, transposedprj=True)
    tmesh = pb.get_tint(0.0, 1.0, Nts, True)
    nad = dict(pb.default_nwtn_adi_dict(), ms=pb.logshifts(0.5, 2e3, args.shifts, interleave=True))
    radi_dict = dict(ms="hamiltonian-dominant", radi_max_steps=args.radi_max_steps,
                     radi_res_reltol=args.radi_res_reltol)
    radi_dicts = {"radi": radi_dict}
    if args.radi_sweep_width > 0:
        radi_dicts["radi-sweep"] = dict(radi_dict, ms="hamiltonian-sweep", sweep_width=args.radi_sweep_width)
    NY2 = mct.shape[1]

    def ystar(t):
        return (0.1 * np.sin(5 * np.pi * t) * np.arange(1, NY2 + 1)).reshape(-1, 1)

    def tdpart(time=None, **kw):
        return (1.0 + 0.5 * np.sin(2 * np.pi * time)) * pr.Nc, np.zeros((pr.NV, 1))

    rec = []

    class Timed:
        def __getattr__(self, name):
            f = getattr(pru, name)
            if name not in ("proj_alg_ric_newtonadi", "proj_alg_ric_radi"):
                return f

            def g(*a, **k):
                t0 = time.perf_counter()
                o = f(*a, **k)
                r = dict(seconds=round(time.perf_counter() - t0, 3), shift_solves=int(o["shift_solves"]),
                         gmres_iters=int(o["gmres_iters"]), w_cols=int(k["wmat"].shape[1]),
                         nonconverged=int(o["gmres_nonconverged"]))
                if name == "proj_alg_ric_radi":
                    r.update(steps=int(o["radi_steps"]), fallbacks=int(o["shift_fallbacks"]),
                             res_rel=float(o["res_hist"][-1]), stop_rule=int(o["stop_rule"]))
                    if "sweep_widths" in o:
                        r.update(sweep_cap=int(o["sweep_width"]), sweeps=int(o["sweeps"]),
                                 sweep_widths=[int(v) for v in o["sweep_widths"]])
                else:
                    r.update(steps=int(o["adi_steps"]), newton_steps=int(o["nwtn_steps"]))
                rec.append(r)
                print("[dre_compare] %s time step %d of %d: %s" % (name, len(rec), Nts, r), file=sys.stderr, flush=True)
                return o
            return g

    count = [0]

    def sweep(solver):
        count[0] += 1
        tag = count[0]
        kw = dict(mmat=pr.M, amat=pr.A, jmat=pr.J, bmat=pr.b_mat, mcmat=mct.T, v_is_my=True, rmat=pr.rmat,
                  vmat=pr.y_masmat, rhsv=np.zeros((pr.NV, 1)), gamma=1e-1, tmesh=tmesh, ystarvec=ystar,
                  nwtn_adi_dict=nad, comprz_thresh=5e-5, comprz_maxc=50, get_tdpart=tdpart,
                  get_datastr=lambda time=None, **k: "dre%d_t%.6f" % (tag, time), gtdtstrargs={})
        if solver in radi_dicts:
            kw.update(ric_solver="radi", radi_dict=radi_dicts[solver])
        del rec[:]
        store = MemoryStore()
        t0 = time.perf_counter()
        fb = solve_flow_daeric(store=store, pru=Timed(), lau=lau, **kw)
        el = time.perf_counter() - t0
        outs = {t: (np.asarray(store.load(fb[t]["mtxtb"])), np.asarray(store.load(fb[t]["w"]))) for t in tmesh}
        return el, list(rec), outs

    results = {}
    for solver in ["newton-adi"] + list(radi_dicts):
        sweep(solver)                                            # warm-up
        results[solver] = sweep(solver)

    def rel(a, b):
        return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))

    info = backend.context().setup_info()
    lines = []
    for solver, other in [("newton-adi", "radi")] + [(v, "newton-adi") for v in radi_dicts]:
        el, steps, outs = results[solver]
        line = dict(variant=solver, workload="cfg4-dre", N=args.N, n=int(pr.NV + pr.NP), nts=Nts,
                    seconds_per_sweep=round(el, 3), seconds_in_riccati=round(sum(r["seconds"] for r in steps), 3),
                    time_steps=steps, shift_solves=sum(r["shift_solves"] for r in steps),
                    gmres_iters=sum(r["gmres_iters"] for r in steps), w_cols=[r["w_cols"] for r in steps],
                    gain_rel_to_other=[rel(outs[t][0], results[other][2][t][0]) for t in tmesh],
                    w_rel_to_other=[rel(outs[t][1], results[other][2][t][1]) for t in tmesh],
                    preconditioner_levels=info["levels"])
        if solver in radi_dicts:
            line.update(fallbacks=sum(r["fallbacks"] for r in steps), radi_dict=radi_dicts[solver],
                        radi_steps_needed=max(r["steps"] for r in steps))
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as fh:
        for line in lines:
            s = json.dumps(line)
            fh.write(s + "\n")
            print(s)


if __name__ == "__main__":
    main()
