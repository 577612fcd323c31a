"""Newton-ADI against RADI at cfg2 (N = 58, the benchmark's B, W and shift list) on one context, device-resident
panels: steps, shift solves, GMRES iterations, wall-clock to the gain K and final column count of both paths, and
their distance to the oracle's K (tests/golden/cfg2_golden.npz).  Not a pass/fail gate: the lines it prints (JSON,
one per path and tolerance, then a summary) are the record behind DESIGN.md section 3d.

RADI runs twice per tolerance: with the benchmark's shift list cycled ("radi") and with the shifts generated from the
iteration ("radi-ham": ms='hamiltonian'; its lines also carry the fallback count and the shifts).

Both paths start from zero, with the per-shift cache cleared before every call (the setup is part of the call), and
end with K on the host.  RADI runs at several residual tolerances; the one compared is the loosest whose K is as
close to the fixture as Newton's (within 10 %), else the tightest.  Timings: one warm-up call of every variant, then
the variants alternate for --trials rounds; median and best of the host clock around calls that end synchronised.

With --sweep-width W [W ...] the cycled list also runs in sweeps of those widths ("radi-sweepW": radi_dict['sweep_width'],
DESIGN.md 3d-3), in the same process and alternating with the others; their lines carry the effective width, the
sweeps and the solves issued, and a "summary-sweeps" line per tolerance compares them with width 1.

With --gen-sweep-width W [W ...] the generated shifts also run in sweeps of up to W solves ("radi-hamsweepW":
ms='hamiltonian-sweep'), alternating with the others; their lines carry the cap, the sweeps, the solves
of every sweep and the shifts, and a "summary-gen-sweeps" line per tolerance compares them with 'hamiltonian', with the
cycled list at the widest --sweep-width and with Newton-ADI.  --only PREFIX [PREFIX ...] runs just the variants whose
names start so and prints no summaries (for a RICADI_TIMING=1 run of a few variants).

python tools/radi_compare.py [--N 58] [--trials 5] [--sweep-width 2 4 8] [--gen-sweep-width 2 4 8]
                             [--out profiles/radi_cfg2.json]"""
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
    ap.add_argument("--shifts", type=int, default=16)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--tols", type=float, nargs="+", default=[1e-6, 1e-7, 1e-8, 1e-10, 1e-12])
    ap.add_argument("--sweep-width", type=int, nargs="*", default=[])
    ap.add_argument("--gen-sweep-width", type=int, nargs="*", default=[])
    ap.add_argument("--only", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import sadptprj_riclyap_adi.lin_alg_utils as lau
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    from optconpy_amd import backend, problems as pb

    pr = pb.ricc_problem(args.N, args.nu, NU=4, NY=4, alphau=1e-2)
    mct = lau.app_prj_via_sadpnt(amat=pr.M, jmat=pr.J, rhsv=pr.mc_mat.T, transposedprj=True)
    tb = lau.apply_invsqrt_fromright(pr.rmat, pr.b_mat, output="dense")
    trct = lau.apply_invsqrt_fromright(pr.y_masmat, mct, output="dense")
    ms = pb.logshifts(1.0, 3e3, args.shifts)
    F = (-pr.A - pr.Nc).tocsr()
    MT = pr.M.T.tocsr()
    K_ref = None
    g = np.load(os.path.join(ROOT, "tests", "golden", "cfg2_golden.npz"))
    if int(g["cfg"][0]) == args.N and len(g["shifts"]) == len(ms) and np.allclose(g["shifts"], ms, rtol=1e-14):
        K_ref = g["K_ric"]
    tb_d, trct_d = pru.to_device(tb), pru.to_device(trct)
    ctx = backend.context_for(F.T.tocsr(), MT, pr.J)
    dist = lambda K: None if K_ref is None else float(np.linalg.norm(K - K_ref) / np.linalg.norm(K_ref))

    def newton():
        ctx.clear_cache()
        d = dict(pb.default_nwtn_adi_dict(), ms=ms, sweep_width=16)
        out = pru.proj_alg_ric_newtonadi(mmat=pr.M, amat=F, jmat=pr.J, bmat=tb_d, wmat=trct_d, nwtn_adi_dict=d)
        K = -pru.get_mTzzTtb(MT, out["zfac"], tb_d)
        return K, dict(path="newton-adi", steps=out["adi_steps"], newton_steps=out["nwtn_steps"],
                       shift_solves=out["shift_solves"], gmres_iters=out["gmres_iters"], cols=out["zfac"].shape[1],
                       nonconverged=out["gmres_nonconverged"])

    def radi(tol, generated=False, width=1):
        gensweep = generated and width > 1
        def run():
            ctx.clear_cache()
            out = pru.proj_alg_ric_radi(mmat=pr.M, amat=F, jmat=pr.J, bmat=tb_d, wmat=trct_d,
                                        radi_dict=dict(ms="hamiltonian-sweep" if gensweep else "hamiltonian" if generated
                                                       else ms, radi_res_reltol=tol, radi_max_steps=400,
                                                       sweep_width=width))
            info = dict(path="radi-hamsweep%d" % width if gensweep else "radi-ham" if generated else "radi" if width == 1
                        else "radi-sweep%d" % width,
                        radi_res_reltol=tol, steps=out["radi_steps"], sweep_width=out["sweep_width"],
                        sweeps=out["sweeps"],
                        shift_solves=out["shift_solves"], gmres_iters=out["gmres_iters"],
                        cols=out["zfac"].shape[1], nonconverged=out["gmres_nonconverged"],
                        stop_rule=out["stop_rule"], last_res=float(out["res_hist"][-1]))
            if generated:
                info.update(shift_fallbacks=out["shift_fallbacks"], shifts=[float(p) for p in out["ms"]])
            if gensweep:
                info.update(sweep_widths=out["sweep_widths"])
            return -out["gain"], info
        return run

    variants = ([("newton-adi", newton)] + [("radi %g" % t, radi(t)) for t in args.tols]
                + [("radi-ham %g" % t, radi(t, generated=True)) for t in args.tols]
                + [("radi-sweep%d %g" % (w, t), radi(t, width=w)) for w in args.sweep_width if w > 1 for t in args.tols]
                + [("radi-hamsweep%d %g" % (w, t), radi(t, generated=True, width=w)) for w in args.gen_sweep_width if w > 1
                   for t in args.tols])
    if args.only:
        variants = [v for v in variants if any(v[0].startswith(p) for p in args.only)]
    rec, times = {}, {name: [] for name, _ in variants}
    for name, fn in variants:                         # warm-up: every shape the timed calls use
        K, info = fn()
        info["K_vs_fixture"] = dist(K)
        rec[name] = info
    for _ in range(args.trials):
        for name, fn in variants:
            t0 = time.perf_counter()
            fn()
            times[name].append(1e3 * (time.perf_counter() - t0))
    lines = []
    for name, _ in variants:
        rec[name].update(N=args.N, n=pr.NV + pr.NP, ms_median=statistics.median(times[name]), ms_best=min(times[name]),
                         ms_all=[round(t, 2) for t in times[name]], trials=args.trials)
        lines.append(rec[name])
    if args.only:
        print("\n".join(json.dumps(l) for l in lines))
        return
    nd = rec["newton-adi"]["K_vs_fixture"]
    pick = None
    for t in sorted(args.tols, reverse=True):
        r = rec["radi %g" % t]
        if nd is None or r["K_vs_fixture"] <= 1.1 * nd:
            pick = r
            break
    pick = pick or rec["radi %g" % min(args.tols)]
    nt, rt = rec["newton-adi"]["ms_median"], pick["ms_median"]
    lines.append(dict(path="summary", compared_radi_res_reltol=pick["radi_res_reltol"], newton_ms=nt, radi_ms=rt,
                      newton_K_vs_fixture=nd, radi_K_vs_fixture=pick["K_vs_fixture"],
                      faster="radi" if rt < nt else "newton-adi", ratio=max(rt, nt) / min(rt, nt)))
    for t in args.tols:                               # generated shifts against the cycled list, tolerance by tolerance
        c, h = rec["radi %g" % t], rec["radi-ham %g" % t]
        lines.append(dict(path="summary-shifts", radi_res_reltol=t, cycled_steps=c["steps"], generated_steps=h["steps"],
                          cycled_ms=c["ms_median"], generated_ms=h["ms_median"], newton_ms=nt,
                          generated_K_vs_fixture=h["K_vs_fixture"],
                          faster="generated" if h["ms_median"] < c["ms_median"] else "cycled"))
    for t in args.tols:                               # sweeps against width 1, tolerance by tolerance
        c = rec["radi %g" % t]
        for w in args.sweep_width:
            if w > 1:
                r = rec["radi-sweep%d %g" % (w, t)]
                lines.append(dict(path="summary-sweeps", radi_res_reltol=t, asked=w, sweep_width=r["sweep_width"],
                                  steps=r["steps"], shift_solves=r["shift_solves"], gmres_iters=r["gmres_iters"],
                                  ms=r["ms_median"], width1_ms=c["ms_median"], width1_steps=c["steps"],
                                  width1_gmres_iters=c["gmres_iters"], K_vs_fixture=r["K_vs_fixture"],
                                  speedup=c["ms_median"] / r["ms_median"]))
    wmax = max([w for w in args.sweep_width if w > 1], default=None)
    for t in args.tols:                               # generated shifts in sweeps against one per step, tolerance by tolerance
        h = rec["radi-ham %g" % t]
        for w in args.gen_sweep_width:
            if w > 1:
                r = rec["radi-hamsweep%d %g" % (w, t)]
                cyc = None if wmax is None else rec["radi-sweep%d %g" % (wmax, t)]
                lines.append(dict(path="summary-gen-sweeps", radi_res_reltol=t, asked=w, cap=r["sweep_width"],
                                  steps=r["steps"], sweeps=r["sweeps"], shift_solves=r["shift_solves"],
                                  sweep_widths=r["sweep_widths"], gmres_iters=r["gmres_iters"], ms=r["ms_median"],
                                  ms_spread=[min(r["ms_all"]), max(r["ms_all"])], fallbacks=r["shift_fallbacks"],
                                  one_per_step_ms=h["ms_median"], one_per_step_steps=h["steps"],
                                  one_per_step_gmres_iters=h["gmres_iters"],
                                  cycled_sweep_ms=None if cyc is None else cyc["ms_median"],
                                  cycled_sweep_width=wmax, cycled_sweep_steps=None if cyc is None else cyc["steps"],
                                  newton_ms=nt, K_vs_fixture=r["K_vs_fixture"],
                                  speedup_vs_one_per_step=h["ms_median"] / r["ms_median"]))
    text = "\n".join(json.dumps(l) for l in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
