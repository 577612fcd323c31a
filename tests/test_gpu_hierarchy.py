"""The fine hierarchy on the device (``hierarchy=1``): structure against the host plan, the V-cycle against the FP64
model of tests/hierarchy_model.py built from the device's own structure, batched solves, the iteration count against
the default rule at cfg2's mesh, and the drop-in.  The shapes and the forced ``coarse_max`` are those of
tests/test_hierarchy_cpu.py (N = 30: 150 -> 3 levels, 100 -> 4 levels; N = 15: 30 -> 4 levels); the parity bounds are the
rule of tests/test_gpu_precond_parity.py and tests/test_gpu_vanka.py (precond_model.TOL_ROUNDED / tol_fp64)."""
import os

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

from optconpy_amd import _lib, problems as pb
import hierarchy_model as hm
import precond_model as pm
import vanka_model as vm

pytestmark = pytest.mark.gpu
CM = hm.COARSE_MAX
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCT_ARRAYS = ("bv_ptr", "bv_rows", "bp_ptr", "bp_rows", "aggof")
STRUCT_SCALARS = ("nv", "np", "nbv", "nbp", "bs", "kc", "kcv", "kcp", "smoothed", "child", "folded", "rect",
                  "precond32", "agg_v", "agg_p")


@pytest.fixture(scope="module")
def n30():
    pr = pb.ricc_problem(30, 0.05)
    return pr, (-pr.A - pr.Nc).T.tocsr(), pr.M.T.tocsr(), pr.J.tocsr()


def _structures(ctx):
    out = [ctx.precond_structure(0)]
    while out[-1]["child"]:
        out.append(ctx.precond_structure(len(out)))
    return out


def _same_structure(a, b):
    assert all(a[k] == b[k] for k in STRUCT_SCALARS), [(k, a[k], b[k]) for k in STRUCT_SCALARS if a[k] != b[k]]
    assert all(np.array_equal(a[k], b[k]) for k in STRUCT_ARRAYS)
    assert (a["P"] is None) == (b["P"] is None) and (a["P"] is None or abs(a["P"] - b["P"]).max() == 0.0)


def _apply(ctx, shifts, betas, R):
    import torch
    G, n, m = R.shape
    Rd = torch.from_numpy(R).cuda()
    Zd = torch.full((G, n, m), float("nan"), dtype=torch.float64, device="cuda")
    form = ctx.precond_apply_batch_dev(shifts, betas, Rd.data_ptr(), n * m, m, Zd.data_ptr())
    ctx.synchronize()
    return Zd.cpu().numpy(), form


def _solve(ctx, alphas, betas, R):
    import torch
    Rd = torch.as_tensor(R).cuda()
    X = torch.empty(len(alphas), ctx.n, R.shape[1], dtype=torch.float64, device="cuda")
    its, rr = ctx.shift_solve_batch_dev(alphas, betas, Rd.data_ptr(), 0, R.shape[1], X.data_ptr())
    ctx.synchronize()
    return list(its), np.asarray(rr), X.cpu().numpy()


# ----------------------------------------------------------------------------- 1. structure
@pytest.mark.parametrize("levels", [3, 4])
def test_structure_agrees_with_the_host_plan(n30, levels):
    pr, calA, calE, J = n30
    cm = CM[30][levels]
    plan = _lib.host_plan_hierarchy(calA, calE, J, hierarchy=1, coarse_max=cm)
    assert len(plan) == levels
    for cs in (0, 1):
        with _lib.Context(0, hierarchy=1, coarse_max=cm, child_smoother=cs) as ctx:
            ctx.set_operator(calA, calE, J)
            info = ctx.setup_info()
            sts = _structures(ctx)
            vps = [ctx.precond_vanka(l) for l in range(levels)]
            with pytest.raises(ValueError):
                ctx.precond_structure(levels)
        assert (info["hierarchy"], info["hierarchy_levels"], info["hierarchy_dense"]) == (1, levels, plan[-1]["dense_dim"])
        assert info["levels"] == levels + 1 and info["dense_coarse"] == plan[-1]["dense_dim"]   # (counts the dense problem)
        assert len(sts) == levels
        for st, row in zip(sts, plan):
            got = dict(nv=st["nv"], np=st["np"], kv=st["kcv"], kp=st["kcp"], agg_v=st["agg_v"], agg_p=st["agg_p"],
                       has_child=int(st["child"]), dense_dim=0 if st["child"] else st["kc"], smoothed=st["smoothed"])
            assert got == row, (got, row)
        # the smoother option reaches every child level, and only child levels
        assert vps[0]["patches"] == 0
        assert all((vp["pressure_patches"] == st["np"]) if cs else (vp["patches"] == 0) for vp, st in zip(vps[1:], sts[1:]))
        assert info["child_smoother"] == cs


def test_default_structure_untouched(n30, monkeypatch):
    """``hierarchy=0`` is the default: the same structure and setup report as a context that never set the field, with
    and without a child level (``RICADI_SA=0`` lets this operator have one, as in tests/test_gpu_vanka.py)."""
    pr, calA, calE, J = n30
    for sa in (None, "0"):
        if sa is not None:
            monkeypatch.setenv("RICADI_SA", sa)
        got = []
        for opts in (dict(coarse_max=300), dict(coarse_max=300, hierarchy=0)):
            with _lib.Context(0, **opts) as ctx:
                ctx.set_operator(calA, calE, J)
                got.append((ctx.setup_info(), _structures(ctx)))
        assert got[0][0] == got[1][0] and got[0][0]["hierarchy"] == 0
        assert len(got[0][1]) == len(got[1][1]) == (1 if sa is None else 2)
        for a, b in zip(got[0][1], got[1][1]):
            _same_structure(a, b)
        plan = _lib.host_plan_hierarchy(calA, calE, J, coarse_max=300) if sa is None else None
        if plan:
            assert (plan[0]["kv"], plan[0]["kp"], plan[0]["agg_v"]) == (got[0][1][0]["kcv"], got[0][1][0]["kcp"],
                                                                        got[0][1][0]["agg_v"])


# ----------------------------------------------------------------------------- 2. cycle parity
SHIFTS = [-1.0, -30.0, -1000.0]


@pytest.mark.parametrize("smoother", [0, 1])
@pytest.mark.parametrize("levels", [3, 4])
def test_cycle_parity(n30, monkeypatch, levels, smoother):
    """The batch form (reduced storage: against the model rounded where the device rounds, TOL_ROUNDED per block) and
    the FP64 host entry with FP64-stored operands (against the exact model, tol_fp64), m = 16, three shifts; two
    identical applications agree bitwise."""
    pr, calA, calE, J = n30
    opts = dict(hierarchy=1, coarse_max=CM[30][levels], child_smoother=smoother)
    with _lib.Context(0, **opts) as ctx:
        ctx.set_operator(calA, calE, J)
        R = np.random.default_rng(10 * levels + smoother).standard_normal((len(SHIFTS), ctx.n, 16))
        Z, form = _apply(ctx, SHIFTS, [1.0] * 3, R)
        Z2, _ = _apply(ctx, SHIFTS, [1.0] * 3, R)
        model, sts = hm.from_context(ctx, calA, calE, J)
    chain = hm.chain(model)
    assert len(chain) == levels and form["coarse"] == "child"
    assert all(isinstance(l, vm.VankaModel) == bool(smoother) for l in chain[1:])
    form["precond32"] = sts[0]["precond32"]
    assert form["precond32"]
    for g, p in enumerate(SHIFTS):
        assert np.all(np.isfinite(Z[g])) and np.array_equal(Z[g], Z2[g]), ("two applications differ", g)
        e = float(pm.block_errors(Z[g], model.apply(p, 1.0, R[g], rounded=form), model.st).max())
        tol = max(pm.TOL_ROUNDED, pm.tol_fp64(model, p, 1.0))
        print("[hierarchy parity] %d levels, smoother %d, batch form, shift %g: worst per-block error %.2e (tolerance %.2e)"
              % (levels, smoother, p, e, tol))
        assert e <= tol, (g, e, tol)
    monkeypatch.setenv("RICADI_PRECOND64", "1")
    with _lib.Context(0, **opts) as ctx:
        ctx.set_operator(calA, calE, J)
        assert not ctx.precond_structure(levels - 1)["precond32"]
        for g, p in enumerate(SHIFTS):
            Zh = ctx.precond_apply(p, 1.0, R[g])
            assert np.array_equal(Zh, ctx.precond_apply(p, 1.0, R[g]))
            e = float(pm.block_errors(Zh, model.apply(p, 1.0, R[g]), model.st).max())
            t64 = pm.tol_fp64(model, p, 1.0)
            print("[hierarchy parity] %d levels, smoother %d, FP64 host entry, shift %g: worst per-block error %.2e "
                  "(tol_fp64 %.2e)" % (levels, smoother, p, e, t64))
            assert e <= t64, (g, e, t64)


# ----------------------------------------------------------------------------- 3. solve
@pytest.mark.parametrize("smoother", [0, 1])
def test_batched_solve_four_levels(n30, smoother):
    """Eight shifts and the projection operator (alpha, beta) = (1, 0) in one lockstep batch, 16 columns: every
    column at 1e-10, J V = 0, and the solutions of a sparse LU of the assembled saddle matrices."""
    pr, calA, calE, J = n30
    ms = [float(p) for p in pb.logshifts(1.0, 1e3, 8)]
    alphas, betas = ms + [1.0], [1.0] * 8 + [0.0]
    R = np.random.default_rng(6).standard_normal((pr.NV, 16))
    bn = np.linalg.norm(R, axis=0)
    with _lib.Context(0, hierarchy=1, coarse_max=CM[30][4], child_smoother=smoother) as ctx:
        ctx.set_operator(calA, calE, J)
        assert ctx.setup_info()["hierarchy_levels"] == 4
        its, rr, X = _solve(ctx, alphas, betas, R)
    print("[hierarchy solve] smoother %d: iterations %s, worst relative residual %.2e" % (smoother, its, rr.max()))
    assert rr.max() <= 1e-10 * 1.0000001 and min(its) > 0, (rr.max(), its)
    rhs = np.vstack([R, np.zeros((pr.NP, 16))])
    for g, (a, b) in enumerate(zip(alphas, betas)):
        V, L = X[g, :pr.NV], X[g, pr.NV:]
        rv = b * (calA @ V) + a * (calE @ V) + J.T @ L - R
        rp = J @ V
        res = np.sqrt(np.linalg.norm(rv, axis=0) ** 2 + np.linalg.norm(rp, axis=0) ** 2) / bn
        S = sps.bmat([[b * calA + a * calE, J.T], [J, None]], format="csc")
        ref = spla.splu(S).solve(rhs)
        err = np.linalg.norm(X[g] - ref) / np.linalg.norm(ref)
        print("[hierarchy solve] group %d (%g, %g): true residual %.2e, |J V| / |V| %.2e, against the sparse LU %.2e"
              % (g, a, b, res.max(), np.abs(rp).max() / np.abs(V).max(), err))
        assert res.max() <= 1.05e-10, (g, res.max())
        assert np.abs(rp).max() <= 1e-9 * np.abs(V).max(), g
        assert err <= 1e-7, (g, err)


# ----------------------------------------------------------------------------- 4. iterations at cfg2's mesh
def test_iterations_against_the_default_rule_at_cfg2():
    """N = 58 (n = 29 930), ``coarse_max=600``, the 16 shifts of cfg2, 16 columns.  The default rule grows the aggregates
    of its two levels to (36, 54) (k = 807, smoothed prolongation), the fine rule keeps (16, 24) over a chain of three
    levels (1 817 -> 989 -> 575).  Measured on the MI355X, iterations per shift from |p| = 1 to 3 000:

        default      109 107 105 102  98  92  86  77  67  59  52  46  45  49  59  73   sum 1 226
        fine, SIMPLE 172 162 145 131 114  98  85  75  67  63  55  48  44  42  43  46   sum 1 390
        fine, Vanka  150 140 127 117 103  95  88  82  72  66  61  54  47  44  49  62   sum 1 357

    The fine hierarchy LOSES against the default rule at the small shifts (its children stand in for a dense inverse
    under a smoothed prolongation there) and wins at the large ones, so the sum is not below the default's; what is
    asserted is the ordering of the two child smoothers under ``hierarchy=1``: Vanka <= SIMPLE."""
    pr = pb.ricc_problem(58, 0.05, NU=4, NY=4, alphau=1e-2)
    calA, calE, J = (-pr.A - pr.Nc).T.tocsr(), pr.M.T.tocsr(), pr.J.tocsr()
    ms = [float(p) for p in pb.logshifts(1.0, 3e3, 16)]
    old = _lib.host_plan_hierarchy(calA, calE, J, coarse_max=600)
    fine = _lib.host_plan_hierarchy(calA, calE, J, coarse_max=600, hierarchy=1)
    print("[hierarchy iterations] default plan", old, "| fine plan", fine)
    assert old[0]["agg_v"] >= 36 and old[0]["agg_p"] >= 54 and len(fine) >= 3 and fine[0]["agg_v"] == 16
    R = np.random.default_rng(2).standard_normal((pr.NV, 16))
    its = {}
    for name, opts in (("default", dict()), ("fine_simple", dict(hierarchy=1, child_smoother=0)),
                       ("fine_vanka", dict(hierarchy=1, child_smoother=1))):
        with _lib.Context(0, coarse_max=600, **opts) as ctx:
            ctx.set_operator(calA, calE, J)
            its[name], rr, _ = _solve(ctx, ms, [1.0] * 16, R)
            assert ctx.setup_info()["hierarchy_levels"] == (len(fine) if opts else len(old))
        assert rr.max() <= 1e-10 * 1.0000001 and min(its[name]) > 0, (name, rr.max(), its[name])
        print("[hierarchy iterations] %s: per shift %s, sum %d" % (name, its[name], sum(its[name])))
    print("[hierarchy iterations] fine with the Vanka children against the default rule: %d / %d"
          % (sum(its["fine_vanka"]), sum(its["default"])))
    assert sum(its["fine_vanka"]) <= sum(its["fine_simple"]), its


# ----------------------------------------------------------------------------- 5. drop-in
def test_dropin_newton_adi_on_cfg1(cfg1, golden):
    """``backend.configure(hierarchy=1, coarse_max=30)``: the reference's Newton-ADI call on cfg1 (N = 15, four
    levels) gives the golden feedback gain at the parity bar of 1e-6."""
    from optconpy_amd import backend
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    pr, tb, trct, ms = cfg1
    F = (-pr.A - pr.Nc).tocsr()
    d = dict(pb.default_nwtn_adi_dict(), ms=ms)
    backend.configure(hierarchy=1, coarse_max=CM[15][4])
    try:
        out = pru.proj_alg_ric_newtonadi(mmat=pr.M, amat=F, jmat=pr.J, bmat=tb, wmat=trct, nwtn_adi_dict=d)
        info = backend.context().setup_info()
        K = -pru.get_mTzzTtb(pr.M.T, out["zfac"], tb)
    finally:
        backend.configure()
    assert backend._opts == {}
    assert (info["hierarchy"], info["hierarchy_levels"]) == (1, 4), info
    assert out["gmres_nonconverged"] == 0 and out["nwtn_steps"] == int(golden["nwtn_steps"][0])
    err = np.linalg.norm(K - golden["K_ric"]) / np.linalg.norm(golden["K_ric"])
    print("[hierarchy drop-in] K against the golden gain: %.2e" % err)
    assert err < 1e-6, err
