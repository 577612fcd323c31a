"""The coloured Vanka smoother of a child level on the device (``child_smoother=1``), on the problem of
``test_third_level_forced_small_problem``: N = 30, nu = 0.05, ``coarse_max=300``, ``RICADI_SA=0``, shifts
``logshifts(1, 1e3, 8)``, 16 columns.  The model of the child cycle is tests/vanka_model.py, built from the patches
the library exports; the parity tolerances are the rule of tests/test_gpu_precond_parity.py (precond_model)."""
import numpy as np
import pytest

from optconpy_amd import _lib, problems as pb
import precond_model as pm
import vanka_model as vm

pytestmark = pytest.mark.gpu

NEW_KEYS = ("child_smoother", "vanka_colours", "vanka_patches", "vanka_largest_patch", "vanka_dropped",
            "vanka_lone_patches")


@pytest.fixture(scope="module")
def n30():
    pr = pb.ricc_problem(30, 0.05)
    return pr, (-pr.A - pr.Nc).T.tocsr(), pr.M.T.tocsr(), pr.J.tocsr(), [float(p) for p in pb.logshifts(1.0, 1e3, 8)]


@pytest.fixture(autouse=True)
def _plain_aggregation(monkeypatch):
    monkeypatch.setenv("RICADI_SA", "0")


def _solve(ctx, ms, R):
    import torch
    Rd = torch.as_tensor(R).cuda()
    X = torch.empty(len(ms), ctx.n, R.shape[1], dtype=torch.float64, device="cuda")
    its, rr = ctx.shift_solve_batch_dev(ms, [1.0] * len(ms), Rd.data_ptr(), 0, R.shape[1], X.data_ptr())
    ctx.synchronize()
    return list(its), np.asarray(rr), X.cpu().numpy()


def _apply(ctx, shifts, betas, R, active=None):
    import torch
    G, n, m = R.shape
    Rd = torch.from_numpy(R).cuda()
    Zd = torch.full((G, n, m), float("nan"), dtype=torch.float64, device="cuda")
    form = ctx.precond_apply_batch_dev(shifts, betas, Rd.data_ptr(), n * m, m, Zd.data_ptr(), active=active)
    ctx.synchronize()
    return Zd.cpu().numpy(), form


def test_setup_info_and_default_unchanged(n30):
    pr, calA, calE, J, ms = n30
    R = np.random.default_rng(6).standard_normal((pr.NV, 16))
    got = {}
    for name, opts in (("none", dict(coarse_max=300)), ("off", dict(coarse_max=300, child_smoother=0)),
                       ("vanka", dict(coarse_max=300, child_smoother=1))):
        with _lib.Context(0, **opts) as ctx:
            ctx.set_operator(calA, calE, J)
            info = ctx.setup_info()
            its, rr, _ = _solve(ctx, ms, R)
            _, form = _apply(ctx, ms[:2], [1.0, 1.0], np.random.default_rng(1).standard_normal((2, ctx.n, 16)))
            child_np = ctx.precond_structure(1)["np"]
            got[name] = (info, its, form, child_np)
    i0, i1, iv = got["none"][0], got["off"][0], got["vanka"][0]
    assert i0["levels"] == i1["levels"] == iv["levels"] == 3
    assert all(i0[k] == 0 and i1[k] == 0 for k in NEW_KEYS), (i0, i1)
    assert (i0["levels"], i0["kc"]) == (i1["levels"], i1["kc"]) and got["none"][2] == got["off"][2]
    assert got["none"][1] == got["off"][1], (got["none"][1], got["off"][1])        # iteration counts: default unchanged
    assert iv["child_smoother"] == 1 and iv["vanka_colours"] >= 1 and iv["vanka_patches"] == got["vanka"][3]
    assert 2 <= iv["vanka_largest_patch"] <= 64
    assert got["vanka"][2]["coarse"] == "child" and not got["vanka"][2]["vanka"]   # the parent's form word is as ever
    print("setup_info with the Vanka child:", {k: iv[k] for k in NEW_KEYS})


def test_device_patches_equal_host_rule(n30):
    pr, calA, calE, J, ms = n30
    with _lib.Context(0, coarse_max=300, child_smoother=1) as ctx:
        ctx.set_operator(calA, calE, J)
        st0 = ctx.precond_structure(0)
        dev = ctx.precond_vanka(1)
        assert ctx.precond_vanka(0)["patches"] == 0
    cA, cE, cJ = vm.child_operators(st0, calA, calE, J)
    host = _lib.host_vanka_patches(cA.shape[0], cJ)
    for k in host:
        assert np.array_equal(host[k], dev[k]), k


def _parity(n30, monkeypatch, env, shifts, betas, m, active=None, seed=0):
    pr, calA, calE, J, _ = n30
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with _lib.Context(0, coarse_max=300, child_smoother=1) as ctx:
        ctx.set_operator(calA, calE, J)
        R = np.random.default_rng(seed).standard_normal((len(shifts), ctx.n, m))
        Z, form = _apply(ctx, shifts, betas, R, active)
        Z2, _ = _apply(ctx, shifts, betas, R, active)
        st0 = ctx.precond_structure(0)
        child = vm.VankaModel.from_context(ctx, *vm.child_operators(st0, calA, calE, J), level=1, omega=0.7)
        model = pm.CycleModel(calA, calE, J, st0, child=child)
    assert isinstance(child, vm.VankaModel) and model.levels() >= 2 and form["coarse"] == "child"
    form["precond32"] = st0["precond32"]
    groups = range(len(shifts)) if active is None else active
    for g in range(len(shifts)):
        if g not in groups:
            assert np.all(np.isnan(Z[g])), g
            continue
        assert np.all(np.isfinite(Z[g])), g
        assert np.array_equal(Z[g], Z2[g]), ("two applications differ", g)         # determinism: bitwise
        a, b = shifts[g], betas[g]
        t64 = pm.tol_fp64(model, a, b)
        reduced = form["h16"] or form["x32"] or form["mid32"] or form["b16"] or form["precond32"]
        ref = model.apply(a, b, R[g], rounded=form if reduced else None)
        e = pm.block_errors(Z[g], ref, model.st)
        tol = max(pm.TOL_ROUNDED, t64) if reduced else t64
        print("[vanka parity] env %s group %d shift %g: worst per-block error %.2e (tolerance %.2e)" % (
            env, g, a, float(e.max()), tol))
        assert float(e.max()) <= tol, (g, float(e.max()), tol)
    return form


def test_parity_single_and_batch(n30, monkeypatch):
    """One shift, then the batch form: 8 shifts of which 1, 4 and 7 are active; then a panel that is not 16 wide."""
    _parity(n30, monkeypatch, {}, [-3.0], [1.0], 16, seed=1)
    ms = n30[4]
    _parity(n30, monkeypatch, {}, ms, [1.0] * 4 + [0.5] + [1.0] * 3, 16, active=[1, 4, 7], seed=2)
    _parity(n30, monkeypatch, {}, ms[:2], [1.0, 1.0], 5, seed=3)


def test_parity_fp64_stored_inverses(n30, monkeypatch):
    """``RICADI_PRECOND64=1``: the batch form (FP16 input, FP32 output: against the rounded model), then the host
    entry ``ctx.precond_apply`` -- FP64 in and out, FP64 inverses -- against the exact model at ``tol_fp64``."""
    form = _parity(n30, monkeypatch, {"RICADI_PRECOND64": "1"}, [-1.0, -50.0, -1000.0], [1.0, 1.0, 0.5], 16, seed=4)
    assert not form["precond32"]
    pr, calA, calE, J, _ = n30
    with _lib.Context(0, coarse_max=300, child_smoother=1) as ctx:
        ctx.set_operator(calA, calE, J)
        R = np.random.default_rng(11).standard_normal((ctx.n, 7))
        st0 = ctx.precond_structure(0)
        assert not st0["precond32"]
        child = vm.VankaModel.from_context(ctx, *vm.child_operators(st0, calA, calE, J), level=1, omega=0.7)
        model = pm.CycleModel(calA, calE, J, st0, child=child)
        for p in (-3.0, -700.0):
            Z = ctx.precond_apply(p, 1.0, R)
            e = float(pm.block_errors(Z, model.apply(p, 1.0, R), model.st).max())
            t64 = pm.tol_fp64(model, p, 1.0)
            print("[vanka parity] FP64 host entry, shift %g: worst per-block error %.2e (tol_fp64 %.2e)" % (p, e, t64))
            assert e <= t64, (p, e, t64)


def test_end_to_end_iterations_not_above_simple_child(n30):
    """Batched solves meet 1e-10 in the true residual and J V = 0; the sum of iterations over the 8 shifts with the
    Vanka child is at most the sum with the SIMPLE child (the unchanged default path) -- a count, no margin."""
    pr, calA, calE, J, ms = n30
    R = np.random.default_rng(6).standard_normal((pr.NV, 16))
    bn = np.linalg.norm(R, axis=0)
    its = {}
    for cs in (0, 1):
        with _lib.Context(0, coarse_max=300, child_smoother=cs) as ctx:
            ctx.set_operator(calA, calE, J)
            assert ctx.setup_info()["levels"] == 3
            its[cs], rr, X = _solve(ctx, ms, R)
        assert rr.max() <= 1e-10 * 1.0000001 and min(its[cs]) > 0, (cs, rr.max(), its[cs])    # no unconverged solve
        for g, p in enumerate(ms):
            V, L = X[g, :pr.NV], X[g, pr.NV:]
            rv = calA @ V + p * (calE @ V) + J.T @ L - R
            rp = J @ V
            res = np.sqrt(np.linalg.norm(rv, axis=0) ** 2 + np.linalg.norm(rp, axis=0) ** 2) / bn
            assert res.max() <= 1.05e-10, (cs, g, res.max())
            assert np.abs(rp).max() <= 1e-9 * np.abs(V).max()
    print("iterations per shift: SIMPLE child", its[0], "sum", sum(its[0]), "| Vanka child", its[1], "sum", sum(its[1]))
    assert sum(its[1]) <= sum(its[0]), (its[1], its[0])


def test_dropin_configure(n30):
    """``backend.configure(child_smoother=1, coarse_max=300)`` reaches the drop-in's ADI: the factor's
    ``comp_proj_lyap_res_norm`` agrees with the CPU oracle's ADI of the same steps as the existing ADI parity test
    asks (test_gpu_parity.py: rtol 1e-7), and ``backend.configure()`` restores the default."""
    from optconpy_amd import backend
    from oracle import proj_ric_utils as opru
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    pr = n30[0]
    F = (-pr.A - pr.Nc).tocsr()
    W = np.random.default_rng(9).standard_normal((pr.NV, 4))
    d = dict(adi_max_steps=8, adi_newZ_reltol=1e-30, ms=[float(p) for p in pb.logshifts(1.0, 1e3, 8)])
    backend.configure(child_smoother=1, coarse_max=300)
    try:
        Z = pru.solve_proj_lyap_stein(amat=F, mmat=pr.M, jmat=pr.J, wmat=W, adi_dict=d)["zfac"]
        info = backend.context().setup_info()
        assert info["levels"] == 3 and info["child_smoother"] == 1, info
        r_gpu = pru.comp_proj_lyap_res_norm(Z, F, pr.M, W, pr.J)
    finally:
        backend.configure()
    assert backend._opts == {}
    Zo = opru.solve_proj_lyap_stein(amat=F, mmat=pr.M, jmat=pr.J, wmat=W, adi_dict=d)["zfac"]
    r_cpu = opru.comp_proj_lyap_res_norm(Zo, F, pr.M, W, pr.J)
    print("drop-in ADI with the Vanka child: residual norm %.6e, oracle %.6e" % (r_gpu, r_cpu))
    assert r_cpu > 0 and np.isclose(r_gpu, r_cpu, rtol=1e-7)
