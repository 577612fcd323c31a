"""``ms='auto'`` on the MI355X: the projected-pencil kernel (K7) against NumPy, ``auto_shifts`` against the SciPy
model (``adi_shift_model``), and the drop-in's ADI / Newton-ADI / DRE sweep with the generated shifts."""
import numpy as np
import pytest
import scipy.sparse as sps

from optconpy_amd import _lib, adi_shifts as ads, backend, problems as pb

pytestmark = pytest.mark.gpu
KS = [1, 16, 40, 64, 128]


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _int_values(M, rng, lo, hi, diag):
    """The pattern of M with small-integer values, diagonal ``diag`` (nonzero)."""
    M = sps.csr_matrix(M, copy=True)
    M.data = rng.integers(lo, hi, M.nnz).astype(float)
    M = M.tolil()
    M.setdiag(diag)
    return M.tocsr()


@pytest.fixture(scope="module", params=[15, 58])
def pencil_case(request):
    N = request.param
    pr = pb.ricc_problem(N, 0.05)
    rng = np.random.default_rng(N)
    calA = _int_values((pr.A + pr.Nc).T, rng, -3, 4, -7.0)                  # non-symmetric
    calE = _int_values(pr.M, rng, -1, 2, 5.0)
    ctx = _lib.Context(0)
    ctx.set_operator(calA, calE, pr.J)
    yield pr, calA, calE, ctx
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_project_pencil_exact_on_integers(pencil_case, k):
    pr, calA, calE, ctx = pencil_case
    Q = np.random.default_rng(k).integers(-2, 3, (pr.NV, k)).astype(float)
    HA, HE = ctx.project_pencil(Q)
    assert np.array_equal(HA, Q.T @ (calA @ Q))
    assert np.array_equal(HE, Q.T @ (calE @ Q))


@pytest.mark.parametrize("k", KS)
def test_project_pencil_random_lowrank_and_bitwise(pencil_case, k):
    pr, calA, calE, ctx = pencil_case
    rng = np.random.default_rng(100 + k)
    Q = rng.standard_normal((pr.NV, k))
    HA, HE = ctx.project_pencil(Q)
    assert rel(HA, Q.T @ (calA @ Q)) <= 1e-13
    assert rel(HE, Q.T @ (calE @ Q)) <= 1e-13
    HA2, HE2 = ctx.project_pencil(Q)
    assert HA.tobytes() == HA2.tobytes() and HE.tobytes() == HE2.tobytes()
    U, V = rng.standard_normal((pr.NV, 3)), rng.standard_normal((pr.NV, 3))
    ctx.set_lowrank(U, V)
    try:
        HL, HEL = ctx.project_pencil(Q)
        HL2, _ = ctx.project_pencil(Q)
    finally:
        ctx.set_lowrank(None, None)
    assert rel(HL, Q.T @ (calA @ Q) - (Q.T @ U) @ (V.T @ Q)) <= 1e-13
    assert HEL.tobytes() == HE.tobytes()
    assert HL.tobytes() == HL2.tobytes()


def _dre30(tau):
    from identities import dre_step_inputs
    pr = pb.ricc_problem(30, 0.05)
    kw, p = dre_step_inputs(pr, tau=tau)
    return pr, kw, p


def test_auto_shifts_match_model_n30():
    from adi_shift_model import model_shifts
    pr, kw, p = _dre30(3e-4)
    calA, calE, J, W = kw["amat"], kw["mmat"], kw["jmat"], kw["wmat"]
    ctx = _lib.Context(0)
    try:
        ctx.set_operator(calA, calE, J)
        ms = ads.auto_shifts(ctx, W)
    finally:
        ctx.close()
    ref = model_shifts(calA, calE, J, W)
    assert not ms.info["fallback"] and ms.info["warm_solves"] > 0
    assert len(ms) == len(ref), (ms, ref)
    assert np.allclose(ms, ref, rtol=1e-8, atol=0.0), (ms, ref)


def test_solve_proj_lyap_stein_auto_n30():
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    from identities import check_reference_identities
    backend.reset()
    pr, kw, p = _dre30(3e-4)
    F, M, J, W = p["ft"].T.tocsr(), pr.M, pr.J, p["wmat"]
    base = pru.solve_proj_lyap_stein(amat=F, mmat=M, jmat=J, wmat=W, adi_dict=dict(sweep_width=1))
    auto = pru.solve_proj_lyap_stein(amat=F, mmat=M, jmat=J, wmat=W, adi_dict=dict(ms="auto", sweep_width=1))
    assert auto["adi_steps"] <= 0.5 * base["adi_steps"], (auto["adi_steps"], base["adi_steps"], auto["ms"])
    assert auto["ms"] and all(x < 0 for x in auto["ms"]) and not auto["shift_info"]["fallback"]
    check_reference_identities(pru, M, J, F, W, dict(ms="auto", sweep_width=1))
    # the sweep form: windows of the generated list recombined through their Cauchy matrices
    sw = pru.solve_proj_lyap_stein(amat=F, mmat=M, jmat=J, wmat=W, adi_dict=dict(ms="auto", sweep_width=16))
    assert sw["adi_rel_newZ"] < 1e-8
    backend.reset()


def test_newton_adi_auto_vs_dense_are_n15():
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    from identities import dense_projected_are, dre_step_inputs
    backend.reset()
    pr = pb.ricc_problem(15, 0.05)
    kw, p = dre_step_inputs(pr, tau=0.05, with_old=True)
    B = np.sqrt(p["tau"]) * p["tb"]
    calA = p["ft"].toarray() + kw["mtxoldb"] @ B.T
    X = dense_projected_are(calA, p["MT"], pr.J, B, p["wmat"])
    tight = dict(adi_max_steps=300, adi_newZ_reltol=1e-12, nwtn_max_steps=30, nwtn_upd_reltol=1e-11,
                 nwtn_upd_abstol=1e-14)
    out = pru.proj_alg_ric_newtonadi(nwtn_adi_dict=dict(tight, ms="auto"), **kw)
    Z = out["zfac"]
    assert out["ms"] and not out["shift_info"]["fallback"]
    assert rel(p["MT"] @ (Z @ (Z.T @ B)), p["MT"] @ (X @ B)) < 1e-6
    backend.reset()


def test_two_step_dre_sweep_auto_vs_dense():
    from identities import dense_dre_sweep_gains
    from optconpy_amd.dae_ric import MemoryStore, solve_flow_daeric
    from test_dae_ric import _pin_setup
    backend.reset()
    pr, kw, tmesh = _pin_setup()
    kw = dict(kw, nwtn_adi_dict=dict(kw["nwtn_adi_dict"], ms="auto"))
    dense = dense_dre_sweep_gains(pr, kw, tmesh)
    store = MemoryStore()
    fb = solve_flow_daeric(store=store, **kw)
    for t in tmesh:
        K = store.load(fb[t]["mtxtb"])
        assert np.linalg.norm(K - dense[t]) <= 1e-6 * np.linalg.norm(dense[t]), t
    backend.reset()
