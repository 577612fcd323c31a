"""The NumPy model of the low-rank RADI iteration (tests/radi_model.py) against SciPy's dense Riccati solver on
ker J (tests/identities.dense_projected_are).  The model is the yardstick of tests/test_gpu_radi.py, so this file
has to pass before those tests mean anything."""
import numpy as np
import pytest

import radi_model as rm

BAR = 1e-12           # relative, X and cal E X B


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module", params=[4, 8])
def solved(request):
    """Every call form at one mesh size, solved once by the model (residual rule at 1e-16) and by the dense solver."""
    out = []
    for f in rm.call_forms(request.param) + rm.call_forms(request.param, narrow=True):
        r = rm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], f["ms"], old=f["old"], max_steps=200,
                    res_reltol=1e-16)
        out.append((f, r, rm.dense_are_of(f)))
    return request.param, out


def test_model_reproduces_dense_are(solved):
    N, runs = solved
    assert [f["name"] for f, _, _ in runs] == ["steady", "dre", "dre_old", "narrow"]
    for f, r, (X, K) in runs:
        ex, ek = rel(r["Z"] @ r["Z"].T, X), rel(r["gain"], K)
        print("N = %d %-8s steps %3d  rel X %.2e  rel K %.2e" % (N, f["name"], r["steps"], ex, ek))
        assert r["stopped"] == "res", f["name"]
        assert ex < BAR and ek < BAR, (f["name"], ex, ek)


def test_model_history_is_the_dense_riccati_residual(solved):
    N, runs = solved
    for f, r, _ in runs:
        m = f["W"].shape[1]
        dense = rm.dense_riccati_residuals(f["calA"], f["calE"], f["J"], f["B"], f["W"], r["Z"], m, old=f["old"])
        hist = r["res_hist"]
        assert dense.shape == hist.shape
        big = dense > 1e-10
        assert big.sum() >= 5
        dev = np.max(np.abs(hist[big] - dense[big]) / dense[big])
        print("N = %d %-8s history against the dense residual: %.2e over %d entries" % (N, f["name"], dev, big.sum()))
        assert dev < 1e-5, (f["name"], dev)


def test_model_update_is_the_iteration_step():
    """The longdouble update of one step (what the device kernels are compared with) is the step of the iteration."""
    f = rm.call_forms(4)[0]
    calA, calE, J = (rm._dn(f[k]) for k in ("calA", "calE", "J"))
    B, p = f["B"], -3.0
    R = rm.project(calE, J, f["W"])
    m = R.shape[1]
    V = rm.saddle_solve(calA + p * calE, J, R)
    G, C, RU, Zb = rm.update(p, V, B, np.hstack([R, np.zeros_like(B)]), f["calE"])
    Y = np.eye(m) + (V.T @ B) @ (V.T @ B).T
    T = -2 * p * np.linalg.solve(Y, V.T).T
    assert rel(np.asarray(RU[:, :m], float), R + calE @ T) < 1e-13
    assert rel(np.asarray(RU[:, m:], float), calE @ T @ (V.T @ B)) < 1e-13
    assert rel(np.asarray(Zb @ Zb.T, float), -2 * p * V @ np.linalg.solve(Y, V.T)) < 1e-13
    bounds = rm.update_bounds(p, V, B, np.hstack([R, np.zeros_like(B)]), f["calE"], 2.0 ** -53)
    assert all(np.all(np.isfinite(b)) and np.all(b >= 0) for b in bounds)
