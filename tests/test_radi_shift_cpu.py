"""RADI with shifts generated from the iteration, on the CPU:

1. the NumPy model (tests/radi_shift_model.py) against SciPy's dense Riccati solver on ker J, and its step counts
   against the cycled list's;
2. the library's host selection ``ricadi_host_radi_shift`` (its own Hessenberg-QR eigensolver and null vectors)
   against the model's selection with NumPy's ``eig``: on every reduced matrix the N = 8 runs produce and on random
   instances;
3. the entry's argument contract.

No GPU is needed: the entry is host code, like ``ricadi_host_cauchy``.
"""
import numpy as np
import pytest

import radi_model as rm
import radi_shift_model as sm
from optconpy_amd import _lib

BAR = 1e-12           # relative, X and cal E X B (the bar of test_radi_model_cpu.py)
EIG_TOL = 1e-9        # relative, every eigenvalue of the Hamiltonian and the chosen shift
MARGIN_MIN = 1.01     # instances whose two best criterion values are closer than this may be left out ...
LEFT_OUT_MAX = 0.05   # ... at most this share of all instances


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


_runs = {}


def runs(N):
    """Every call form at one mesh size: (form, generated-shift model run at the tolerance, its recorded H)."""
    if N not in _runs:
        out = []
        for f in rm.call_forms(N) + rm.call_forms(N, narrow=True):
            p0 = sm.initial_shift(f["calA"], f["calE"])
            rec = []
            tight = sm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], [p0], old=f["old"], max_steps=200,
                            res_reltol=1e-16)
            loose = sm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], [p0], old=f["old"], max_steps=200,
                            res_reltol=1e-10, record=rec)
            cyc = rm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], f["ms"], old=f["old"], max_steps=200,
                          res_reltol=1e-10)
            out.append(dict(form=f, tight=tight, loose=loose, cycled=cyc, rec=rec))
        _runs[N] = out
    return _runs[N]


# ---------------------------------------------------------------------------------------------------- 1. the model
@pytest.mark.parametrize("N", [4, 8])
def test_model_reproduces_dense_are(N):
    rs = runs(N)
    assert [r["form"]["name"] for r in rs] == ["steady", "dre", "dre_old", "narrow"]
    for r in rs:
        f, t = r["form"], r["tight"]
        X, K = rm.dense_are_of(f)
        ex, ek = rel(t["Z"] @ t["Z"].T, X), rel(t["gain"], K)
        print("N = %d %-8s steps %3d fallbacks %d  rel X %.2e  rel K %.2e" % (N, f["name"], t["steps"], t["fallbacks"],
                                                                             ex, ek))
        assert t["stopped"] == "res", f["name"]
        assert ex < BAR and ek < BAR, (f["name"], ex, ek)


@pytest.mark.parametrize("N", [4, 8])
def test_model_needs_no_more_steps_than_the_cycled_list(N):
    for r in runs(N):
        g, cy = r["loose"], r["cycled"]
        mg = g["margins"]
        print("N = %d %-8s steps %d (cycled list %d)  fallbacks %d  smallest margin %.3f" % (
            N, r["form"]["name"], g["steps"], cy["steps"], g["fallbacks"], mg.min() if mg.size else np.inf))
        assert g["stopped"] == "res" and cy["stopped"] == "res"
        assert g["steps"] <= cy["steps"], (r["form"]["name"], g["steps"], cy["steps"])
        assert np.all(g["ms"] < 0) and len(g["ms"]) == g["steps"]


# ------------------------------------------------------------------------------- 2. the host entry against the model
def _match(a, b):
    """Largest relative distance of the eigenvalues a from b under the greedy pairing by distance."""
    b = list(b)
    worst = 0.0
    for x in sorted(a, key=lambda z: -abs(z)):
        i = int(np.argmin([abs(x - y) for y in b]))
        worst = max(worst, abs(x - b[i]) / max(abs(b[i]), 1e-300))
        b.pop(i)
    return worst


def _check_instances(insts, what):
    left_out, worst_e, worst_p, worst_m, smallest = 0, 0.0, 0.0, 0.0, np.inf
    for k, m, nb, H in insts:
        p_ref, margin, lam, _ = sm.select(k, m, nb, H)
        p, mg, ev = _lib.host_radi_shift(k, m, nb, H, eigs=True)
        assert ev.size == 2 * k
        worst_e = max(worst_e, _match(ev, lam))
        smallest = min(smallest, margin)
        if margin < MARGIN_MIN:
            left_out += 1
            continue
        assert p < 0 and p_ref < 0
        worst_p = max(worst_p, abs(p - p_ref) / abs(p_ref))
        if np.isfinite(margin):
            worst_m = max(worst_m, abs(mg - margin) / margin)
        else:
            assert mg == np.inf
        p2, mg2 = _lib.host_radi_shift(k, m, nb, H)
        assert p2 == p and mg2 == mg
    print("%s: %d instances, %d left out (margin < %.2f), smallest margin %.4f, eigenvalues within %.2e, shifts "
          "within %.2e, margins within %.2e" % (what, len(insts), left_out, MARGIN_MIN, smallest, worst_e, worst_p, worst_m))
    assert worst_e <= EIG_TOL, worst_e
    assert worst_p <= EIG_TOL, worst_p
    return left_out


def test_host_selection_on_the_model_runs():
    """Every H the N = 8 runs at 1e-10 produce.  (Below a relative residual of about 1e-13 H_R H_R^T falls under the
    rounding errors of the other blocks and the eigenvectors' lower halves with it: the criterion is noise there.)"""
    insts = [h for r in runs(8) for h in r["rec"]]
    assert len(insts) >= 60
    assert _check_instances(insts, "N = 8 runs") == 0           # (their margins are all above 1.03)


def test_host_selection_on_random_instances():
    insts = []
    for i in range(50):
        k = [1, 2, 5, 16, 32][i % 5]
        nb = [1, 2, 3, 64][(i // 5) % 4]
        insts.append((k, k, nb, sm.random_instance(k, k, nb, seed=100 + i)))
    left_out = _check_instances(insts, "random")
    assert left_out <= LEFT_OUT_MAX * len(insts)


# ---------------------------------------------------------------------------------------------------- 3. contract
def test_contract():
    H = sm.random_instance(2, 2, 1, seed=1)
    for k, m, nb in [(0, 2, 1), (33, 2, 1), (2, 0, 1), (2, 33, 1), (2, 2, 0), (2, 2, 65)]:
        with pytest.raises(ValueError):
            _lib.host_radi_shift(k, m, nb, np.zeros(max(k, 1) * (2 * max(k, 0) + max(m, 0) + 2 * max(nb, 0)) + 8))
    with pytest.raises(ValueError):
        _lib.host_radi_shift(2, 2, 1, H[:, :-1])
    # singular H_E
    Hs = H.copy()
    Hs[:, 2:4] = np.array([[1.0, 2.0], [2.0, 4.0]])
    with pytest.raises(RuntimeError, match="singular"):
        _lib.host_radi_shift(2, 2, 1, Hs)
    Hn = H.copy()
    Hn[0, 0] = np.nan
    with pytest.raises(RuntimeError):
        _lib.host_radi_shift(2, 2, 1, Hn)
    # no eigenvalue in the open left half plane: Ham = [[0, 0], [-r^2, 0]]
    H0 = np.array([[0.0, 1.0, 0.7, 0.0, 0.0]])
    p, mg = _lib.host_radi_shift(1, 1, 1, H0)
    assert p == 0.0
    assert sm.select(1, 1, 1, H0)[0] == 0.0
    # one candidate: the margin is +inf
    H1 = np.array([[-2.0, 1.0, 0.5, 0.0, 0.3]])
    p, mg = _lib.host_radi_shift(1, 1, 1, H1)
    assert p < 0 and mg == np.inf
    assert abs(p - sm.select(1, 1, 1, H1)[0]) <= 1e-12 * abs(p)
