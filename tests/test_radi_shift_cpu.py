"""RADI with shifts generated from the iteration, on the CPU:

1. the NumPy model (tests/radi_shift_model.py) against SciPy's dense Riccati solver on ker J, and its step counts
   against the cycled list's;
2. the library's host selection ``ricadi_host_radi_shift`` (its own Hessenberg-QR eigensolver and null vectors)
   against the model's selection (NumPy's eigenvalues, extended-precision null vectors): on every reduced matrix the N = 8 runs produce and on random
   instances;
3. the entry's argument contract;
4. the model with refused selections (the fallback cycle) against the dense solver;
5. ``ricadi_host_radi_next_shift`` -- what the driver does with the H and R a step has fetched: the ``keep`` rule, the
   restriction of H, the refusals -- against ``keep_columns``, ``restrict`` and ``select`` of the model.

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
            rec, full = [], []
            tight = sm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], [p0], old=f["old"], max_steps=200,
                            res_reltol=1e-16)
            loose = sm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], [p0], old=f["old"], max_steps=200,
                            res_reltol=1e-10, record=rec, record_full=full)
            cyc = rm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], f["ms"], old=f["old"], max_steps=200,
                          res_reltol=1e-10)
            out.append(dict(form=f, tight=tight, loose=loose, cycled=cyc, rec=rec, full=full))
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


# ------------------------------------------------------------------------------------ 4. the model with refusals
REFUSE = (2, 3, 6)


def fallback_list(f):
    """The first shift and three entries of the form's own list: the fallback cycle of the refusal tests."""
    return [sm.initial_shift(f["calA"], f["calE"])] + [float(v) for v in f["ms"][:3]]


@pytest.mark.parametrize("N", [4, 8])
def test_model_with_refusals_reproduces_dense_are(N):
    """Refused selections after steps 2, 3 and 6: steps 3, 4 and 7 run with entries 1, 2 and 3 of the list (the
    fallback cycle's counter starts at entry 1 and is its own), every other step with a generated shift, and the
    iteration converges to the same X and K."""
    for f in rm.call_forms(N) + rm.call_forms(N, narrow=True):
        fb = fallback_list(f)
        t = sm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], fb, old=f["old"], max_steps=200, res_reltol=1e-16,
                    refuse=REFUSE)
        X, K = rm.dense_are_of(f)
        ex, ek = rel(t["Z"] @ t["Z"].T, X), rel(t["gain"], K)
        print("N = %d %-8s steps %3d fallbacks %d  rel X %.2e  rel K %.2e" % (N, f["name"], t["steps"], t["fallbacks"],
                                                                             ex, ek))
        assert t["stopped"] == "res", f["name"]
        assert ex < BAR and ek < BAR, (f["name"], ex, ek)
        assert t["steps"] >= 7
        assert (t["ms"][2], t["ms"][3], t["ms"][6]) == (fb[1], fb[2], fb[3]), f["name"]
        assert t["fallbacks"] == 3, f["name"]
        assert len(t["kept"]) == t["steps"] - 1           # one selection after every step but the last
        free = sm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], fb, old=f["old"], max_steps=200,
                       res_reltol=1e-16)
        assert free["ms"][1] == t["ms"][1] and free["ms"][2] != t["ms"][2]       # the refusal is what changed step 3


# ------------------------------------------------------- 5. the driver's use of the selection against the model
def _reference_next(m, nb, H, Rq):
    keep = sm.keep_columns(Rq)
    k = int(keep.sum())
    p, margin, _, _ = sm.select(k, m, nb, sm.restrict(H, m, nb, keep))
    return p, margin, k


def _check_next(m, nb, H, Rq):
    """The entry against keep_columns, restrict, select; returns (kept, relative shift error, model's margin,
    relative margin error)."""
    p_ref, margin, k = _reference_next(m, nb, H, Rq)
    p, mg, kept, refusal = _lib.host_radi_next_shift(m, nb, H, Rq)
    assert refusal is None and kept == k, (refusal, kept, k)
    assert p < 0 and p_ref < 0
    if not np.isfinite(margin):
        assert mg == np.inf
    return kept, abs(p - p_ref) / abs(p_ref), margin, abs(mg - margin) / margin if np.isfinite(margin) else 0.0


def test_host_next_shift_on_the_model_runs():
    """Every (H, R) of all m columns the N = 8 runs record, all four forms: 4 of 4 columns kept in the steady form, 3
    of 3 in the narrow one, 4 of 8 in the two dre forms."""
    total = 0
    for r in runs(8):
        name = r["form"]["name"]
        m = r["form"]["W"].shape[1]
        want = {"steady": 4, "narrow": 3, "dre": 4, "dre_old": 4}[name]
        assert m == {"steady": 4, "narrow": 3, "dre": 8, "dre_old": 8}[name]
        assert len(r["full"]) == len(r["rec"]) >= 12
        worst, smallest = 0.0, np.inf
        for (mm, nb, H, Rq), (k, _, _, _) in zip(r["full"], r["rec"]):
            assert H.shape == (mm, 3 * mm + 2 * nb) and Rq.shape == (mm, mm) and mm == m
            kept, err, margin, _ = _check_next(mm, nb, H, Rq)
            assert kept == want == k, (name, kept, k)
            assert margin >= MARGIN_MIN                   # (all above 1.02: the selection is well determined)
            worst, smallest = max(worst, err), min(smallest, margin)
            total += 1
        print("N = 8 %-8s %2d selections, kept %d of %d, shifts within %.2e, smallest margin %.3f" % (
            name, len(r["full"]), want, m, worst, smallest))
        assert worst <= EIG_TOL, (name, worst)
    assert total >= 60


def test_host_next_shift_margins_on_the_model_runs():
    """The margins of the same selections within EIG_TOL of the model's.  (Late selections -- relative residual below
    1e-8 -- have eigenvectors whose lower half is tiny: the model takes them from extended-precision null vectors,
    radi_shift_model.select; with LAPACK's eigenvectors its own margins were off by up to 2.8e-7 there.)"""
    worst = {}
    for r in runs(8):
        for i, (mm, nb, H, Rq) in enumerate(r["full"]):
            _, _, margin, merr = _check_next(mm, nb, H, Rq)
            if merr > EIG_TOL:
                print("N = 8 %-8s selection %2d: the model's margin %.12f, the entry's off it by %.2e" % (
                    r["form"]["name"], i + 1, margin, merr))
            worst[r["form"]["name"]] = max(worst.get(r["form"]["name"], 0.0), merr)
    print("margins within", worst)
    assert max(worst.values()) <= EIG_TOL, worst


def _dense_instance(nv, m, nb, seed):
    """A small dense problem and an iteration state: stable pencil (cal A, cal E), B, R, U."""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((nv, nv))
    calE = M @ M.T / nv + np.eye(nv)
    S = rng.standard_normal((nv, nv))
    N = rng.standard_normal((nv, nv))
    calA = 0.5 * (S - S.T) - N @ N.T / nv - 0.1 * np.eye(nv)
    B = rng.standard_normal((nv, nb))
    U = np.zeros((nv, nb))
    R = 0.1 * rng.standard_normal((nv, m))
    return calA, calE, B, R, U


def test_host_next_shift_leaves_out_dependent_columns():
    """A block with duplicated columns (6 columns, rank 3; nb = 2): the QR's diagonal has three entries at rounding
    level, the basis is the other three columns -- not the leading ones: the duplicates are interleaved -- and the
    shift is the one the model selects on that basis."""
    nv, m, nb = 30, 6, 2
    calA, calE, B, R, U = _dense_instance(nv, m, nb, seed=7)
    rng = np.random.default_rng(8)
    Z3 = rng.standard_normal((nv, 3))
    blk = Z3[:, [0, 0, 1, 2, 1, 2]] * np.array([1.0, -2.0, 1.0, 1.0, 0.5, 3.0])
    Q, Rq = np.linalg.qr(blk)
    keep = sm.keep_columns(Rq)
    assert keep.tolist() == [True, False, True, True, False, False]
    H = sm.pack(Q, calA, calE, R, U, B)
    kept, err, margin, merr = _check_next(m, nb, H, Rq)
    print("duplicated columns: kept %d of %d, shift within %.2e, margin %.3f within %.2e" % (kept, m, err, margin, merr))
    assert kept == 3 and margin >= MARGIN_MIN and err <= EIG_TOL and merr <= EIG_TOL
    # the columns left out are arbitrary directions: whatever H holds for them, the result is the same, bit for bit
    H2 = H.copy()
    out = np.flatnonzero(~keep)
    H2[out, :] = 1e3
    H2[:, out] = -1e3
    H2[:, m + out] = 7.0
    assert _lib.host_radi_next_shift(m, nb, H2, Rq) == _lib.host_radi_next_shift(m, nb, H, Rq)
    # columns that depend on their predecessors only to the accuracy of an iterative solve (the device's blocks:
    # relative residual 1e-10 per column) are left out as well, and the shift is that of the clean block to that
    # accuracy.  (Dependent columns LAST, as in the dre forms: a kept column that follows a dropped one is
    # orthogonalised against that one's arbitrary direction too, and the span of the kept columns of Q is then not the
    # block's range -- above, the entry and the model agree on such a block because they read the same Q.)
    blk = Z3[:, [0, 1, 2, 0, 1, 2]] * np.array([1.0, 1.0, 1.0, -2.0, 0.5, 3.0])
    Qt, Rt = np.linalg.qr(blk)
    keep = sm.keep_columns(Rt)
    assert keep.tolist() == [True, True, True, False, False, False]
    noise = rng.standard_normal((nv, m))
    noise *= 1e-10 * np.linalg.norm(blk, axis=0) / np.linalg.norm(noise, axis=0)
    Qn, Rn = np.linalg.qr(blk + noise)
    dn = np.abs(np.diag(Rn))
    assert 1e-12 * dn.max() < dn[~keep].min() and dn[~keep].max() < 1e-9 * dn.max()     # the old rule kept these
    pn, _, keptn, refusal = _lib.host_radi_next_shift(m, nb, sm.pack(Qn, calA, calE, R, U, B), Rn)
    p, _, keptt, _ = _lib.host_radi_next_shift(m, nb, sm.pack(Qt, calA, calE, R, U, B), Rt)
    assert refusal is None and keptn == keptt == 3 and sm.keep_columns(Rn).tolist() == keep.tolist()
    assert abs(pn - p) <= 1e-6 * abs(p), (pn, p)
    keep = sm.keep_columns(Rq)
    # the threshold is relative to the largest diagonal entry and inclusive
    assert sm.RANK_TOL == 3e-8
    Rs = np.diag([4.0, 1.2e-7, 1.19e-7, 1.0, 1.0, 1.0])
    assert _lib.host_radi_next_shift(m, nb, H, Rs)[2] == 5
    assert int(sm.keep_columns(Rs).sum()) == 5
    assert _lib.host_radi_next_shift(m, nb, H, -Rs)[2] == 5         # (the sign of a diagonal entry does not matter)


def test_host_next_shift_kept_one():
    m, nb = 2, 1
    calA, calE, B, R, U = _dense_instance(12, m, nb, seed=3)
    Q = np.linalg.qr(np.random.default_rng(4).standard_normal((12, m)))[0]
    H = sm.pack(Q, calA, calE, R, U, B)
    for Rq, col in ((np.array([[2.0, 0.3], [0.0, 1e-9]]), 0), (np.array([[1e-9, 0.3], [0.0, -2.0]]), 1)):
        p, mg, kept, refusal = _lib.host_radi_next_shift(m, nb, H, Rq)
        assert refusal is None and kept == 1 and mg == np.inf           # one candidate: nothing to compare it with
        Hk = sm.pack(Q[:, [col]], calA, calE, R, U, B)
        p_ref = sm.select(1, m, nb, Hk)[0]
        assert p_ref < 0 and abs(p - p_ref) <= EIG_TOL * abs(p_ref)
        assert _lib.host_radi_shift(1, m, nb, Hk)[0] == pytest.approx(p, rel=1e-12)


def test_host_next_shift_refusals():
    """Every refusal is a return value of its own, not an error; p and the margin are then not set."""
    H = sm.random_instance(2, 2, 1, seed=1)            # (k = m: the packed H of all columns has the same shape)
    I2 = np.eye(2)
    p, mg, kept, refusal = _lib.host_radi_next_shift(2, 1, H, I2)
    assert refusal is None and kept == 2 and p < 0
    assert abs(p - sm.select(2, 2, 1, H)[0]) <= EIG_TOL * abs(p)
    for bad in (np.nan, np.inf, -np.inf):
        for i in (0, 1):
            Rn = I2.copy()
            Rn[i, i] = bad
            assert _lib.host_radi_next_shift(2, 1, H, Rn) == (None, None, 0, "r_not_finite")
    Rn = I2.copy()
    Rn[0, 1] = np.nan                                   # (only the diagonal is looked at)
    assert _lib.host_radi_next_shift(2, 1, H, Rn)[3] is None
    assert _lib.host_radi_next_shift(2, 1, H, np.zeros((2, 2))) == (None, None, 0, "r_zero")
    assert _lib.host_radi_next_shift(2, 1, H, np.array([[0.0, 5.0], [0.0, 0.0]])) == (None, None, 0, "r_zero")
    # no candidate: the H0 of test_contract
    H0 = np.array([[0.0, 1.0, 0.7, 0.0, 0.0]])
    assert _lib.host_radi_next_shift(1, 1, H0, np.array([[1.0]])) == (None, None, 1, "no_shift")
    # singular H_E; a value in H that is not finite
    Hs = H.copy()
    Hs[:, 2:4] = np.array([[1.0, 2.0], [2.0, 4.0]])
    assert _lib.host_radi_next_shift(2, 1, Hs, I2) == (None, None, 2, "breakdown")
    Hn = H.copy()
    Hn[1, 0] = np.nan
    assert _lib.host_radi_next_shift(2, 1, Hn, I2) == (None, None, 2, "breakdown")
    # ... but not where it belongs to a column that is left out
    assert _lib.host_radi_next_shift(2, 1, Hn, np.diag([1.0, 1e-9]))[2:] == (1, None)
    # sizes
    for m, nb in [(0, 1), (33, 1), (2, 0), (2, 65)]:
        with pytest.raises(ValueError):
            _lib.host_radi_next_shift(m, nb, np.zeros(max(m, 1) * (3 * max(m, 0) + 2 * max(nb, 0))),
                                      np.zeros(max(m, 1) ** 2))
    with pytest.raises(ValueError):
        _lib.host_radi_next_shift(2, 1, H[:, :-1], I2)
    with pytest.raises(ValueError):
        _lib.host_radi_next_shift(2, 1, H, np.eye(3))
