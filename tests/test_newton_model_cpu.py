"""The dense model of the Newton-Kleinman driver (tests/newton_model.py) held to what it is used for, on the host:

1. the loop against SciPy's dense Riccati solver on ker J, and started from its own first iterate;
2. the update norm: NumPy's float64 QR route within ``UPD_DISTANCE`` units of the longdouble reference over the shapes
   of the GPU test, three seeded faults outside the GPU test's allowance;
3. the margins of every stopping decision in the cases tests/test_gpu_newton_steps.py runs, and their coverage;
4. the N = 8 fixture is the model's.

tests/test_gpu_newton_steps.py means what it says only while these pass.
"""
import numpy as np
import pytest

import newton_model as nm
import radi_model as rm

_forms = {}


def forms(N):
    if N not in _forms:
        _forms[N] = rm.call_forms(N)
    return _forms[N]


_live = {}


def live(N, i, G):
    key = (N, i, G)
    if key not in _live:
        _live[key] = nm.history_case(forms(N)[i], sweep_width=G)
    return _live[key]


# ------------------------------------------------------------------------------------------- 1. the loop
@pytest.mark.parametrize("i", [0, 1, 2])
def test_model_reaches_the_dense_solution(i):
    """Run to a relative update of 1e-13: the last iterate against identities.dense_projected_are at 1e-12."""
    f = forms(4)[i]
    run = nm.newton(f, newZ_reltol=1e-10, nwtn_max_steps=8, nwtn_upd_reltol=1e-13, nwtn_upd_abstol=0.0)
    X, _ = rm.dense_are_of(f)
    Z = run["steps"][-1]["Z"]
    err = np.linalg.norm(Z @ Z.T - X) / np.linalg.norm(X)
    print("%s: %d Newton steps, ADI steps %s, upd_rel %s, against the dense solution %.2e"
          % (f["name"], len(run["steps"]), [s["adi_steps"] for s in run["steps"]],
             ["%.1e" % s["upd_rel"] for s in run["steps"]], err))
    assert run["rule"] == "reltol" and 3 <= len(run["steps"]) <= 5
    assert err <= 1e-12


@pytest.mark.parametrize("i", [0, 2])
def test_model_started_from_its_first_iterate_repeats_the_later_steps(i):
    f = forms(4)[i]
    kw = dict(newZ_reltol=1e-9, nwtn_max_steps=8, nwtn_upd_reltol=1e-9, nwtn_upd_abstol=0.0)
    plain = nm.newton(f, **kw)
    again = nm.newton(f, Z0=plain["steps"][0]["Z"], problem=plain["problem"], **kw)
    assert len(again["steps"]) == len(plain["steps"]) - 1 >= 2
    for a, b in zip(again["steps"], plain["steps"][1:]):
        assert a["adi_steps"] == b["adi_steps"] and a["width"] == b["width"]
        assert a["upd"] == b["upd"] and a["x1"] == b["x1"] and np.array_equal(a["Z"], b["Z"])


def test_stop_rules_of_the_model():
    f = forms(4)[0]
    free = nm.newton(f, nwtn_max_steps=3, nwtn_upd_reltol=0.0, nwtn_upd_abstol=0.0)
    assert free["rule"] == "max_steps" and len(free["steps"]) == 3
    u = [s["upd"] for s in free["steps"]]
    r = [s["upd_rel"] for s in free["steps"]]
    pb = free["problem"]
    a = nm.newton(f, nwtn_max_steps=5, nwtn_upd_reltol=0.0, nwtn_upd_abstol=float(np.sqrt(u[1] * u[2])), problem=pb)
    b = nm.newton(f, nwtn_max_steps=5, nwtn_upd_abstol=0.0, nwtn_upd_reltol=float(np.sqrt(r[1] * r[2])), problem=pb)
    both = nm.newton(f, nwtn_max_steps=5, nwtn_upd_abstol=float(np.sqrt(u[1] * u[2])),
                     nwtn_upd_reltol=float(np.sqrt(r[1] * r[2])), problem=pb)
    assert (a["rule"], len(a["steps"])) == ("abstol", 3) and (b["rule"], len(b["steps"])) == ("reltol", 3)
    assert (both["rule"], len(both["steps"])) == ("abstol", 3)          # the first test of the ||


# ------------------------------------------------------------------------------------------- 2. the update norm
def _distances(route):
    """Largest |route - reference| / unit per shape, for upd and x1, over every case of every shape."""
    worst = {}
    for nv, k1, k0 in nm.upd_shapes():
        du = dx = 0.0
        for kind, Z1, Z0 in nm.upd_cases(nv, k1, k0):
            ref = nm.upd_reference(Z1, Z0)
            got = route(Z1, Z0)
            unit = nm.unit(Z1, Z0)
            du, dx = max(du, abs(got[0] - ref[0]) / unit), max(dx, abs(got[1] - ref[1]) / unit)
        worst[(nv, k1, k0)] = (du, dx)
    return worst


def test_numpy_route_within_the_distance():
    """``upd_float64_qr`` against ``upd_reference`` over the shapes of the GPU test: UPD_DISTANCE is the largest
    distance, measured here."""
    worst = _distances(nm.upd_float64_qr)
    for shape, (du, dx) in worst.items():
        print("nv %4d k1 %3d k0 %3d: upd %.3f  x1 %.3f  units of u (|Z1|^2 + |Z0|^2)" % (shape + (du, dx)))
    top = max(max(v) for v in worst.values())
    print("largest distance %.3f (UPD_DISTANCE = %.1f)" % (top, nm.UPD_DISTANCE))
    assert top <= nm.UPD_DISTANCE
    assert top >= nm.UPD_DISTANCE / 4.0            # the constant is the measurement, not a guess far above it


def test_delta_cases_keep_their_digits():
    """At delta = 1e-10 the update lies about 1e-10 below x1 and the GPU allowance is at most 1e-3 of it: four
    digits, the claim of diff_zzt_fnorm's comment."""
    for nv, k in ((300, 100), (1100, 128)):
        cases = dict((kind, (Z1, Z0)) for kind, Z1, Z0 in nm.upd_cases(nv, k, k))
        Z1, Z0 = cases["delta1e-10"]
        upd, x1 = nm.upd_reference(Z1, Z0)
        print("nv %d k %d: upd / x1 %.2e, allowance / upd %.2e" % (nv, k, upd / x1, nm.allowance(Z1, Z0) / upd))
        assert 1e-11 <= upd / x1 <= 1e-9
        assert nm.allowance(Z1, Z0) <= 1e-3 * upd


def _exceeds(route, which, shapes, kinds=None):
    out = []
    for nv, k1, k0 in shapes:
        for kind, Z1, Z0 in nm.upd_cases(nv, k1, k0):
            if Z0 is None or (kinds and kind not in kinds):
                continue
            err = abs(route(Z1, Z0)[which] - nm.upd_reference(Z1, Z0)[which])
            if err > nm.allowance(Z1, Z0):
                out.append((nv, k1, k0, kind, err / nm.allowance(Z1, Z0)))
    return out


SMALL_SHAPES = [s for s in nm.upd_shapes() if s[0] in (33, 300)]


def test_seeded_fault_gram_route():
    """The norm from the Gram matrix of [Z1, Z0] loses an update 1e-10 below x1."""
    bad = _exceeds(lambda a, b: (nm.upd_gram_route(a, b), 0.0), 0, SMALL_SHAPES, kinds=("delta1e-10",))
    print(bad)
    assert bad


def test_seeded_fault_sign():
    bad = _exceeds(lambda a, b: nm.upd_float64_qr(a, b, s0=+1.0), 0, SMALL_SHAPES)
    print(bad[:4])
    assert bad


def test_seeded_fault_x1_from_the_whole_r():
    bad = _exceeds(lambda a, b: nm.upd_float64_qr(a, b, x1_cols=a.shape[1] + b.shape[1]), 1, SMALL_SHAPES)
    print(bad[:4])
    assert bad


def test_shapes_are_the_issue_s():
    shapes = nm.upd_shapes()
    assert {s[0] for s in shapes} == {1, 33, 300, 1100}
    for nv in (1, 33, 300, 1100):
        assert {(a, b) for n, a, b in shapes if n == nv} >= set(nm.UPD_WIDTHS)      # nothing is above the limit
    assert (33, 33, 33) in shapes and (33, 20, 30) in shapes
    kinds = [k for k, _, _ in nm.upd_cases(33, 33, 33)]
    assert kinds == ["independent", "equal", "rotated", "delta1e-06", "delta1e-10", "delta1e-13"]
    _, Z1, Z0 = nm.upd_cases(300, 100, 100)[0]
    n1 = np.linalg.norm(Z1, axis=0)
    assert 1e5 <= n1.max() / n1.min() <= 1e7                 # graded over six orders of magnitude
    _, Z1, Zq = nm.upd_cases(300, 100, 100)[2]
    assert np.linalg.norm(Z1 @ Z1.T - Zq @ Zq.T) <= 1e-13 * np.linalg.norm(Z1 @ Z1.T) and not np.allclose(Z1, Zq)


# ------------------------------------------------------------------------------------------- 3. margins, coverage
def test_coverage_of_the_history_cases():
    cases = nm.HISTORY_CASES
    assert {i for N, i, G in cases if N == 4 and G == 1} == {0, 1, 2}
    assert len({i for N, i, G in cases if N == 8 and G == 1}) >= 2
    assert sum(1 for N, i, G in cases if N == 8 and G == 4) == 1
    assert [f["name"] for f in forms(4)] == list(nm.FORM_NAMES)
    fx = np.load(nm.GOLDEN)
    for N, i, G in cases:
        if N == 8:
            assert nm.case_key(N, i, G) + "/hist" in fx.files


@pytest.mark.parametrize("N,i,G", [c for c in nm.HISTORY_CASES if c[0] == 4])
def test_margins_live(N, i, G):
    case = live(N, i, G)
    assert case is not None
    _margins(nm.case_key(N, i, G), case["adi_margin"], case["newton_margin"], case["nwtn_upd_reltol"],
             [s["upd_rel"] for s in case["run"]["steps"]], [s["adi_steps"] for s in case["run"]["steps"]])
    # the margins the case reports are those of its run
    for s in case["run"]["steps"]:
        k = s["adi_steps"]
        assert s["rel_newZ"][k - 1] * nm.ADI_MARGIN <= case["newZ_reltol"] <= min(s["rel_newZ"][:k - 1]) / nm.ADI_MARGIN


@pytest.mark.parametrize("N,i,G", [c for c in nm.HISTORY_CASES if c[0] == 8])
def test_margins_fixture(N, i, G):
    case = nm.unpack(np.load(nm.GOLDEN), nm.case_key(N, i, G))
    _margins(nm.case_key(N, i, G), case["adi_margin"], case["newton_margin"], case["nwtn_upd_reltol"],
             [s["upd_rel"] for s in case["steps"]], [s["adi_steps"] for s in case["steps"]])
    assert max(s["trunc"] for s in case["steps"]) <= 0.02 * nm.K_TOL
    assert case["steps"][-1]["Z"] is not None and (G > 1 or all(s["Z"] is not None for s in case["steps"]))


def _margins(name, adi_margin, newton_margin, rtol, upd_rel, adi_steps):
    print("%s: ADI steps %s, ADI margin %.2f, upd_rel %s, Newton tolerance %.3e, margin %.1f"
          % (name, adi_steps, adi_margin, ["%.2e" % v for v in upd_rel], rtol, newton_margin))
    assert adi_margin >= nm.ADI_MARGIN
    assert newton_margin >= nm.NEWTON_MARGIN
    assert all(v >= nm.NEWTON_MARGIN * rtol for v in upd_rel[:-1]) and upd_rel[-1] * nm.NEWTON_MARGIN <= rtol
    assert rtol >= nm.UPD_REL_FLOOR and len(upd_rel) >= 2


# ------------------------------------------------------------------------------------------- 4. the fixture
def test_fixture_is_the_model_s():
    """One N = 8 case recomputed: tolerances, step counts and histories equal the fixture's to rounding (the LAPACK
    and BLAS underneath may differ between machines), the iterates at the truncation they are kept at."""
    N, i, G = 8, 1, 1
    key = nm.case_key(N, i, G)
    kept = nm.unpack(np.load(nm.GOLDEN), key)
    now = nm.live_case(N, i, G)
    assert [s["adi_steps"] for s in now["steps"]] == [s["adi_steps"] for s in kept["steps"]]
    assert np.isclose(now["newZ_reltol"], kept["newZ_reltol"], rtol=1e-6)
    assert np.isclose(now["nwtn_upd_reltol"], kept["nwtn_upd_reltol"], rtol=1e-6)
    for a, b in zip(now["steps"], kept["steps"]):
        assert a["width"] == b["width"]
        assert np.isclose(a["x1"], b["x1"], rtol=1e-10)
        assert abs(a["upd"] - b["upd"]) <= 1e-10 * b["x1"]
        assert nm.upd_float64_qr(a["Z"], b["Z"])[0] <= 1e-10 * b["x1"]
        assert np.isclose(a["trunc"], b["trunc"], rtol=1e-3)
