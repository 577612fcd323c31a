"""Dense FP64 model of the Newton-Kleinman driver (``ric_newtonadi_run`` of optconpy_amd/csrc/solver_newton.inl) and
of its update norm (``diff_zzt_fnorm`` of csrc/solver_dense.inl), in NumPy / SciPy.  Nothing is shared with the
library or with oracle/; the inner ADI is ``adi_res_model.AdiResModel`` on the closed loop, its stopping step
``adi_res_model.stopping_step`` (sweep form: ``adi_sweep_model.sweep_schedule``).

  step k       K = cal E Z Z^T B  (0 without an iterate);  closed loop  cal A - (K - old) B^T;  rhs [W, K] (W alone
               without an iterate), W projected once;  ADI until its rule fires;  Z_new = its blocks
  update       upd = ||Z_new Z_new^T - Z Z^T||_F,  x1 = ||Z_new Z_new^T||_F,  upd_rel = upd / x1
  stop         upd < nwtn_upd_abstol ('abstol', reported where both fire)  ||  upd_rel < nwtn_upd_reltol ('reltol')

The library recompresses Z_new before it forms the update (truncation at 3e-8 of the largest singular value of Z,
1e-15 in Z Z^T); the model keeps the raw blocks.

The update norm has two models: :func:`upd_reference`, the quantity itself in ``np.longdouble`` from the explicitly
formed difference, and :func:`upd_float64_qr`, the route the device takes in float64 NumPy.  The distance of the
second from the first over the shapes of :func:`upd_cases`, in units of ``u (||Z1||_F^2 + ||Z0||_F^2)``, is
``UPD_DISTANCE``; the device is allowed ``UPD_FACTOR`` times that (the rule of ``dense_model.QR_R_FACTOR``).
"""
import os

import numpy as np

from adi_res_model import AdiResModel, stopping_step

LD = np.longdouble
U64 = 2.0 ** -53
# Largest distance of upd_float64_qr (upd and x1) from upd_reference over upd_cases(), in units of
# u (||Z1||_F^2 + ||Z0||_F^2), as measured by tests/test_newton_model_cpu.py::test_numpy_route_within_the_distance
# (which prints it) with NumPy's Householder QR: 6.87, at nv = 300 with one column on either side; rounded up.
UPD_DISTANCE = 7.0
UPD_FACTOR = 10.0
# The bar Z Z^T and the gain are held to against the dense Riccati solution (K_TOL of tests/test_gpu_small_ops.py,
# tests/test_gpu_radi.py: "the project's parity bar")
K_TOL = 1e-6
# Relative update below which the device's value is the noise of its inexact inner solves, not the model's number
# (tests/test_gpu_adi_res.py: "an update of 1e-8 relative is what inner solves at a residual of 1e-10 can resolve"),
# times ten: no Newton tolerance of a history case is placed below it
UPD_REL_FLOOR = 1e-7
ADI_MARGIN, NEWTON_MARGIN = 2.0, 10.0
ADI_MAX_STEPS = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "newton_model.npz")
# Truncation (relative to the largest singular value of Z) of the iterates as the cases keep them (the fixture has to
# stay below 1 MiB): about 1e-8 in Z Z^T, a hundredth of K_TOL.  The error made is measured and kept with each iterate
# (`trunc`), and the tests that hold a device factor against such an iterate take it off their bar.  The sweep-form
# case keeps its last iterate only.
GOLDEN_TRUNC = 1e-4


def _dn(a):
    return a.toarray() if hasattr(a, "toarray") else np.asarray(a, dtype=float)


# ------------------------------------------------------------------------------------------------ the update norm
def unit(Z1, Z0=None):
    """``u (||Z1||_F^2 + ||Z0||_F^2)``: the unit the errors of the update norm are counted in."""
    z = float(np.sum(np.asarray(Z1, dtype=float) ** 2))
    if Z0 is not None and np.size(Z0):
        z += float(np.sum(np.asarray(Z0, dtype=float) ** 2))
    return U64 * z


def allowance(Z1, Z0=None):
    return UPD_FACTOR * UPD_DISTANCE * unit(Z1, Z0)


def _sym_fro(D, sgn, blk=256):
    """||D diag(sgn) D^T||_F in longdouble from the explicitly formed matrix, block row by block row (the blocks
    below the diagonal are the transposes of those above it and are counted, not formed)."""
    D = np.asarray(D, dtype=LD)
    DS = D * np.asarray(sgn, dtype=LD)[None, :]
    n = D.shape[0]
    tot = LD(0)
    for i in range(0, n, blk):
        M = DS[i:i + blk] @ D[i:].T
        w = M.shape[0]
        tot += np.sum(M[:, :w] ** 2) + 2 * np.sum(M[:, w:] ** 2)
    return np.sqrt(tot)


def upd_reference(Z1, Z0=None):
    """``(||Z1 Z1^T - Z0 Z0^T||_F, ||Z1 Z1^T||_F)`` in longdouble, as floats."""
    Z1 = np.asarray(Z1, dtype=float)
    k1 = Z1.shape[1]
    k0 = 0 if Z0 is None else np.shape(Z0)[1]
    D = Z1 if k0 == 0 else np.hstack([Z1, np.asarray(Z0, dtype=float)])
    sgn = np.r_[np.ones(k1), -np.ones(k0)]
    return float(_sym_fro(D, sgn)), float(_sym_fro(Z1, np.ones(k1)))


def upd_float64_qr(Z1, Z0=None, s0=-1.0, x1_cols=None):
    """The same two numbers by the device's route in float64: R of ``[Z1, Z0]`` (NumPy's Householder QR), then
    ``||R S R^T||_F`` with ``S = diag(I, s0 I)`` and ``||R_1 R_1^T||_F`` of its first ``x1_cols`` (default k1) columns.
    ``s0`` and ``x1_cols`` exist for the seeded faults of the CPU tests."""
    Z1 = np.asarray(Z1, dtype=float)
    k1 = Z1.shape[1]
    k0 = 0 if Z0 is None else np.shape(Z0)[1]
    D = Z1 if k0 == 0 else np.hstack([Z1, np.asarray(Z0, dtype=float)])
    R = np.linalg.qr(D, mode="r")
    sgn = np.r_[np.ones(k1), s0 * np.ones(k0)]
    R1 = R[:, :k1 if x1_cols is None else x1_cols]
    return float(np.linalg.norm((R * sgn) @ R.T)), float(np.linalg.norm(R1 @ R1.T))


def upd_gram_route(Z1, Z0):
    """Seeded fault: the update norm from the Gram matrices, ``tr((S D^T D)^2)`` -- the squaring the QR route avoids."""
    D = np.hstack([Z1, Z0])
    sgn = np.r_[np.ones(Z1.shape[1]), -np.ones(Z0.shape[1])]
    G = D.T @ D
    return float(np.sqrt(abs(np.sum((sgn[:, None] * G) * (sgn[:, None] * G).T))))


# Shapes of the entry-by-entry tests: the split inside the first 128-column panel, on its edge, just past it, a thin
# factor on either side; at nv = 33 also k1 + k0 > nv with the second factor's panels noise after the projection
UPD_NV = (1, 33, 300, 1100)
UPD_WIDTHS = ((1, 0), (1, 1), (5, 0), (100, 100), (128, 128), (129, 127), (130, 3), (3, 130))
UPD_WIDTHS_33 = ((33, 33), (20, 30))
UPD_DELTAS = (1e-6, 1e-10, 1e-13)
UPD_WIDTH_LIMIT = 4096          # RICADI_MAX_UPD_COLS of include/ricadi.h


def upd_shapes():
    """[(nv, k1, k0)] of the tests, without what exceeds the documented width limit."""
    out = []
    for nv in UPD_NV:
        for k1, k0 in UPD_WIDTHS + (UPD_WIDTHS_33 if nv == 33 else ()):
            if k1 + k0 <= UPD_WIDTH_LIMIT:
                out.append((nv, k1, k0))
    return out


def _graded(rng, nv, k):
    """nv x k Gaussian columns graded over six orders of magnitude."""
    return rng.standard_normal((nv, k)) * np.logspace(0.0, -6.0, k)[None, :] if k > 1 else rng.standard_normal((nv, k))


def _reflector(rng, k):
    """An orthogonal k x k matrix from elementwise operations alone: I - 2 v v^T / (v^T v)."""
    v = rng.standard_normal(k)
    return np.eye(k) - 2.0 * np.outer(v, v) / float(np.sum(v * v))


def upd_cases(nv, k1, k0):
    """[(kind, Z1, Z0)] for one shape: 'independent' always (Z0 None for k0 = 0); with k0 = k1 also 'equal'
    (Z0 = Z1), 'rotated' (Z0 = Z1 Q, Q orthogonal: the same Z Z^T from another factor) and 'delta<d>'
    (Z0 = Z1 + d * graded noise) for d of UPD_DELTAS."""
    rng = np.random.default_rng(100000 * nv + 1000 * k1 + k0)
    Z1 = np.ascontiguousarray(_graded(rng, nv, k1))
    if k0 == 0:
        return [("independent", Z1, None)]
    cases = [("independent", Z1, np.ascontiguousarray(_graded(rng, nv, k0)))]
    if k0 == k1:
        cases.append(("equal", Z1, Z1.copy()))
        cases.append(("rotated", Z1, np.ascontiguousarray(Z1 @ _reflector(rng, k1))))
        for d in UPD_DELTAS:
            cases.append(("delta%g" % d, Z1, np.ascontiguousarray(Z1 + d * _graded(rng, nv, k1))))
    return cases


# ------------------------------------------------------------------------------------------------ the Newton loop
def _margin(value, tol):
    if not np.isfinite(value) or value <= 0.0 or tol <= 0.0:
        return np.inf
    return max(value / tol, tol / value)


class Problem:
    """The dense pieces of one call form (radi_model.call_forms) that do not change from step to step: the matrices,
    the null-space basis of J (computed once) and the projected W."""

    def __init__(self, form):
        self.form = form
        self.A, self.E, self.J = _dn(form["calA"]), _dn(form["calE"]), _dn(form["J"])
        self.B, self.W = np.asarray(form["B"], dtype=float), np.asarray(form["W"], dtype=float)
        self.old = None if form["old"] is None else _dn(form["old"])
        self.ms = np.asarray(form["ms"], dtype=float)
        self.base = AdiResModel(self.A, self.E, self.J)
        self.Wp = self.base.project(self.W)

    def closed_loop(self, Kall):
        """AdiResModel of ``cal A - Kall B^T`` on the basis this problem already has."""
        if Kall is None:
            return self.base
        m = AdiResModel.__new__(AdiResModel)
        m.A, m.E, m.Th = self.A - Kall @ self.B.T, self.E, self.base.Th
        m.Ah, m.Eh = m.Th.T @ m.A @ m.Th, self.base.Eh
        m._lu = {}
        return m


def newton(form, Z0=None, newZ_reltol=1e-8, adi_max_steps=ADI_MAX_STEPS, nwtn_max_steps=16, nwtn_upd_reltol=5e-8,
           nwtn_upd_abstol=1e-7, sweep_width=1, problem=None):
    """The loop.  Returns dict(steps = [dict(adi_steps, adi_margin, rel_newZ, upd, upd_rel, x1, Z, width)], rule,
    problem).  ``adi_margin``: the smallest factor between ``newZ_reltol`` and anything the ADI's rule compared
    with it in that step; ``rel_newZ``: the step form's whole sequence (adi_max_steps entries)."""
    pb = problem if problem is not None else Problem(form)
    Zk = None if Z0 is None else np.asarray(Z0, dtype=float)
    steps, rule = [], "max_steps"
    for _ in range(nwtn_max_steps):
        if Zk is not None:
            K = pb.E @ (Zk @ (Zk.T @ pb.B))
            Kall = K if pb.old is None else K - pb.old
            rhs = np.hstack([pb.Wp, K])
        else:
            Kall = None if pb.old is None else -pb.old
            rhs = pb.Wp
        mdl = pb.closed_loop(Kall)
        ref = mdl.step_form(rhs, pb.ms, adi_max_steps)
        if sweep_width > 1:
            from adi_sweep_model import sweep_schedule
            sch = sweep_schedule(ref["rel_newZ"], ref["hist"], pb.ms, sweep_width, newZ_reltol=newZ_reltol,
                                 max_steps=adi_max_steps, m=rhs.shape[1])
            k, margin = sch["steps"], sch["margin"]
        else:
            k, _ = stopping_step(ref["rel_newZ"], ref["hist"], newZ_reltol, 0.0, adi_max_steps)
            margin = min(_margin(v, newZ_reltol) for v in ref["rel_newZ"][:k])
        Znew = np.hstack(ref["Z"][:k])
        upd, x1 = upd_float64_qr(Znew, Zk)
        upd_rel = upd / x1 if x1 > 0.0 else 0.0
        steps.append(dict(adi_steps=k, adi_margin=margin, rel_newZ=ref["rel_newZ"], upd=upd, upd_rel=upd_rel, x1=x1,
                          Z=Znew, width=rhs.shape[1]))
        Zk = Znew
        if upd < nwtn_upd_abstol or upd_rel < nwtn_upd_reltol:
            rule = "abstol" if upd < nwtn_upd_abstol else "reltol"
            break
    return dict(steps=steps, rule=rule, problem=pb)


def adi_tolerance(run):
    """(lo, hi, tol) of the step form: the tolerances for which every Newton step of `run` takes the ADI steps it
    took, and their geometric middle.  The iterates do not depend on the tolerance inside the interval, so the run
    with `tol` is the same run.  None where the interval is empty."""
    lo = max(s["rel_newZ"][s["adi_steps"] - 1] for s in run["steps"])
    hi = min(min(s["rel_newZ"][:s["adi_steps"] - 1]) for s in run["steps"])
    if not lo < hi:
        return None
    return float(lo), float(hi), float(np.sqrt(lo * hi))


def newton_tolerance(upd_rel):
    """(step, tol): the relative Newton tolerance of a history case and the (1-based) step it stops at.  The last
    step k whose decision and the one before it have a margin of NEWTON_MARGIN on the geometric middle of
    ``max(upd_rel_k, UPD_REL_FLOOR)`` and ``upd_rel_{k-1}``; the floor keeps the tolerance where the device's inexact
    solves do not decide.  None if no step has it."""
    for k in range(len(upd_rel), 1, -1):
        lo, hi = max(upd_rel[k - 1], UPD_REL_FLOOR), min(upd_rel[:k - 1])
        if hi / lo >= NEWTON_MARGIN ** 2:
            return k, float(np.sqrt(lo * hi))
    return None


def history_case(form, sweep_width=1, nominal=1e-8, problem=None):
    """The run of one history case with its tolerances chosen by the two rules above: dict(newZ_reltol,
    nwtn_upd_reltol, run (the model's run with them), adi_margin, newton_margin).  The nominal ADI tolerance only
    fixes the step counts; the tolerance used is the middle of the interval that gives them."""
    pb = problem if problem is not None else Problem(form)
    if sweep_width > 1:
        nominal = _sweep_tolerance(form, pb, sweep_width, nominal)
    free = newton(form, newZ_reltol=nominal, nwtn_max_steps=4, nwtn_upd_reltol=1e-14, nwtn_upd_abstol=0.0,
                  sweep_width=sweep_width, problem=pb)
    nt = newton_tolerance([s["upd_rel"] for s in free["steps"]])
    if nt is None:
        return None
    k, rtol = nt
    tol = nominal
    if sweep_width == 1:
        # the step counts with the widest interval, judged on the nominal run's sequences; then that run itself
        tol = _widest(free["steps"][:k])
        free = newton(form, newZ_reltol=tol, nwtn_max_steps=k, nwtn_upd_reltol=0.0, nwtn_upd_abstol=0.0, problem=pb)
        iv = adi_tolerance(free)
        if iv is None:
            return None
        tol = iv[2]
    run = newton(form, newZ_reltol=tol, nwtn_max_steps=6, nwtn_upd_reltol=rtol, nwtn_upd_abstol=0.0,
                 sweep_width=sweep_width, problem=pb)
    assert len(run["steps"]) == k and run["rule"] == "reltol"
    return dict(newZ_reltol=tol, nwtn_upd_reltol=rtol, run=run,
                adi_margin=min(s["adi_margin"] for s in run["steps"]),
                newton_margin=min(_margin(s["upd_rel"], rtol) for s in run["steps"]))


def _widest(steps, grid=np.logspace(-10.0, -6.0, 161)):
    """The tolerance of the grid at which the step-form decisions of these Newton steps have the largest smallest
    margin."""
    def worst(t):
        out = np.inf
        for s in steps:
            k, _ = stopping_step(s["rel_newZ"], s["rel_newZ"], t, 0.0)
            out = min(out, min(_margin(v, t) for v in s["rel_newZ"][:k]))
        return out
    return float(max(grid, key=worst))


def _sweep_tolerance(form, pb, G, nominal):
    """Sweep form: of a geometric grid of tolerances around the nominal one, the one whose run has the largest
    smallest margin (sweep_schedule's: predictions and revealed values alike)."""
    best = None
    for t in nominal * np.logspace(-1.0, 1.0, 5):
        r = newton(form, newZ_reltol=float(t), nwtn_max_steps=2, nwtn_upd_reltol=1e-14, nwtn_upd_abstol=0.0,
                   sweep_width=G, problem=pb)
        mg = min(s["adi_margin"] for s in r["steps"])
        if best is None or mg > best[0]:
            best = (mg, float(t))
    return best[1]


# ------------------------------------------------------------------------------------------------ the cases
# (N, index into radi_model.call_forms(N), sweep width) of the GPU history tests; N = 8 comes from the fixture
HISTORY_CASES = [(4, 0, 1), (4, 1, 1), (4, 2, 1), (8, 0, 1), (8, 1, 1), (8, 1, 4)]
FORM_NAMES = ("steady", "dre", "dre_old")


def case_key(N, i, G):
    return "n%d_%s_g%d" % (N, FORM_NAMES[i], G)


def compress_factor(Z, rel=GOLDEN_TRUNC):
    """Z V_r with the right singular vectors of the singular values above rel * sigma_1."""
    U, s, _ = np.linalg.svd(Z, full_matrices=False)
    r = int(np.sum(s > rel * s[0]))
    return U[:, :r] * s[:r]


def pack(case, last_only=False):
    """The arrays of one case as the fixture holds them (last_only: no iterate but the last)."""
    st = case["run"]["steps"]
    out = dict(tol=np.array([case["newZ_reltol"], case["nwtn_upd_reltol"], case["adi_margin"], case["newton_margin"]]),
               hist=np.array([[s["upd"], s["upd_rel"], s["adi_steps"], s["width"], s["x1"], 0.0] for s in st]))
    for k, s in enumerate(st):
        if last_only and k < len(st) - 1:
            continue
        Zc = compress_factor(s["Z"])
        out["Z%d" % k] = Zc
        out["hist"][k, 5] = upd_float64_qr(Zc, s["Z"])[0] / s["x1"]
    return out


def unpack(arrs, key):
    """dict(newZ_reltol, nwtn_upd_reltol, adi_margin, newton_margin, steps = [dict(upd, upd_rel, adi_steps, width, x1,
    Z (truncated; None where the fixture does not keep it), trunc = ||Z Z^T - (model's) Z Z^T||_F / x1)]) of one case from the fixture (or from :func:`pack`'s output with the key prefixed)."""
    tol, hist = arrs[key + "/tol"], arrs[key + "/hist"]
    steps = [dict(upd=h[0], upd_rel=h[1], adi_steps=int(h[2]), width=int(h[3]), x1=h[4], trunc=h[5],
                  Z=arrs["%s/Z%d" % (key, k)] if "%s/Z%d" % (key, k) in arrs else None)
             for k, h in enumerate(hist)]
    return dict(newZ_reltol=float(tol[0]), nwtn_upd_reltol=float(tol[1]), adi_margin=float(tol[2]),
                newton_margin=float(tol[3]), steps=steps)


def live_case(N, i, G):
    """A case computed now, in the fixture's form."""
    import radi_model as rm
    case = history_case(rm.call_forms(N)[i], sweep_width=G)
    assert case is not None, "no tolerance with the margins for " + case_key(N, i, G)
    key = case_key(N, i, G)
    return unpack({key + "/" + k: v for k, v in pack(case).items()}, key)


def make():
    """Writes tests/golden/newton_model.npz: the N = 8 cases of HISTORY_CASES (15 to 30 s each on the host)."""
    import radi_model as rm
    forms = rm.call_forms(8)
    out = {}
    for N, i, G in HISTORY_CASES:
        if N != 8:
            continue
        case = history_case(forms[i], sweep_width=G)
        assert case is not None, case_key(N, i, G)
        for k, v in pack(case, last_only=G > 1).items():
            out[case_key(N, i, G) + "/" + k] = v
    np.savez(GOLDEN, **out)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    make()
