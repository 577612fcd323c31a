"""The ADI's second stopping rule (``adi_res_reltol``: relative projected Lyapunov residual) and its per-step
residual history on the MI355X, against the dense FP64 model ``tests/adi_res_model.py``: step form and sweep form
(one Gram matrix of ``[W, E U_1 .. E U_G]`` per sweep, fixed summation order), the Newton driver, two ranks through
the library's exchange, and the defaults.  N = 15 (n = 1937), m = 4."""
import os
import subprocess
import sys

import numpy as np
import pytest

from optconpy_amd import _lib, backend, problems as pb
from oracle import lin_alg_utils as olau

from adi_res_model import AdiResModel, stopping_step

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 32
MS = pb.logshifts(1.0, 1e3, 16)
ONE_SHIFT = -50.0
# Largest relative deviation of the device history from the model's over the entries above 1e-6, measured on the
# MI355X (step form; sweep form of width 16), times 10.  The shift solves carry a 1e-10 GMRES tolerance and the
# sweep form's prefix formula cancels, so the figures are measured, not derived.
HIST_BOUND = {1: 10 * 2.049e-10, 16: 10 * 1.641e-06}


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def lyap_inputs():
    pr = pb.ricc_problem(15, 0.05, NU=2, NY=2)
    F = (-pr.A - pr.Nc).tocsr()
    mct = olau.app_prj_via_sadpnt(amat=pr.M, jmat=pr.J, rhsv=pr.mc_mat.T, transposedprj=True)
    W = olau.apply_invsqrt_fromright(pr.y_masmat, mct, output="dense")
    return pr, F, W


@pytest.fixture(scope="module")
def case():
    """Problem, model and the model's histories (computed once, read only)."""
    pr, F, W = lyap_inputs()
    assert pr.NV + pr.J.shape[0] == 1937 and W.shape[1] == 4
    mdl = AdiResModel(F.T, pr.M.T, pr.J)
    W0 = mdl.project(W)
    ref = mdl.step_form(W0, MS, STEPS)
    one = mdl.step_form(W0, [ONE_SHIFT], 200)
    return dict(pr=pr, F=F, W=W, mdl=mdl, W0=W0, ref=ref, one=one)


def _solve(case, **d):
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    pr = case["pr"]
    return pru.solve_proj_lyap_stein(amat=case["F"], mmat=pr.M, jmat=pr.J, wmat=case["W"], adi_dict=d)


@pytest.mark.parametrize("width", [1, 16])
def test_history_against_the_model(case, width):
    """Nothing stops early (tiny tolerance): every entry of the device history against the model's, and the last
    one against the factored residual of the returned factor (identity (2) of tests/identities.py)."""
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    backend.reset()
    pr, ref = case["pr"], case["ref"]
    out = _solve(case, ms=MS, adi_max_steps=STEPS, adi_newZ_reltol=0.0, adi_res_reltol=1e-300, sweep_width=width)
    h = out["adi_res_hist"]
    assert out["adi_steps"] == STEPS and out["adi_stopped_by"] == "max_steps" and h.shape == (STEPS,)
    big = ref["hist"] > 1e-6
    assert big.sum() >= 20
    dev = np.abs(h - ref["hist"]) / ref["hist"]
    print("width %d: largest relative deviation of the history over the entries above 1e-6: %.3e (all: %.3e)"
          % (width, dev[big].max(), dev.max()))
    factored = np.sqrt(abs(pru.comp_proj_lyap_res_norm(out["zfac"], case["F"], pr.M, case["W"], pr.J)))
    print("width %d: last entry * rhs %.6e, factored residual %.6e, res_fro %.6e, rhs %.6e"
          % (width, h[-1] * ref["rhs"], factored, out["res_fro"], ref["rhs"]))
    assert dev[big].max() <= HIST_BOUND[width]
    assert abs(h[-1] * ref["rhs"] - factored) <= 1e-5 * ref["rhs"]
    backend.reset()


def _gap_step(hist, first):
    """Smallest 1-based step k >= first with h_k / h_{k+1} >= 2 and every earlier entry above sqrt(h_k h_{k+1})."""
    for k in range(first, len(hist)):
        hk, hk1 = hist[k - 1], hist[k]
        if hk / hk1 >= 2.0 and hist[:k].min() > np.sqrt(hk * hk1):
            return k
    return None


@pytest.mark.parametrize("first", [4, 18])
def test_same_stopping_step_in_both_forms(case, first):
    """A tolerance in the middle of a gap of the model's history (a factor >= 2 between two steps): step form and
    sweep form end after the same step, inside the first sweep (first = 4) and inside the second (first = 18)."""
    backend.reset()
    ref = case["ref"]
    k = _gap_step(ref["hist"], first)
    assert k is not None and (k + 1) % 16 != 0 and (k + 1) // 16 == first // 16, k
    tol = float(np.sqrt(ref["hist"][k - 1] * ref["hist"][k]))
    assert stopping_step(ref["rel_newZ"], ref["hist"], 0.0, tol) == (k + 1, "res")
    for width in (1, 16):
        out = _solve(case, ms=MS, adi_max_steps=STEPS, adi_newZ_reltol=0.0, adi_res_reltol=tol, sweep_width=width)
        print("width %d: stopped after step %d by %s, residual %.3e (tolerance %.3e)"
              % (width, out["adi_steps"], out["adi_stopped_by"], out["res_fro"] / ref["rhs"], tol))
        assert out["adi_steps"] == k + 1 and out["adi_stopped_by"] == "res"
        assert out["zfac"].shape[1] == (k + 1) * 4
        assert out["res_fro"] <= tol * ref["rhs"]
        assert len(out["adi_res_hist"]) == k + 1 and out["adi_res_hist"][-1] <= tol
    backend.reset()


def test_the_residual_rule_changes_the_outcome(case):
    """A single shift (-50, the best single shift of the model's scan).  The reference's rule at 1e-8 goes on long
    after the equation is solved: the model ends it at step 171 with a relative residual of 4e-15.  The residual
    rule at 1e-8 ends the same run at the model's step, with the densely formed residual at or below 1e-8 and
    above it one step earlier.

    (The opposite case -- the reference's rule at 1e-8 ending a single-shift run while the dense relative residual
    is still above 1e-6 -- does not exist for this operator: in the model, for every single shift between -3 and
    -1e6, the rule at 1e-8 fires only once the residual is below 1e-13, or not at all within 3000 steps.)"""
    from identities import dense_projected_residual, leray_projector
    backend.reset()
    pr, one = case["pr"], case["one"]
    k_new, rule_new = stopping_step(one["rel_newZ"], one["hist"], 1e-8, 0.0)
    k_res, rule_res = stopping_step(one["rel_newZ"], one["hist"], 1e-8, 1e-8)
    assert (rule_new, rule_res) == ("newZ", "res") and k_res < k_new and one["hist"][k_new - 1] < 1e-12
    base = _solve(case, ms=[ONE_SHIFT], adi_max_steps=200, adi_newZ_reltol=1e-8)
    out = _solve(case, ms=[ONE_SHIFT], adi_max_steps=200, adi_newZ_reltol=1e-8, adi_res_reltol=1e-8)
    print("reference rule: %d steps (model %d); with the residual rule: %d steps (model %d), stopped by %s"
          % (base["adi_steps"], k_new, out["adi_steps"], k_res, out["adi_stopped_by"]))
    assert base["adi_stopped_by"] == "newZ" and abs(base["adi_steps"] - k_new) <= 2
    assert out["adi_stopped_by"] == "res" and out["adi_steps"] == k_res
    P = leray_projector(pr.M, pr.J)
    Z = out["zfac"]
    r_end, rhs = dense_projected_residual(Z, case["F"], pr.M, case["W"], P)
    r_before, _ = dense_projected_residual(Z[:, :-4], case["F"], pr.M, case["W"], P)
    print("dense relative residual: %.3e at the stopping step, %.3e one step earlier" % (r_end / rhs, r_before / rhs))
    assert r_end <= 1e-8 * rhs < r_before
    backend.reset()


ARE_FIXTURE = os.path.join(ROOT, "tests", "golden", "adi_res_n15_are_gain.npz")


def _are_inputs():
    from identities import dre_step_inputs
    pr = pb.ricc_problem(15, 0.05)
    kw, p = dre_step_inputs(pr, tau=0.05, with_old=True)
    B = np.sqrt(p["tau"]) * p["tb"]
    return pr, kw, p, B


def make_are_fixture():
    """Writes tests/golden/adi_res_n15_are_gain.npz: the gain M^T X B of the dense solution X of the projected
    Riccati equation of test_newton_adi_auto_vs_dense_are_n15 (identities.dense_projected_are: SciPy's Schur method
    on ker J, two minutes on the host -- hence recorded), with the norms of the inputs it was made from."""
    from identities import dense_projected_are
    pr, kw, p, B = _are_inputs()
    calA = p["ft"].toarray() + kw["mtxoldb"] @ B.T
    X = dense_projected_are(calA, p["MT"], pr.J, B, p["wmat"])
    np.savez(ARE_FIXTURE, K=p["MT"] @ (X @ B), b_fro=np.linalg.norm(B), w_fro=np.linalg.norm(p["wmat"]),
             old_fro=np.linalg.norm(kw["mtxoldb"]))


def test_newton_adi_with_the_residual_rule_vs_dense_are_n15():
    """The bar of test_newton_adi_auto_vs_dense_are_n15 with the inner ADI stopped on its residual alone; the dense
    solution's gain comes from the recorded fixture (make_are_fixture), checked to belong to these inputs."""
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    backend.reset()
    pr, kw, p, B = _are_inputs()
    fx = np.load(ARE_FIXTURE)
    assert np.isclose(fx["b_fro"], np.linalg.norm(B), rtol=1e-12)
    assert np.isclose(fx["w_fro"], np.linalg.norm(p["wmat"]), rtol=1e-12)
    assert np.isclose(fx["old_fro"], np.linalg.norm(kw["mtxoldb"]), rtol=1e-12)
    # (Newton tolerance: an update of 1e-8 relative is what inner solves at a residual of 1e-10 can resolve; the
    # 1e-11 of the test named above is never met with them and only runs the Newton loop to its step limit)
    d = dict(adi_max_steps=300, adi_newZ_reltol=0.0, adi_res_reltol=1e-10, nwtn_max_steps=30, nwtn_upd_reltol=1e-8,
             nwtn_upd_abstol=1e-14, ms="auto")
    out = pru.proj_alg_ric_newtonadi(nwtn_adi_dict=d, **kw)
    Z = out["zfac"]
    print("Newton steps %d, ADI steps %d, last solve: %d steps, stopped by %s at %.3e"
          % (out["nwtn_steps"], out["adi_steps"], len(out["adi_res_hist"]), out["adi_stopped_by"],
             out["adi_res_hist"][-1]))
    assert out["adi_stopped_by"] == "res" and out["adi_res_hist"][-1] <= 1e-10
    assert rel(p["MT"] @ (Z @ (Z.T @ B)), fx["K"]) < 1e-6
    backend.reset()


def test_two_ranks_stop_at_the_same_step_with_equal_histories(tmp_path):
    """World 2 on one GPU, the sweeps sharded by shift inside the library (gloo callback): both ranks end after the
    same step, by the residual rule, with bitwise equal histories -- each rank decides alone on the Gram matrix."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "adi_res_ranks.py"), str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    a, b = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    print("steps %d / %d, rule %s / %s, exchanges %d / %d" % (a["steps"], b["steps"], a["rule"], b["rule"],
                                                              a["sharded"], b["sharded"]))
    assert int(a["sharded"]) == 1 and int(b["sharded"]) == 1
    assert int(a["steps"]) == int(b["steps"]) and str(a["rule"]) == str(b["rule"]) == "res"
    assert 0 < int(a["steps"]) < STEPS and len(a["hist"]) == int(a["steps"])
    assert a["hist"].tobytes() == b["hist"].tobytes()
    assert a["hist"][-1] <= float(a["tol"]) < a["hist"][-2]


def test_defaults_compute_nothing_new(cfg1, golden):
    """Key absent: the cfg1 Lyapunov solve of test_gpu_parity (same steps, same gain against the golden file), no
    launch of the residual kernels, an empty history, no 'adi_res_hist' key."""
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    pr, tb, trct, ms = cfg1
    F = (-pr.A - pr.Nc).tocsr()
    for width in (1, 16):
        ctx = _lib.Context(0)
        try:
            ctx.set_operator(F.T.tocsr(), pr.M.T.tocsr(), pr.J)
            with pytest.raises(RuntimeError):
                ctx.adi_res_history()                 # RICADI_ESTATE before any ADI call
            d = dict(pb.default_nwtn_adi_dict(), ms=ms, sweep_width=width)
            Z, info = ctx.lyap_adi(ms, trct, _lib.adi_params(d))
            assert info["adi_steps"] == int(golden["lyap_steps"][0]) and info["adi_stopped_by"] == "newZ"
            K = -(pr.M.T @ (Z @ (Z.T @ tb.toarray())))
            assert rel(K, golden["K_lyap"]) < 1e-6
            assert ctx.adi_res_launches() == 0 and ctx.adi_res_history().size == 0
            # on request: same steps and factor, the history comes with it
            ctx.set_adi_res_history(True)
            Z2, info2 = ctx.lyap_adi(ms, trct, _lib.adi_params(d))
            assert info2["adi_steps"] == info["adi_steps"]
            assert rel(-(pr.M.T @ (Z2 @ (Z2.T @ tb.toarray()))), K) < 1e-8
            assert ctx.adi_res_history().size == info["adi_steps"] and ctx.adi_res_launches() > 0
        finally:
            ctx.close()
    backend.reset()
    out = pru.solve_proj_lyap_stein(amat=F, mmat=pr.M, jmat=pr.J, wmat=trct, adi_dict=dict(ms=ms))
    assert "adi_res_hist" not in out and out["adi_stopped_by"] == "newZ"
    backend.reset()
