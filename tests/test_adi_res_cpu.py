"""The dense FP64 model of the ADI's residual history (``tests/adi_res_model.py``) against the densely formed
projected residual, the sweep form's prefix formula against the step form, the Python sweep driver's residual rule,
and the new field of the parameter struct.  CPU only."""
import numpy as np
import pytest
import torch

from optconpy_amd import _lib, problems as pb
from optconpy_amd.shift_parallel import lyap_adi_shift_parallel, prefix_residuals
from oracle import lin_alg_utils as olau

from adi_res_model import AdiResModel, cauchy_numpy, gram_fro, stopping_step
from identities import dense_projected_residual, leray_projector

MS = pb.logshifts(1.0, 500.0, 8)
STEPS = 16


@pytest.fixture(scope="module")
def case():
    pr = pb.ricc_problem(10, 0.05, NU=2, NY=2)
    F = (-pr.A - pr.Nc).tocsr()
    mct = olau.app_prj_via_sadpnt(amat=pr.M, jmat=pr.J, rhsv=pr.mc_mat.T, transposedprj=True)
    W = olau.apply_invsqrt_fromright(pr.y_masmat, mct, output="dense")
    mdl = AdiResModel(F.T, pr.M.T, pr.J)
    W0 = mdl.project(W)
    return dict(pr=pr, F=F, W=W, mdl=mdl, W0=W0, ref=mdl.step_form(W0, MS, STEPS))


def test_history_is_the_dense_projected_residual(case):
    """Entry j of the model's history is ||P^T (F^T X_j M + M^T X_j F + W W^T) P||_F / ||P^T W W^T P||_F formed
    densely from Z_j = [Z_1 .. Z_j]: both sides are exact-solve FP64, 1e-10 relative."""
    pr, ref = case["pr"], case["ref"]
    P = leray_projector(pr.M, pr.J)
    for j in range(1, STEPS + 1):
        Z = np.hstack(ref["Z"][:j])
        res, rhs = dense_projected_residual(Z, case["F"], pr.M, case["W"], P)
        assert abs(res / rhs - ref["hist"][j - 1]) <= 1e-10 * ref["hist"][j - 1], j
    assert np.isclose(rhs, ref["rhs"], rtol=1e-12)
    assert ref["hist"][-1] < 1e-3 * ref["hist"][0]          # the run does converge


def _prefix_tolerance(case, G):
    """Bound on the relative difference between the prefix formula and the step form, entry by entry.  The Gram
    matrix of P = [W, E U_1 .. E U_G] carries an error of nv eps ||P_x|| ||P_y|| per block (dot products of length
    nv), and the exact solves behind U_i an error of cond eps ||U_i|| (cond <= 1e4: the pencil's eigenvalues span
    2.7 .. 1.4e3, the shifts 1 .. 500).  Both are amplified by the coefficients of W_j = sum_x d_x P_x, whose terms
    cancel: the error of W_j^T W_j is (nv + cond) eps S_j^2 with S_j = sum_x |d_x| ||P_x||_F, relative to
    ||W_j^T W_j||_F = h_j rhs."""
    mdl, ref = case["mdl"], case["ref"]
    nv = case["W0"].shape[0]
    tol = np.zeros(STEPS)
    for s0 in range(0, STEPS, G):
        Wb = ref["W"][s0]
        ps = [MS[(s0 + i) % len(MS)] for i in range(min(G, STEPS - s0))]
        T = [mdl.E @ mdl.solve(p, Wb) for p in ps]
        for j in range(1, len(ps) + 1):
            c = cauchy_numpy(ps[:j])[1]
            S = np.linalg.norm(Wb) + sum(abs(ci) * np.linalg.norm(Ti) for ci, Ti in zip(c, T))
            tol[s0 + j - 1] = (nv + 1e4) * np.finfo(float).eps * S * S / (ref["hist"][s0 + j - 1] * ref["rhs"])
    return tol


@pytest.mark.parametrize("G", [2, 8])
def test_prefix_formula_reproduces_the_step_form(case, G):
    """Sweep form: the Gram matrix of [W, E U_i] with the closed-form coefficients C_j^-1 1 gives the step form's
    history -- with the library's ricadi_host_cauchy and with a dense solve of the Cauchy system."""
    ref = case["ref"]
    tol = _prefix_tolerance(case, G)
    assert tol.max() < 1e-3                                       # the bound itself says something
    for cauchy in (_lib.host_cauchy, cauchy_numpy):
        h = case["mdl"].sweep_form_history(case["W0"], MS, G, STEPS, cauchy=cauchy)
        dev = np.abs(h - ref["hist"]) / ref["hist"]
        assert (dev <= tol).all(), (dev / tol).max()
    # both rules end the two forms after the same step
    k, rule = stopping_step(ref["rel_newZ"], h, 0.0, float(np.sqrt(ref["hist"][5] * ref["hist"][6])))
    assert (k, rule) == stopping_step(ref["rel_newZ"], ref["hist"], 0.0, float(np.sqrt(ref["hist"][5] * ref["hist"][6])))


def test_prefix_residuals_of_the_python_driver(case):
    """optconpy_amd.shift_parallel.prefix_residuals (host arithmetic of the Python sweep driver) on the model's
    Gram matrix."""
    mdl, ref = case["mdl"], case["ref"]
    ps = list(MS)
    T = [mdl.E @ mdl.solve(p, case["W0"]) for p in ps]
    Pn = np.hstack([case["W0"]] + T)
    got = prefix_residuals(Pn.T @ Pn, case["W0"].shape[1], ps) / ref["rhs"]
    assert np.allclose(got, ref["hist"][:len(ps)], rtol=_prefix_tolerance(case, len(ps))[:len(ps)].max(), atol=0.0)


class _ModelOps:
    """The operations lyap_adi_shift_parallel needs, on the dense model (torch CPU tensors)."""

    def __init__(self, mdl):
        self.mdl = mdl

    def solve(self, p, W):
        return torch.from_numpy(self.mdl.solve(p, W.numpy()))

    def lincomb(self, coef, U_all):
        return torch.einsum("s,snm->nm", torch.as_tensor(np.asarray(coef)), U_all)

    def fro2(self, T):
        return float((T * T).sum())

    def apply_E(self, coef, V, W):
        W += coef * torch.from_numpy(self.mdl.E @ V.numpy())

    def gram_fro(self, T):
        return gram_fro(T.numpy())


@pytest.mark.parametrize("width", [1, 4, 8])
def test_python_sweep_driver_stops_on_the_residual(case, width):
    """The Python sweep driver with the same rule: same stopping step as the model's step form, history, rule."""
    ref = case["ref"]
    k = 6
    assert ref["hist"][k - 1] / ref["hist"][k] >= 1.5 and ref["hist"][:k].min() > ref["hist"][k]
    tol = float(np.sqrt(ref["hist"][k - 1] * ref["hist"][k]))
    blocks, info = lyap_adi_shift_parallel(_ModelOps(case["mdl"]), MS, torch.from_numpy(case["W0"].copy()),
                                           adi_max_steps=STEPS, adi_newZ_reltol=0.0, adi_res_reltol=tol, width=width)
    assert info["adi_steps"] == k + 1 and info["adi_stopped_by"] == "res" and len(blocks) == k + 1
    assert np.allclose(info["adi_res_hist"], ref["hist"][:k + 1], rtol=1e-6)
    assert info["res_fro"] <= tol * ref["rhs"]
    # off by default: nothing recorded, the reference's rule alone
    blocks, info = lyap_adi_shift_parallel(_ModelOps(case["mdl"]), MS, torch.from_numpy(case["W0"].copy()),
                                           adi_max_steps=STEPS, adi_newZ_reltol=0.05, width=width)
    k_new, rule = stopping_step(ref["rel_newZ"], ref["hist"], 0.05, 0.0)
    assert rule == "newZ" and info["adi_steps"] == k_new and info["adi_stopped_by"] == "newZ"
    assert len(info["adi_res_hist"]) == 0


def test_params_struct_round_trips_the_new_field():
    p = _lib.adi_params(None)
    assert p.adi_res_reltol == 0.0                                  # off by default
    p = _lib.adi_params(dict(adi_res_reltol=1e-9, adi_newZ_reltol=0.0, sweep_width=16))
    assert (p.adi_res_reltol, p.adi_newZ_reltol, p.sweep_width) == (1e-9, 0.0, 16)
    q = _lib.RicadiAdiParams.from_buffer_copy(bytes(p))
    assert q.adi_res_reltol == 1e-9 and q.sweep_width == 16
    _lib.load().ricadi_default_adi_params(q)
    assert q.adi_res_reltol == 0.0 and q.adi_newZ_reltol == 1e-8
