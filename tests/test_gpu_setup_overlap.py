"""GPU tests of the per-shift setup beside the projection solve (the default) against the serial order
(RICADI_SETUP_OVERLAP=0, read when a context is created): one Newton-ADI step, the same ADI steps and shift-solves,
the same gain to the solves' accuracy.  The projection operator's coarse inverse is computed alone in the overlapped
order and inside the batch of the shifts in the serial one (rocBLAS may choose other GEMM kernels for the two batch
sizes), so the projected right-hand side differs in the last bits; a GMRES group that ends near its tolerance can
then take an iteration more or less.  The total of a Newton step varies by a few iterations from run to run in either
order anyway (measured: cfg1 2 664 / 2 662 and 2 665 / 2 661, cfg2 7 702 / 7 701 and 7 701 / 7 704 overlapped /
serial; K 1e-15 apart)."""
import numpy as np
import pytest

from optconpy_amd import _lib, problems as pb
from oracle import lin_alg_utils as olau

pytestmark = pytest.mark.gpu


def _inputs(pr):
    mct = olau.app_prj_via_sadpnt(amat=pr.M, jmat=pr.J, rhsv=pr.mc_mat.T, transposedprj=True)
    tb = olau.apply_invsqrt_fromright(pr.rmat, pr.b_mat, output="dense")
    trct = olau.apply_invsqrt_fromright(pr.y_masmat, mct, output="dense")
    return tb, trct


def _newton_step(pr, tb, trct, ms, monkeypatch, overlap):
    monkeypatch.setenv("RICADI_SETUP_OVERLAP", "1" if overlap else "0")
    d = dict(pb.default_nwtn_adi_dict(), ms=ms, nwtn_max_steps=1, sweep_width=16)
    try:
        with _lib.Context(0) as ctx:
            ctx.set_operator((-pr.A - pr.Nc).T.tocsr(), pr.M.T.tocsr(), pr.J)
            Z, info = ctx.ric_newtonadi(ms, tb, trct, _lib.adi_params(d))
            K = -ctx.gain(tb)
    finally:
        monkeypatch.delenv("RICADI_SETUP_OVERLAP", raising=False)
    return K, info


def _check(pr, tb, trct, ms, monkeypatch, kbar):
    K1, i1 = _newton_step(pr, tb, trct, ms, monkeypatch, True)
    K0, i0 = _newton_step(pr, tb, trct, ms, monkeypatch, False)
    d = np.linalg.norm(K1 - K0) / np.linalg.norm(K0)
    print("overlap / serial: gmres iterations %d / %d, K rel diff %.2e" % (i1["gmres_iters"], i0["gmres_iters"], d))
    for key in ("nwtn_steps", "adi_steps", "shift_solves", "cols"):
        assert i1[key] == i0[key], (key, i1[key], i0[key])
    # the total varies run to run in either order (FP64 atomics in the recompression's Gram matrices)
    assert abs(i1["gmres_iters"] - i0["gmres_iters"]) <= 5e-3 * i0["gmres_iters"], (i1["gmres_iters"], i0["gmres_iters"])
    assert d < kbar, d


def test_overlap_cfg1(cfg1, monkeypatch):
    pr, tb, trct, ms = cfg1
    _check(pr, tb, trct, list(ms), monkeypatch, 1e-12)


def test_overlap_cfg2_sixteen_shifts(monkeypatch):
    """The benchmark's size (N = 58) with 16 shifts: the setup batch of the ADI shifts beside the projection."""
    pr = pb.ricc_problem(58, 0.05, NU=4, NY=4, alphau=1e-2)
    tb, trct = _inputs(pr)
    _check(pr, tb, trct, list(pb.logshifts(1.0, 3e3, 16)), monkeypatch, 1e-10)
