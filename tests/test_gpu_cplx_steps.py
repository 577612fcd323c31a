"""GPU tests of the complex GMRES cycle (ricadi_cplx.hip: cplx_gmres_start_kernel, the CGS2 step, cplx_gmres_hess_kernel,
cplx_gmres_backsolve_kernel, cplx_update_kernel with sign = +1) STEP BY STEP against the extended-precision model of
tests/cplx_model.py.  The step probe of the C-ABI (``ricadi_cplx_probe_*_dev``) runs the functions ``cplx_solve`` is
made of on the solver's own workspace, with a panel ``W_j = noise + 3 v_j`` in the place of ``S P^-1 v_j``; after every
step everything the step wrote is read back and compared with the model, whose inputs are the device's own stored
arrays -- errors do not compound -- and everything it did not write must still read as NaN.  Every comparison is
``error / bound <= 1`` against a bound derived by counting roundings (cplx_model's comment block;
tests/test_cplx_model_cpu.py shows that a float64 twin of the kernels meets every bound at these shapes with a factor
two to spare and that the faults the bounds exist for do not).  Every check prints
``[cplx] case | check | measured | bound`` before it asserts.

Operators ``small_ops.synthetic(nv=n, np_=0, lumped=True)`` with n = 61, 130, 450 (one partial 128-row block; one full
block plus two rows; four blocks with a tail), ``gmres_restart = 10`` and one case at the default restart, mc = 1, 3,
8, three groups: group 1 leaves the table after step 3 and its whole state stays bitwise what it was; the cycle end
runs with k = (10, 4, 10) and again with k = (7, 4, 2).  One short cycle has the two exact rotation branches in one
panel (cplx_model.cycle_inputs).  DESIGN.md 3f has the table measured on MI355X.
"""
import ctypes as C
import time

import numpy as np
import pytest

import cplx_model as cm
import small_ops as so
from optconpy_amd import _lib

pytestmark = pytest.mark.gpu
REACHED = {"branches": set(), "closes": set()}
WORST = {}
CLOCK = {"t": 0.0}


def _say(name, check, value, bound):
    ok = bool(np.isfinite(value)) and value <= bound
    print("[cplx] %s | %s | %.3e | %.3e%s" % (name, check, value, bound, "" if ok else "  MISS"))
    return ok


def _cdev(a):
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.complex128, order="C")).to("cuda:0")
    torch.cuda.synchronize()
    return t


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A test that leaves the device in an error state ends the run: nothing more is started on it."""
    yield
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:            # pragma: no cover - only after a device fault
        pytest.exit("device error after a test, stopping: %r" % (e,), returncode=3)


def _operator(n):
    return so.synthetic(nv=n, np_=0, seed=700 + n, lumped=True)


class ProbeDevice:
    """The step probe behind the interface cplx_model.check_cycle drives."""

    def __init__(self, ctx):
        self.ctx = ctx

    def begin(self, R, bnorm):
        self.ctx.cplx_probe_begin_dev(_cdev(R), bnorm)

    def step(self, j, W, groups):
        # (a group that left the table has NaN in its panel: it is not in `groups`, and the entry must not read it)
        self.ctx.cplx_probe_step_dev(j, _cdev(W), groups)

    def close(self, ks, Z, X):
        import torch
        Xd = _cdev(X)
        self.ctx.cplx_probe_close_dev(ks, _cdev(Z), Xd)
        torch.cuda.synchronize()
        return Xd.cpu().numpy()

    def read(self, what, slot=0):
        return self.ctx.cplx_probe_read_dev(what, slot)


@pytest.mark.parametrize("case", cm.CYCLE_CASES, ids=[c["name"] for c in cm.CYCLE_CASES])
def test_cycle_against_the_model(case):
    """One cycle (cplx_model.check_cycle): the cycle start bitwise NumPy's; per step the CGS2 coefficients, the new
    basis vector (orthogonality, reconstruction), column j of R, cs, sn, gv within ``C1 (j + 2) eps ||h_col||`` (gv:
    ``|gv[j]|``), the residual estimate against the least-squares residual of the Hessenberg system of the device's
    own columns; after the cycle end ``|R y - g| <= C2 k eps (|R| |y| + |g|)`` and the correction within
    ``C_CPLX (k + 2) eps (|Z| |y| + |x|)``; a zero column gives y = 0 and leaves x bitwise; nothing else is written."""
    t0 = time.perf_counter()
    with _lib.Context(0, **case["opts"]) as ctx:
        ctx.set_operator(*_operator(case["n"]))
        rep = cm.run_case(ProbeDevice(ctx), case)
    dt = time.perf_counter() - t0
    CLOCK["t"] += dt
    REACHED["branches"] |= rep.branches
    REACHED["closes"] |= set(rep.closes)
    ok = [_say(case["name"], "%s: error / bound" % k, rep[k], 1.0) for k in cm.QUANTITIES]
    for k, v in rep.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("[cplx] %s | branches %s | cycle ends %s | %.2f s" % (case["name"], sorted(rep.branches), rep.closes, dt))
    assert set(rep) == set(cm.QUANTITIES)
    assert all(ok), {k: v for k, v in rep.items() if v > 1.0}
    if case["breakdowns"]:
        assert rep.branches == {"general", "zero", "breakdown"}


def test_invalid_arguments_are_refused():
    """RICADI_EINVAL (ValueError) before anything is launched: step / close / read before a begin, ng outside 1 .. 16,
    mc outside 1 .. 8, j outside 0 .. gmres_restart - 1, a group id outside 0 .. ng - 1 or listed twice, more vectors
    at the cycle end than steps were run, a slot or a quantity that does not exist; a complex solve ends the probe
    cycle (it takes the workspace); the cycle in flight survives the refused calls."""
    n, mc = 61, 3
    rng = np.random.default_rng(5)
    with _lib.Context(0, gmres_restart=10) as ctx:
        ctx.set_operator(*_operator(n))
        R, W = _cdev(cm._crandn(rng, 2, n, mc)), _cdev(cm._crandn(rng, 2, n, mc))
        Z, X = _cdev(cm._crandn(rng, 1, 2, n, mc)), _cdev(cm._crandn(rng, 2, n, mc))
        bn = np.ones((2, mc))
        for call in (lambda: ctx.cplx_probe_step_dev(0, W, [0]), lambda: ctx.cplx_probe_close_dev([0, 0], Z, X),
                     lambda: ctx.cplx_probe_read_dev("scale")):
            with pytest.raises(ValueError):
                call()
        for ng in (0, 17):
            with pytest.raises(ValueError):
                ctx.cplx_probe_begin_dev(_cdev(np.ones((ng, n, mc))), np.ones((ng, mc)))
        with pytest.raises(ValueError):
            ctx.cplx_probe_begin_dev(_cdev(np.ones((2, n, 9))), np.ones((2, 9)))
        with pytest.raises(ValueError):
            ctx.cplx_probe_step_dev(0, W, [0])                  # (none of the refused begins counts)
        ctx.cplx_probe_begin_dev(R, bn)
        before = ctx.cplx_probe_read_dev("V", 0)
        for j in (-1, 10):
            with pytest.raises(ValueError):
                ctx.cplx_probe_step_dev(j, W, [0, 1])
        for groups in ([-1], [2], [0, 2], [1, 1], []):
            with pytest.raises(ValueError):
                ctx.cplx_probe_step_dev(0, W, groups)
        with pytest.raises(ValueError):
            ctx.cplx_probe_close_dev([1, 0], Z, X)              # more vectors than steps run
        with pytest.raises(ValueError):
            ctx.cplx_probe_read_dev("V", 11)
        with pytest.raises(ValueError):
            cnt = C.c_int64(0)                                  # (a quantity beyond RICADI_CPROBE_NRM2)
            _lib._chk(_lib.load().ricadi_cplx_probe_read_dev(ctx._h, 10, 0, X.data_ptr(), 64, C.byref(cnt)))
        assert cm.same_bits(ctx.cplx_probe_read_dev("V", 0), before)
        ctx.cplx_probe_step_dev(0, W, [0, 1])
        ctx.cplx_probe_close_dev([1, 1], Z, X)
        assert np.isfinite(X.cpu().numpy().view(np.float64)).all()
        _, _, rr = ctx.shift_solve_cplx_batch_dev([-1j], _cdev(cm._crandn(rng, n, mc)))
        assert rr.max() <= 1e-10
        with pytest.raises(ValueError):
            ctx.cplx_probe_read_dev("scale")


def test_probe_leaves_a_later_solve_bitwise():
    """A solve after a whole probe cycle (begin, steps, cycle end: NaN-filled workspace, wider than the solve's) on
    the same context returns bitwise what a fresh context returns."""
    op = so.get("nv65_np24")
    rng = np.random.default_rng(43)
    R = _cdev(cm._crandn(rng, 2, op.nv, 3))
    case = cm._case(op.n, 8, steps=3, leave={}, ks_list=((3, 3, 3),))
    inp = cm.cycle_inputs(3, op.n, 8, 10, 7)

    def solve(with_probe):
        with _lib.Context(0, gmres_restart=10, **op.opts) as ctx:
            ctx.set_operator(*op.ops)
            if with_probe:
                assert cm.check_cycle(ProbeDevice(ctx), inp, 10, case["steps"], {}, case["ks_list"]).ok()
            X, its, rr = ctx.shift_solve_cplx_batch_dev([-1j, -30 + 30j], R)
            assert rr.max() <= 1e-10
            return X.cpu().numpy(), its

    (X1, its1), (X0, its0) = solve(True), solve(False)
    print("[cplx] nv65_np24 | solve after a probe cycle, iterations %s | fresh context %s" % (its1, its0))
    assert np.all(np.isfinite(X0.view(np.float64))) and its1 == its0
    assert np.array_equal(X1.view(np.float64), X0.view(np.float64))


def test_every_branch_and_close_shape_was_reached():
    """Over all cases above: the three rotation branches (general; r == 0; |cur| == 0 < b) and both shapes of the cycle
    end (all steps of the cycle: k = (10, 4, 10); truncated: k = (7, 4, 2)).  Prints the largest error / bound per
    quantity (the device column of DESIGN.md 3f) and the run time."""
    assert WORST, "the cycle cases of this module did not run in this session"
    print("[cplx] largest error / bound per quantity:")
    for k in cm.QUANTITIES:
        print("  %-22s %.3g" % (k, WORST[k]))
    print("[cplx] run time of the cycle cases: %.1f s" % CLOCK["t"])
    assert REACHED["branches"] == {"general", "zero", "breakdown"}, REACHED["branches"]
    assert {(10, 4, 10), (7, 4, 2)} <= REACHED["closes"], REACHED["closes"]
