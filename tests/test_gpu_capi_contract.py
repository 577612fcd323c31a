"""What the C entry points promise whatever they compute (optconpy_amd/csrc/solver_capi*.inl), on the smallest
operator of the GPU suite (N = 15, n = 1937: the problem of test_gpu_adi_res.py), for 1 and 2 groups of 1 and 16
columns:

* the seven batched entries refuse ``ng`` outside 1 .. 16 and ``m`` outside 1 .. 128 with ``ValueError`` before
  anything is launched, and leave the context as it was;
* the three ways out of the resident factor hand out the same numbers;
* an output panel that the iteration keeps in FP32 comes back widened, not recomputed.
"""
import numpy as np
import pytest

from optconpy_amd import _lib, problems as pb
from oracle import lin_alg_utils as olau

pytestmark = pytest.mark.gpu

CASES = [(1, 1), (2, 1), (1, 16), (2, 16)]          # (groups, panel width)
ALPHAS = [-2.0, -400.0]
BAD = [dict(ng=0), dict(ng=17), dict(m=0), dict(m=129)]
SENTINEL = 7.25


@pytest.fixture(scope="module")
def problem():
    """Operator and the projected right-hand side of the Lyapunov equation (computed once, read only)."""
    pr = pb.ricc_problem(15, 0.05, NU=2, NY=2)
    mct = olau.app_prj_via_sadpnt(amat=pr.M, jmat=pr.J, rhsv=pr.mc_mat.T, transposedprj=True)
    W = olau.apply_invsqrt_fromright(pr.y_masmat, mct, output="dense")
    ops = ((-pr.A - pr.Nc).T.tocsr(), pr.M.T.tocsr(), pr.J.tocsr())
    assert ops[0].shape[0] + ops[2].shape[0] == 1937 and W.shape == (pr.NV, 4)
    return dict(ops=ops, W=np.ascontiguousarray(W), nv=pr.NV, n=1937)


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _host(ctx, t):
    ctx.synchronize()
    return t.cpu().numpy().copy()


class Entries:
    """The seven batched entries of ``_lib.Context`` on one context: ``call(name, ng, m)`` makes the call on buffers
    large enough for any (ng, m) of this file -- the refused ones included, so that a check that let one through would
    show as a wrong answer and not as a fault -- and returns what the call left behind that is the same from run to
    run (a measured time is reduced to "positive")."""
    NAMES = ("precond_apply_batch_dev", "op_apply_batch_dev", "shift_solve_batch_dev", "recycle_guess_dev",
             "time_spmm_batch_dev", "time_kernel_dev", "arnoldi_probe_begin_dev")

    def __init__(self, ctx, n, nv):
        import torch
        self.ctx, self.n, self.nv = ctx, n, nv
        rng = np.random.default_rng(15)
        self.inp = _dev(rng.standard_normal(17 * n * 129))
        self.out = torch.empty_like(self.inp)
        self.small = _dev(np.ones(17 * 129))

    def call(self, name, ng, m):
        ctx, n, i, o = self.ctx, self.n, self.inp.data_ptr(), self.out.data_ptr()
        al, be = (ALPHAS * 9)[:ng], [1.0] * ng
        self.out.fill_(SENTINEL)
        used = slice(0, max(ng, 0) * n * max(m, 0))
        if name == "precond_apply_batch_dev":
            form = ctx.precond_apply_batch_dev(al, be, i, n * m, m, o)
            return form, _host(ctx, self.out[used])
        if name == "op_apply_batch_dev":
            var = ctx.op_apply_batch_dev(al, be, i, n * m, m, o, n * m)
            return var, _host(ctx, self.out[used])
        if name == "shift_solve_batch_dev":
            its, rr = ctx.shift_solve_batch_dev(al, be, i, 0, m, o)
            assert rr.max() <= 1e-10, rr.max()
            return list(its), rr.copy(), _host(ctx, self.out[used])
        if name == "recycle_guess_dev":
            # (no recycling depth set: no guess, the panels stay as they are)
            rank = ctx.recycle_guess_dev(al, be, i, m, o)
            return rank, _host(ctx, self.out[used])
        if name == "time_spmm_batch_dev":
            ms = ctx.time_spmm_batch_dev(al, be, i, m, o, 2)
            info = ctx.setup_info()
            return ms > 0.0, info["k1_variant"], info["fp32_operator_output"]
        if name == "time_kernel_dev":
            ms = ctx.time_kernel_dev("spmm", al, be, m, nvec=2, reps=2)
            info = ctx.setup_info()
            return ms > 0.0, info["k1_variant"], info["fp32_operator_output"]
        assert name == "arnoldi_probe_begin_dev"
        ctx.arnoldi_probe_begin_dev(al, be, m, i, self.small.data_ptr())
        return self.probe_state(ng, m)

    def probe_state(self, ng, m):
        """Column scales and the first basis vector of the probe cycle in flight."""
        got = []
        for what, cnt in (("scale", ng * m), ("basis", ng * self.n * m)):
            assert self.ctx.arnoldi_probe_read_dev(what, self.out.data_ptr(), self.out.numel()) == cnt
            got.append(_host(self.ctx, self.out[:cnt]))
        return got


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


@pytest.mark.parametrize("ng,m", CASES)
def test_argument_table(problem, ng, m):
    """Each entry: a valid call, the four refused ones (ValueError; the branch trace and the exchange count as they
    were, so nothing was launched), the valid call again with the same result bit for bit."""
    with _lib.Context(0) as ctx:
        ctx.set_operator(*problem["ops"])
        e = Entries(ctx, problem["n"], problem["nv"])
        for name in Entries.NAMES:
            before = e.call(name, ng, m)
            state = (ctx.solve_trace(), ctx.exchange_count())
            for bad in BAD:
                with pytest.raises(ValueError):
                    e.call(name, bad.get("ng", ng), bad.get("m", m))
                assert (ctx.solve_trace(), ctx.exchange_count()) == state, (name, bad)
            if name == "arnoldi_probe_begin_dev":
                assert _same(e.probe_state(ng, m), before), "a refused begin disturbed the cycle in flight"
            after = e.call(name, ng, m)
            assert _same(before, after), (name, ng, m)
            if name in ("precond_apply_batch_dev", "op_apply_batch_dev", "shift_solve_batch_dev"):
                assert np.all(np.isfinite(after[-1])) and not np.any(after[-1] == SENTINEL), name
            if name == "recycle_guess_dev":
                assert after[0] == 0 and np.all(after[1] == SENTINEL)


def test_operator_required(problem):
    """On a fresh context every entry that needs an operator says so."""
    with _lib.Context(0) as ctx:
        e = Entries(ctx, problem["n"], problem["nv"])
        for name in Entries.NAMES:
            with pytest.raises(RuntimeError, match="set the operator first"):
                e.call(name, 2, 16)
        for call in (lambda: ctx.spmm_dev(-1.0, 1.0, e.inp.data_ptr(), 2, e.out.data_ptr()),
                     lambda: ctx.shift_solve_dev(-1.0, 1.0, e.inp.data_ptr(), 2, e.out.data_ptr()),
                     lambda: ctx.time_spmm_dev(-1.0, 1.0, e.inp.data_ptr(), 2, e.out.data_ptr(), 1),
                     lambda: ctx.panel_norms_dev(e.inp.data_ptr(), problem["nv"], 2),
                     lambda: ctx.gain_dev(1.0, e.inp.data_ptr(), 2, 2, e.inp.data_ptr(), 2, e.out.data_ptr()),
                     lambda: ctx.set_lowrank(None, None),
                     lambda: ctx.precond_structure(0),
                     lambda: ctx.arnoldi_probe_read_dev("scale", e.out.data_ptr(), 64)):
            with pytest.raises(RuntimeError, match="set the operator first"):
                call()


@pytest.mark.parametrize("width", [1, 16])
def test_one_download_three_doors(problem, width):
    """The factor a ``lyap_adi`` returns, ``factor_get()`` and ``factor_get_dev`` copied back are copies of the
    resident factor: bitwise equal."""
    import torch
    prm = _lib.adi_params(dict(adi_max_steps=16, adi_newZ_reltol=0.0, sweep_width=width))
    with _lib.Context(0) as ctx:
        ctx.set_operator(*problem["ops"])
        Z, info = ctx.lyap_adi(pb.logshifts(1.0, 1e3, 16), problem["W"], prm, fetch=True)
        assert Z.shape == (problem["nv"], 16 * 4) == (problem["nv"], info["cols"]) and np.all(np.isfinite(Z))
        assert np.linalg.norm(Z) > 0.0
        Zg = ctx.factor_get()
        Zt = torch.full(Z.shape, SENTINEL, dtype=torch.float64, device="cuda:0")
        ctx.factor_get_dev(Zt.data_ptr(), info["cols"])
        Zd = _host(ctx, Zt)
    assert np.array_equal(Z, Zg)
    assert np.array_equal(Z, Zd)


def test_widened_output_is_fp32_exact(problem):
    """Where the iteration keeps the preconditioner's output as an FP32 panel (``x32`` of the form word: the hot
    16-column shape of test_gpu_precond_parity.py's default configuration), ``precond_apply_batch_dev`` hands that
    panel back widened: every entry of an active group is an FP32 number, and the groups left out keep what the caller
    put there."""
    import torch
    n = problem["n"]
    rng = np.random.default_rng(16)
    seen = []
    with _lib.Context(0) as ctx:
        ctx.set_operator(*problem["ops"])
        for ng, m in CASES:
            for active in [None] + ([[1]] if ng == 2 else []):
                Rd = _dev(rng.standard_normal((ng, n, m)))
                Zd = torch.full((ng, n, m), SENTINEL, dtype=torch.float64, device="cuda:0")
                form = ctx.precond_apply_batch_dev(ALPHAS[:ng], [1.0] * ng, Rd.data_ptr(), n * m, m, Zd.data_ptr(),
                                                   active=active)
                Z = _host(ctx, Zd)
                groups = range(ng) if active is None else active
                for g in range(ng):
                    if g not in groups:
                        assert np.all(Z[g] == SENTINEL), (ng, m, active, g)
                        continue
                    assert np.all(np.isfinite(Z[g])) and not np.any(Z[g] == SENTINEL), (ng, m, active, g)
                    if form["x32"]:
                        assert np.array_equal(Z[g], Z[g].astype(np.float32).astype(np.float64)), (ng, m, active, g)
                if form["x32"]:
                    seen.append((ng, m, active))
    print("[capi contract] FP32 output panel in the cases (ng, m, active):", seen)
    assert seen, "no case of this test reports the FP32 output panel"
    assert any(a is not None for _, _, a in seen), "no case with a strict subset of the groups reports it"
