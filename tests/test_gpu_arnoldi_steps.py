"""GPU tests of the Arnoldi / Givens kernels of the lockstep GMRES (ricadi_arnoldi.hip) STEP BY STEP against the
longdouble model of tests/arnoldi_model.py: cycle start, every step j = 0 .. 9 of a restart cycle in every kernel form,
the end-of-cycle completion, the back substitution and the correction.  The step probe of the C-ABI
(``ricadi_arnoldi_probe_*_dev``) runs the solver's own phase functions on the solver's own workspace with a panel
``W_j = noise + 3 v_j`` in the place of ``S P^-1 v_j``; after every step everything the step wrote is read back and
compared with the model, whose inputs are the device's own stored vectors and coefficients -- errors do not compound.
Every assertion is ``error / bound <= 1`` against a derived bound (arnoldi_model's docstring;
tests/test_arnoldi_model_cpu.py shows that a float64 implementation meets the bounds at these shapes and that the
faults they exist for do not); frozen columns are compared exactly.

Operators: ``saddle_model.th_operators(N)`` for N = 3, 4, 11 (n = 65, 122, 1025 rows; n % 64 = 1, 58, 1: one full
64-row chunk and a one-row chunk; a 58-row tail; 16 full chunks and a one-row chunk) and cfg1 (n = 1937, n % 64 = 17).
None of the th_operators sizes from N = 3 to 16 has n % 64 == 0, so no case has a last chunk that is full.
gmres_restart = 10: the four-at-a-time body of every loop over basis vectors runs twice and every tail length 0 .. 3
occurs; one cfg1 case runs at the default restart (30) for the default LDS layout.  Forms by the switches a context
reads when it is created (RICADI_ARNOLDI, RICADI_W32, RICADI_FUSEH, RICADI_BASIS32, RICADI_BASIS64), widths 5 / 8 /
16 / 24 / 32 (arnoldi_model.CASES); the IterationForm in force is the one the
probe reports, printed per case and collected for ``test_every_kernel_path_was_reached`` (last in the file).

Three groups: group 1 leaves the table after step 3 and its whole state stays bitwise what it was; the cycle end runs
with k_g = (10, 4, 10), and with k_g = (7, 4, 2) where groups 2 and 0 leave after steps 1 and 6.

The largest error / bound per form and quantity, the stored-vector counts per case and the run time are printed by the
last test; DESIGN.md 3a-1 has the table measured on MI355X.
"""
import time

import numpy as np
import pytest

import arnoldi_model as am
import saddle_model as sm
from optconpy_amd import _lib

pytestmark = pytest.mark.gpu
SWITCHES = {"default": None, "cgs2": ("RICADI_ARNOLDI", "cgs2"), "w32off": ("RICADI_W32", "0"),
            "basis32": ("RICADI_BASIS32", "1"), "basis64": ("RICADI_BASIS64", "1"), "fuseh0": ("RICADI_FUSEH", "0")}
ENV = ("RICADI_ARNOLDI", "RICADI_W32", "RICADI_BASIS32", "RICADI_BASIS64", "RICADI_FUSEH")
ALPHAS = (-2.0, -30.0, -300.0)
REACHED = {}          # case name -> IterationForm bits
WORST = {}            # (form label, quantity) -> largest error / bound
STORE = {}            # case name -> StoreStats
CLOCK = {"t": 0.0}


@pytest.fixture(scope="module")
def operators(cfg1):
    ops = {"th3": sm.th_operators(3), "th4": sm.th_operators(4), "th11": sm.th_operators(11)}
    pr = cfg1[0]
    ops["cfg1"] = ((-pr.A - pr.Nc).T.tocsr(), pr.M.T.tocsr(), pr.J.tocsr())
    for k, (A, E, J) in ops.items():
        assert A.shape[0] + J.shape[0] == am.N_ROWS[k]
    return ops


def _dev(a, dtype=np.float64):
    import torch
    t = torch.from_numpy(np.array(a, dtype=dtype, order="C")).to("cuda:0")      # (a copy: the inputs are read-only)
    torch.cuda.synchronize()
    return t


class ProbeDevice:
    """The step probe behind the interface arnoldi_model.check_case drives."""

    def __init__(self, ctx, n, restart):
        self.ctx, self.n, self.restart = ctx, n, restart

    def begin(self, R, bnorm):
        import torch
        self.ng, _, self.m = R.shape
        Rd, bd = _dev(R), _dev(bnorm)          # (held until the call has returned)
        self.ctx.arnoldi_probe_begin_dev(ALPHAS[:self.ng], [1.0] * self.ng, self.m, Rd.data_ptr(), bd.data_ptr())
        rs, ng, m = self.restart, self.ng, self.m
        self.buf = torch.full((max(ng * self.n * m, ng * m * (rs + 1) * rs, ng * (4 * rs + 10) * 16),), float("nan"),
                              dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        self.shapes = dict(basis=(ng, self.n, m), w=(ng, self.n, m), w32=(ng, self.n, m), vcur=(ng, self.n, m),
                           h1=(ng, rs + 2, m), h2=(ng, rs + 2, m), hsum=(ng, rs + 2, m), H=(ng, m, rs, rs + 1),
                           cs=(ng, m, rs), sn=(ng, m, rs), g=(ng, m, rs + 1), scale=(ng, m), resid0=(ng, m),
                           resid1=(ng, m), y=(ng, rs, m), nrm2=(ng, m), ls_coef=(ng, 4 * rs + 10, 16), form=(8,))

    def form(self):
        return dict(zip(_lib.Context.PROBE_FORM, (bool(v) for v in self.read("form"))))

    def step(self, j, W, groups):
        Wd = _dev(W)
        self.ctx.arnoldi_probe_step_dev(j, Wd.data_ptr(), groups)

    def close(self, ks, Z, X):
        Xd, Zd = _dev(X), _dev(Z, np.float32)
        self.ctx.arnoldi_probe_close_dev(ks, Z.shape[0], Zd.data_ptr(), Xd.data_ptr())
        return Xd.cpu().numpy()

    def read(self, what, slot=0):
        shape = self.shapes[what]
        cnt = self.ctx.arnoldi_probe_read_dev(what, self.buf.data_ptr(), self.buf.numel(), slot)
        assert cnt == int(np.prod(shape)), (what, cnt, shape)
        return self.buf[:cnt].cpu().numpy().reshape(shape).copy()


def _context(monkeypatch, ops, case, **opts):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    if SWITCHES[case["switch"]]:
        monkeypatch.setenv(*SWITCHES[case["switch"]])
    ctx = _lib.Context(0, gmres_restart=case["restart"], gmres_tol=am.TOL, **opts)
    ctx.set_operator(*ops[case["op"]])
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    return ctx


def form_label(f):
    if f["lowsync"]:
        return "one-reduction"
    if f["fuseh"]:
        return "fused Hessenberg, FP32 panel" if f["w32"] else "fused Hessenberg, FP64 panel"
    basis = "FP16" if f["b16"] else "FP32" if f["b32"] else "FP64"
    return "separate Hessenberg, %s, %s basis" % ("w kept" if f["keepw"] else "w rewritten", basis)


@pytest.mark.parametrize("case", am.CASES, ids=[c["name"] for c in am.CASES])
def test_steps_against_the_model(operators, monkeypatch, case):
    t0 = time.perf_counter()
    n = am.N_ROWS[case["op"]]
    with _context(monkeypatch, operators, case) as ctx:
        dev = ProbeDevice(ctx, n, case["restart"])
        # the form is decided by width, groups and operator: a first begin on zero panels reports it
        dev.begin(np.zeros((case["ng"], n, case["m"])), np.zeros((case["ng"], case["m"])))
        form = dev.form()
        rep = am.run_case(dev, case, n, form)
    dt = time.perf_counter() - t0
    CLOCK["t"] += dt
    REACHED[case["name"]] = form
    STORE[case["name"]] = rep.stats
    label = form_label(form)
    for k, v in rep.items():
        WORST[(label, k)] = max(WORST.get((label, k), 0.0), v)
    print("%s: %s %s, %.2f s" % (case["name"], label, {k: int(v) for k, v in form.items()}, dt))
    print("  error / bound:", {k: float("%.3g" % v) for k, v in rep.items()})
    print("  stored vectors:", rep.stats, "; frozen column-steps:", rep.inert)
    assert rep.ok(), ({k: v for k, v in rep.items() if v > 1.0}, rep.stats)
    if case["frozen"]:
        assert rep.inert >= 3, rep.inert
    if case["op"] == "cfg1" and case["switch"] == "default" and case["m"] == 16:
        assert form["lowsync"], form


def test_invalid_arguments_are_refused(operators, monkeypatch):
    """RICADI_EINVAL (ValueError) before anything is launched: j outside 0 .. gmres_restart - 1, ng outside 1 .. 16,
    m outside the panel range, a group id outside 0 .. ng - 1, a step / close / read before begin."""
    case = am._case("th3", "default", 8, ng=2)
    n, m = am.N_ROWS["th3"], 8
    with _context(monkeypatch, operators, case) as ctx:
        R, bn, W = _dev(np.ones((2, n, m))), _dev(np.ones((2, m))), _dev(np.ones((2, n, m)))
        Z, X, out = _dev(np.ones((1, 2, n, m)), np.float32), _dev(np.zeros((2, n, m))), _dev(np.zeros(64))
        with pytest.raises(ValueError):
            ctx.arnoldi_probe_step_dev(0, W.data_ptr(), [0])            # before begin
        with pytest.raises(ValueError):
            ctx.arnoldi_probe_close_dev([0, 0], 1, Z.data_ptr(), X.data_ptr())
        with pytest.raises(ValueError):
            ctx.arnoldi_probe_read_dev("scale", out.data_ptr(), 64)
        for ng in (0, 17):
            with pytest.raises(ValueError):
                ctx.arnoldi_probe_begin_dev([-2.0] * ng, [1.0] * ng, m, R.data_ptr(), bn.data_ptr())
        for bad_m in (0, _lib.MAX_M + 1):
            with pytest.raises(ValueError):
                ctx.arnoldi_probe_begin_dev(ALPHAS[:2], [1.0, 1.0], bad_m, R.data_ptr(), bn.data_ptr())
        with pytest.raises(ValueError):
            ctx.arnoldi_probe_step_dev(0, W.data_ptr(), [0])            # (none of the refused begins counts)
        ctx.arnoldi_probe_begin_dev(ALPHAS[:2], [1.0, 1.0], m, R.data_ptr(), bn.data_ptr())
        for j in (-1, case["restart"]):
            with pytest.raises(ValueError):
                ctx.arnoldi_probe_step_dev(j, W.data_ptr(), [0, 1])
        for groups in ([-1], [2], [0, 2]):
            with pytest.raises(ValueError):
                ctx.arnoldi_probe_step_dev(0, W.data_ptr(), groups)
        with pytest.raises(ValueError):
            ctx.arnoldi_probe_close_dev([1, 0], 1, Z.data_ptr(), X.data_ptr())   # more vectors than steps run
        with pytest.raises(ValueError):
            ctx.arnoldi_probe_read_dev("basis", out.data_ptr(), 64, slot=case["restart"] + 1)
        # ... and the cycle is still intact
        ctx.arnoldi_probe_step_dev(0, W.data_ptr(), [0, 1])
        ctx.arnoldi_probe_close_dev([1, 1], 1, Z.data_ptr(), X.data_ptr())
        assert np.isfinite(X.cpu().numpy()).all()


def test_every_kernel_path_was_reached():
    """Over all cases above: the one-reduction form; the fused Hessenberg launch on an FP32 and on an FP64 panel;
    the separate Hessenberg kernel with w kept and with w rewritten; the generic kernels on an FP32 and an FP64 basis.

    The separate Hessenberg kernel with w kept is what RICADI_FUSEH=0 selects at 16 columns on the FP16 basis: the
    Hessenberg update in its own launch, which also leaves h1 + h2 for the last pass on the kept w."""
    assert REACHED, "the step cases of this module did not run in this session"
    forms = list(REACHED.values())
    paths = {
        "one-reduction form": any(f["lowsync"] for f in forms),
        "fused Hessenberg, FP32 panel": any(f["fuseh"] and f["w32"] and not f["lowsync"] for f in forms),
        "fused Hessenberg, FP64 panel": any(f["fuseh"] and not f["w32"] for f in forms),
        "separate Hessenberg kernel, w kept": any(not f["fuseh"] and f["keepw"] for f in forms),
        "separate Hessenberg kernel, w rewritten": any(not f["fuseh"] and not f["keepw"] for f in forms),
        "generic kernels, FP32 basis": any(f["b32"] for f in forms),
        "generic kernels, FP64 basis": any(not f["b16"] and not f["b32"] for f in forms),
    }
    by_op = {}
    for name, f in REACHED.items():
        by_op.setdefault(name.split("-")[0], set()).add(form_label(f))
    for op in sorted(by_op):
        print("%s: %s" % (op, sorted(by_op[op])))
    print("paths:", paths)
    print("largest error / bound per form and quantity:")
    for (label, k), v in sorted(WORST.items()):
        print("  %-45s %-28s %.3g" % (label, k, v))
    print("stored vectors per case:")
    for name, st in STORE.items():
        print("  %-40s %r" % (name, st))
    print("run time of the step cases: %.1f s" % CLOCK["t"])
    assert all(paths.values()), [k for k, v in paths.items() if not v]
