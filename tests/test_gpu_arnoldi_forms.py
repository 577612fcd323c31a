"""GPU tests of every kernel form of the three-pass Arnoldi (dots, update + dots, update [+ Hessenberg]) and of the
one-reduction form beside it, by panel width and storage form.  Each case solves two shifted cfg1 systems through the
C-ABI with gmres_restart = 6, so every case crosses several cycle ends and the number of basis vectors runs through
1 .. 7: the odd tail and the four-at-a-time (two-at-a-time) body of every loop over vectors.  The sparse LU is the
reference and the FP64 true residual the judge.

Widths: 5 takes the generic kernels, 8 / 16 / 24 / 32 the FP16 kernels with 1 / 2 / 3 / 4 column octets (16: the hot
width).  Storage forms (switches read when a context is created): the default, RICADI_ARNOLDI=cgs2 (three passes on
the hot path), RICADI_W32=0 (FP64 panel w), RICADI_BASIS32=1 and RICADI_BASIS64=1 (generic kernels on an FP32 / FP64
basis; FP64 also reaches the separate Hessenberg kernel and the unfused update).

cfg1 has n = 1937 rows, n % 64 = 17: the last 64-row chunk of every dot kernel is a partial one (17 rows), so the
row-tail branches (nr < DOT_ROWS) are exercised in every case.
"""
import numpy as np
import pytest

from optconpy_amd import _lib
from oracle import lin_alg_utils as olau

pytestmark = pytest.mark.gpu
SHIFTS = [-2.0, -300.0]
WIDTHS = (5, 8, 16, 24, 32)
SWITCHES = ("RICADI_ARNOLDI", "RICADI_W32", "RICADI_BASIS32", "RICADI_BASIS64")
FORMS = {
    "default": None,
    "cgs2": ("RICADI_ARNOLDI", "cgs2"),
    "w32off": ("RICADI_W32", "0"),
    "basis32": ("RICADI_BASIS32", "1"),
    "basis64": ("RICADI_BASIS64", "1"),
}


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def system(cfg1):
    """The cfg1 operator, its sparse LU per shift (factored once) and a cache of reference solutions per panel."""
    pr = cfg1[0]
    calA = (-pr.A - pr.Nc).T.tocsr()
    MT = pr.M.T.tocsr()
    lus = [olau.SaddleLU(calA + p * MT, pr.J) for p in SHIFTS]
    return {"pr": pr, "calA": calA, "MT": MT, "lus": lus, "refs": {}}


def _rhs(system, m, zero_col=None):
    rng = np.random.default_rng(100 + m)
    R = rng.standard_normal((system["pr"].NV, m))
    if zero_col is not None:
        R[:, zero_col] = 0.0
    return R


def _reference(system, key, R):
    if key not in system["refs"]:
        refs = [lu.solve(R) for lu in system["lus"]]
        for r in refs:
            r.setflags(write=False)
        system["refs"][key] = refs
    return system["refs"][key]


def _solve(system, monkeypatch, form, R):
    import torch
    pr = system["pr"]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if FORMS[form]:
        monkeypatch.setenv(*FORMS[form])
    m = R.shape[1]
    with _lib.Context(0, gmres_restart=6) as ctx:
        ctx.set_operator(system["calA"], system["MT"], pr.J)
        Rd = torch.from_numpy(np.ascontiguousarray(R)).cuda()
        Xd = torch.empty((len(SHIFTS), pr.NV + pr.NP, m), dtype=torch.float64, device="cuda")
        its, rr = ctx.shift_solve_batch_dev(SHIFTS, [1.0] * len(SHIFTS), Rd.data_ptr(), 0, m, Xd.data_ptr())
        ctx.synchronize()
        X = Xd.cpu().numpy()
        w32 = ctx.setup_info()["fp32_operator_output"]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return np.asarray(its), np.asarray(rr), X, w32


def _check(system, form, R, refs, out):
    its, rr, X, w32 = out
    NV = system["pr"].NV
    print("%s m=%d: iterations %s, max relative residual %.3e" % (form, R.shape[1], its.tolist(), rr.max()))
    for g in range(len(SHIFTS)):
        print("  shift %g: velocity part vs sparse LU %.3e" % (SHIFTS[g], rel(X[g][:NV], refs[g][:NV])))
    assert rr.max() <= 1e-10, (form, rr.max())
    for g in range(len(SHIFTS)):
        assert rel(X[g][:NV], refs[g][:NV]) < 1e-8, (form, g)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m", WIDTHS)
def test_width_and_storage_form(system, monkeypatch, m, form):
    """Every column meets the tolerance in the true residual, the velocity part matches the sparse LU; at the hot
    width the FP32 operator output is in use exactly where the form admits it."""
    R = _rhs(system, m)
    out = _solve(system, monkeypatch, form, R)
    _check(system, form, R, _reference(system, m, R), out)
    if m == 16 and form in ("default", "cgs2", "w32off"):
        assert out[3] == (0 if form == "w32off" else 1), (form, out[3])


def test_zero_column_stays_inert_at_24_columns(system, monkeypatch):
    """A zero right-hand side column is frozen from the first iteration (the frozen-column rule through the shared
    Givens tail, off the hot width, FP64 panel): its solution stays exactly zero."""
    R = _rhs(system, 24, zero_col=11)
    out = _solve(system, monkeypatch, "w32off", R)
    _check(system, "w32off", R, _reference(system, (24, "zero"), R), out)
    assert np.abs(out[2][:, :, 11]).max() == 0.0
