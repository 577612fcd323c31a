"""CPU tests of the complex-conjugate pair step of the Lyapunov ADI: the dense model of
tests/adi_pairs_model.py against the dense Lyapunov solutions of tests/small_ops.py, with and without a low-rank term;
the parsing of complex shift lists, the new C entries' signatures and the pair selection of ``adi_shifts``; and the
faults the GPU test of the blocks kernel (tests/test_gpu_adi_pairs.py) must be able to see.

The GPU tests mean something only while these pass: they hold the device to this model.
"""
import os
import re

import numpy as np
import pytest

import adi_pairs_model as apm
import small_ops as so
from optconpy_amd import _lib, adi_shifts
from optconpy_amd import proj_ric_utils as pru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAIN = ["fe2", "fe3", "unsym", "nv65_np24", "nv63_np0", "nv33_np1", "e_outside", "free_rows", "arrow200", "nv17_np16"]
LOWRANK = ["fe2", "fe3", "unsym", "nv65_np24", "nv33_np1", "e_outside", "free_rows"]
MODEL_TOL = 1e-12
# the shapes of the blocks-kernel test on the device (tests/test_gpu_adi_pairs.py)
KERNEL_NV = (1, 2, _lib.ADI_PAIR_ROWS - 1, _lib.ADI_PAIR_ROWS + 1, 200)
KERNEL_M = (1, 7, 8, 9, 16, 17, 24)
KERNEL_P = (-1 + 2j, -1 - 2j, -50 + 1j, -0.01 + 1j)

_MODELS = {}


def model_of(name, lowrank):
    """(operator, its PairsModel -- with ``U = -oldB``, ``V = B`` where ``lowrank`` --, the shift list of the recipe)."""
    key = (name, lowrank)
    if key not in _MODELS:
        op = so.get(name)
        mdl = apm.PairsModel(*op.ops, U=-op.oldB if lowrank else None, V=op.B if lowrank else None)
        _MODELS[key] = (op, mdl, apm.pair_shifts(mdl, op.shifts))
    return _MODELS[key]


def _run_checks(name, lowrank):
    op, mdl, ms = model_of(name, lowrank)
    assert max(mdl.pencil_eigs().real) < 0, "the operator as solved must be stable"
    out = mdl.run(ms, op.W, max_steps=300, newZ_reltol=1e-12, woodbury=lowrank)
    Z, X = out["Z"], mdl.lyap(op.W)
    print("[adi pairs] %s lowrank %d | steps %d pairs %d rule %s" % (name, lowrank, out["steps"], out["pairs"],
                                                                     out["rule"]))
    assert out["rule"] == "newZ", out["steps"]
    assert np.isrealobj(Z) and Z.shape[1] == out["steps"] * op.W.shape[1]
    err = so.rel(Z @ Z.T, X)
    print("[adi pairs] %s | Z Z^T vs dense | %.3e | %.3e" % (name, err, MODEL_TOL))
    assert err <= MODEL_TOL
    # the residual identity: the dense projected residual of Z Z^T is W W^T with the factor the iteration carries
    R = mdl.projected_residual(Z, out["W0"])
    Wh = mdl.Th.T @ out["W"]
    rhs = np.linalg.norm(mdl.Th.T @ out["W0"]) ** 2
    rid = np.linalg.norm(R - Wh @ Wh.T) / rhs
    print("[adi pairs] %s | residual identity | %.3e | %.3e" % (name, rid, MODEL_TOL))
    assert rid <= MODEL_TOL
    jz = float(np.max(np.abs(mdl.J @ Z))) if mdl.np else 0.0
    print("[adi pairs] %s | max |J Z| | %.3e | %.3e" % (name, jz, MODEL_TOL))
    assert jz <= MODEL_TOL
    return out


@pytest.mark.parametrize("name", PLAIN)
def test_pair_step_against_dense_lyapunov(name):
    """``Z Z^T`` against ``SmallOp.lyap()`` to 1e-12, the residual identity to 1e-12 relative, a real ``Z`` in ker J."""
    op, mdl, ms = model_of(name, False)
    out = _run_checks(name, False)
    assert so.rel(out["Z"] @ out["Z"].T, op.lyap()) <= MODEL_TOL
    if name == "nv17_np16":
        # ker J has one dimension: no complex eigenvalue, the recipe returns a purely real list
        assert not any(isinstance(p, complex) for p in ms) and out["pairs"] == 0
    else:
        assert isinstance(ms[0], complex) and out["pairs"] >= 1


@pytest.mark.parametrize("name", LOWRANK)
def test_pair_step_with_a_lowrank_term(name):
    """The same with ``calA + oldB B^T`` through the Woodbury form; the Woodbury solve equals the closed-loop one."""
    op, mdl, ms = model_of(name, True)
    out = _run_checks(name, True)
    assert out["steps"] <= 112 and out["pairs"] >= 1
    p = ms[0]
    a, b = mdl.solve(p, out["W0"], woodbury=True), mdl.solve(p, out["W0"], woodbury=False)
    assert so.rel(a, b) <= 1e-10


def test_a_pair_and_its_conjugate_give_the_same_factor():
    op, mdl, ms = model_of("fe3", False)
    conj = [p.conjugate() if isinstance(p, complex) else p for p in ms]
    a = mdl.run(ms, op.W, max_steps=40, newZ_reltol=0.0)
    b = mdl.run(conj, op.W, max_steps=40, newZ_reltol=0.0)
    assert a["steps"] == b["steps"] == 40
    assert so.rel(a["Z"] @ a["Z"].T, b["Z"] @ b["Z"].T) <= 1e-13


def test_a_pair_equals_its_two_complex_steps():
    """One pair step against the textbook complex ADI with ``p`` and then ``conj p``: the same ``Z Z^H`` and the same
    (real) residual factor."""
    op, mdl, ms = model_of("fe3", False)
    p = ms[0]
    out = mdl.run([p], op.W, max_steps=2)
    W0 = out["W0"].astype(complex)
    V = mdl.solve(p, W0)
    W1 = W0 - 2.0 * p.real * (mdl.E @ V)
    V2 = mdl.solve(p.conjugate(), W1)
    W2 = W1 - 2.0 * p.real * (mdl.E @ V2)
    Zc = np.sqrt(-2.0 * p.real) * np.hstack([V, V2])
    assert so.rel(out["Z"] @ out["Z"].T, Zc @ Zc.conj().T) <= 1e-12
    assert so.rel(out["W"], W2) <= 1e-12 and np.linalg.norm(W2.imag) <= 1e-12 * np.linalg.norm(W2.real)


def test_pairs_are_never_split_and_count_twice():
    op, mdl, ms = model_of("fe3", False)
    pair = ms[0]
    out = mdl.run([-1.0, pair], op.W, max_steps=5)
    assert (out["steps"], out["pairs"], out["solves"], out["rule"]) == (4, 1, 3, "max_steps")   # 1 + 2 + 1, a pair due
    out = mdl.run([-1.0, pair], op.W, max_steps=4)
    assert (out["steps"], out["solves"]) == (4, 3)
    out = mdl.run([-1.0, pair], op.W, max_steps=2)
    assert (out["steps"], out["pairs"], out["solves"]) == (1, 0, 1)
    h = mdl.run([pair, -1.0], op.W, max_steps=6)["hist"]
    assert h.size == 6 and h[0] == h[1] and h[3] == h[4] and h[1] != h[2]


# ------------------------------------------------------------------------------------------------ parsing, interface
def test_shift_list_parsing():
    assert pru._shifts(dict(ms=[-1 + 2j])) == [-1 + 2j]
    assert pru._shifts(dict(ms=[-1 + 2j, -1 - 2j, -3.0, -2 - 1j])) == [-1 + 2j, -3.0, -2 - 1j]
    ms = pru._shifts(dict(ms=[-3, -1 - 2j, -1 + 2j, -1 + 2j]))
    assert ms == [-3.0, -1 - 2j, -1 + 2j] and isinstance(ms[0], float) and isinstance(ms[1], complex)
    for bad in ([1 + 2j], [0j + 0.0, -1 + 1j], [-1 + 1j, 2.0], [complex(np.nan, 1.0)], [complex(-1.0, np.inf)]):
        with pytest.raises(ValueError, match="ADI shifts must be negative real numbers"):
            pru._shifts(dict(ms=bad))
    with pytest.raises(ValueError, match="ADI shifts must be negative real numbers"):
        pru._shifts(dict(ms=[-1.0, 2.0]))
    # a real list comes back as before: floats, nothing merged
    ms = pru._shifts(dict(ms=[-3, -3, np.float64(-1.5)]))
    assert ms == [-3.0, -3.0, -1.5] and all(type(p) is float for p in ms)
    assert pru._shifts({}) == [float(p) for p in pru.DEFAULT_MS]
    assert pru._shifts(dict(ms="auto")) == "auto" and pru._shifts(dict(ms="auto-complex")) == "auto-complex"
    # the Riccati iterations keep refusing complex entries
    for d in (dict(ms=[-1 + 2j]), dict(ms="auto-complex")):
        with pytest.raises(ValueError, match="ADI shifts must be negative real numbers"):
            pru._real_shifts(d)
    assert pru._real_shifts(dict(ms=[-2, -1])) == [-2.0, -1.0] and pru._real_shifts(dict(ms="auto")) == "auto"


def test_signatures_of_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "ricadi.h")).read()
    want = {"ricadi_lyap_adi_cplx": 10, "ricadi_adi_pair_blocks_dev": 12, "ricadi_adi_pair_info": 2}
    for name, nargs in want.items():
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl is not None, name + " is not declared in include/ricadi.h"
        assert len(decl.group(1).split(",")) == nargs
    # ricadi_adi_params is pinned: the new entry takes it as ricadi_lyap_adi does
    assert _lib.SIGNATURES["ricadi_lyap_adi_cplx"][1][6:] == _lib.SIGNATURES["ricadi_lyap_adi"][1][5:]
    assert _lib.adi_pair_groups(3) == (1, 3) and _lib.adi_pair_groups(9) == (2, 5) and _lib.adi_pair_groups(17) == (3, 6)
    assert _lib.adi_pair_groups(128) == (16, 8) and apm.groups(24) == _lib.adi_pair_groups(24) == (3, 8)


def test_penzl_select_picks_the_dominant_pair_and_counts_it_twice():
    cands = np.array([-1 + 10j, -1 - 10j, -1.0 + 0j])
    assert adi_shifts.penzl_select(cands, 2) == [-1 + 10j]                  # the pair alone fills num = 2
    picks = adi_shifts.penzl_select(cands, 3)
    assert picks == [-1 + 10j, -1.0] and isinstance(picks[1], float)
    assert adi_shifts.penzl_select(cands, 1) == [-1.0]                      # no room for a pair
    # the pair factor: a pair annihilates both of its members
    t = np.array([-1 + 10j, -1 - 10j, -3.0])
    r = adi_shifts._pair_ratio(t, complex(-1, 10))
    assert r[0] == 0.0 and r[1] == 0.0
    assert np.isclose(r[2], abs((-3 - (-1 + 10j)) * (-3 - (-1 - 10j)) / ((-3 + (-1 + 10j)) * (-3 + (-1 - 10j)))))
    # real candidates take the path they always took
    real = [-1.0, -2.0, -0.5, -40.0]
    assert adi_shifts.penzl_select(np.array(real) + 0j, 3) == adi_shifts.penzl_select(real, 3)


def test_candidates_keep_complex():
    rng = np.random.default_rng(3)
    lam = np.array([-1 + 3j, -1 - 3j, -2.0, -5 + 1e-5j, -5 - 1e-5j, 0.5 + 1j, 0.5 - 1j])
    T = rng.standard_normal((7, 7))
    # a real matrix with these eigenvalues: 2 x 2 rotation blocks
    D = np.zeros((7, 7))
    D[0:2, 0:2] = [[-1, 3], [-3, -1]]
    D[2, 2] = -2
    D[3:5, 3:5] = [[-5, 1e-5], [-1e-5, -5]]
    D[5:7, 5:7] = [[0.5, 1], [-1, 0.5]]
    HA = T @ D @ np.linalg.inv(T)
    old = np.sort(adi_shifts.candidates(HA, np.eye(7)))
    assert np.allclose(old, np.sort(-np.abs(lam)), rtol=1e-8)
    c = adi_shifts.candidates(HA, np.eye(7), keep_complex=True)
    assert np.iscomplexobj(c) and c.size == 7
    off = c[c.imag != 0]
    assert off.size == 2 and np.allclose(off, -1 + 3j, rtol=1e-8)          # both members map to Im > 0
    assert np.allclose(np.sort(c[c.imag == 0].real), np.sort([-2.0, -5.0, -5.0, -abs(0.5 + 1j), -abs(0.5 + 1j)]),
                       rtol=1e-8)


# ------------------------------------------------------------------------------------------------ the kernel's twin
def _kernel_case(nv, m, p, seed=0):
    rng = np.random.default_rng(1000 * nv + 10 * m + seed)
    ng, mc = apm.groups(m)
    X = rng.standard_normal((ng, nv, mc)) + 1j * rng.standard_normal((ng, nv, mc))
    return X


@pytest.mark.parametrize("fault", ["delta_sign", "no_sqrt", "last_row"])
def test_injected_faults_break_the_entrywise_bound(fault):
    """At every shape and shift of the device test the fault moves an entry of the twin beyond the bound the device is
    held to (a NaN counts: the comparison is ``not (diff <= bound)``)."""
    for nv in KERNEL_NV:
        for m in KERNEL_M:
            for p in KERNEL_P:
                X = _kernel_case(nv, m, p)
                Z1, Z2, V1, n2 = apm.blocks_twin(X, nv, m, p)
                F1, F2, FV, fn2 = apm.blocks_twin(X, nv, m, p, fault=fault)
                bz, bv = apm.blocks_bound(X, nv, m, p)
                ok = (np.all(np.abs(F1 - Z1) <= bz) and np.all(np.abs(F2 - Z2) <= bz)
                      and np.all(np.abs(FV - V1) <= bv))
                assert not ok, (fault, nv, m, p)


def test_twin_matches_the_model_step():
    """The twin on the packed dense solution reproduces the two blocks of ``PairsModel.run``."""
    op, mdl, ms = model_of("fe3", False)
    p = ms[0]
    out = mdl.run([p], op.W, max_steps=2)
    m = op.W.shape[1]
    X = apm.pack(mdl.solve(p, out["W0"]))
    assert np.array_equal(apm.unpack(apm.pack(op.W), m), op.W)
    Z1, Z2, V1, n2 = apm.blocks_twin(X, mdl.nv, m, p)
    assert np.array_equal(np.hstack([Z1, Z2]), out["Z"])
    assert np.allclose(n2, [np.sum(Z1 ** 2), np.sum(Z2 ** 2)], rtol=1e-15)
