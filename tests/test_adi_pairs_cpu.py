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


# ------------------------------------------------------------------------------------------------ the Woodbury solve
# what tests/test_gpu_adi_pair_solve.py rests on
LADDER_OPS = ("unsym", "nv33_np1", "nv65_np24", "fe3")
LADDER_DELTAS = (1e-1, 1e-2, 1e-3)
LADDER_TOL, LADDER_ETA, LADDER_Q, LADDER_M = 1e-8, 1e-3, 3, (3, 9)
FIRST_BLOCK_TOL = 0.266


def ladder_of(name):
    """(operator, p, [(delta, U2, V)]) of the refinement ladder on ``name``: ``a = -sqrt(min max |lambda|)`` of the
    operator's projected pencil."""
    op, mdl, _ = model_of(name, False)
    lam = np.abs(mdl.pencil_eigs())
    lam = lam[np.isfinite(lam)]
    a = -float(np.sqrt(lam.min() * lam.max()))
    p, rungs = apm.refinement_ladder(op, a, LADDER_ETA, LADDER_DELTAS, LADDER_Q, seed=130)
    return op, p, rungs


def ladder_rhs(op, m):
    return np.random.default_rng(200 + m).standard_normal((op.nv, m))


def first_block_list(name="fe3"):
    op, mdl, ms = model_of(name, False)
    return op, mdl, [complex(ms[0].real, 20.0 * ms[0].imag)]


def steps_pinned(ref, tol):
    """Whether the model's stopping step is safe from rounding: of the entry that stopped the run (both blocks of a
    pair) the smallest ``rel_newZ`` lies a factor 2 below ``tol``, and the entry before it a factor 2 above."""
    r = ref["rel_newZ"]
    if ref["rule"] != "newZ":
        return False
    k = 2 if (len(r) >= 2 and ref["last_is_pair"]) else 1
    return bool(r[-k:].min() <= tol / 2 and (len(r) == k or r[-k - 1] >= 2 * tol))


def _random_groups(m, q, nv, n, seed):
    rng = np.random.default_rng(seed)
    ng, mc = apm.groups(m + q)
    X = rng.standard_normal((ng, n, mc)) + 1j * rng.standard_normal((ng, n, mc))
    for j in range(m + q, ng * mc):
        X[j // mc, :, j % mc] = 0.0
    V = 0.2 * rng.standard_normal((nv, q))
    return X, V


@pytest.fixture(scope="module")
def smw_probe(tmp_path_factory):
    import test_pair_smw_cpu as tps
    return tps._build(tmp_path_factory.mktemp("pair_smw_twin"), [])


@pytest.mark.parametrize("m,q", [s for s in apm.PAIR_SOLVE_SHAPES if s[1] > 0])
def test_woodbury_bound_holds_a_second_evaluation_and_sees_the_faults(smw_probe, m, q):
    """A second float64 evaluation of the twin -- rows in reversed order, the header's LU and embedding through the
    probe -- stays at or below 0.5 of ``woodbury_bound``; every seeded fault that applies at the shape exceeds 1."""
    nv, n = 37, 45
    X, V = _random_groups(m, q, nv, n, 10 * m + q)
    ng, mc = apm.groups(m + q)
    ref = apm.woodbury_twin(X, V, m, q)
    bound = apm.woodbury_bound(X, V, m, q)
    at = apm._maps(m, q)
    wcols = np.zeros((ng, n, mc), dtype=bool)
    for g, cc in at[:m]:
        wcols[g, :, cc] = True
    assert np.all(bound[wcols] > 0) and np.all(bound[~wcols] == 0)
    assert np.array_equal(ref[~wcols], X[~wcols])
    # second evaluation: V^T X with the rows reversed, then the header
    T = np.einsum("vk,gvc->gkc", V[::-1], X[:, :nv][:, ::-1])
    ht = np.zeros((ng, q, 2 * mc))
    ht[:, :, 0::2], ht[:, :, 1::2] = T.real, T.imag
    cap, ok, low, y, hm = smw_probe.smw(m, q, ht)
    assert ok
    XU = np.stack([X[g, :, cc] for g, cc in at[m:]], axis=1)
    xr = np.ascontiguousarray(XU).view(np.float64)
    second = X.copy()
    for g in range(ng):
        second[g] += np.ascontiguousarray(xr[::-1] @ hm[g]).view(np.complex128)[::-1]
    ratio = float(np.max(np.abs(second - ref)[wcols] / bound[wcols]))
    print("[pair solve] model m %d q %d | second evaluation / bound | %.3e | 0.5" % (m, q, ratio))
    assert ratio <= 0.5 and np.array_equal(second[~wcols], X[~wcols])
    for fault in apm.WOODBURY_FAULTS:
        if not apm.fault_applies(fault, m, q, n, nv):
            continue
        bad = apm.woodbury_twin(X, V, m, q, fault=fault)
        d = np.abs(bad - ref)
        worst = float(np.max(np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d > 0, np.inf, 0.0))))
        print("[pair solve] model m %d q %d | fault %s / bound | %.3e | > 1" % (m, q, fault, worst))
        assert worst > 1.0, (fault, m, q)
    # the two-pass twin: a second evaluation holds, the uncorrected D does not
    D = 1e-6 * _random_groups(m, q, nv, n, 77)[0]
    for g, cc in at[m:]:
        D[g, :, cc] = 0.0
    ref2, bound2 = apm.woodbury_twin(X, V, m, q, Draw=D), apm.woodbury_bound(X, V, m, q, Draw=D)
    rev = apm.woodbury_twin(X[:, ::-1][:, list(range(n - nv, n)) + list(range(n - nv))], V[::-1], m, q,
                            Draw=D[:, ::-1][:, list(range(n - nv, n)) + list(range(n - nv))])
    back = rev[:, list(range(nv, n)) + list(range(nv))][:, ::-1]
    assert float(np.max(np.abs(back - ref2)[wcols] / bound2[wcols])) <= 0.5
    bad = apm.woodbury_twin(X, V, m, q, fault="refine_raw", Draw=D)
    assert float(np.max(np.abs(bad - ref2)[wcols] / bound2[wcols])) > 1.0
    which = [s for s in apm.PAIR_SOLVE_SHAPES if apm.fault_applies("straddle", *s)]
    assert which == [(5, 6), (2, 16)]
    which = [s for s in apm.PAIR_SOLVE_SHAPES if apm.fault_applies("group_of_m", *s)]
    assert which == [(5, 6), (2, 16), (17, 7)]


@pytest.mark.parametrize("name", LOWRANK)
def test_no_refinement_is_due_on_the_lowrank_operators(name):
    """The model's amplification stays at or below 8 along the whole run on every LOWRANK operator (9 is where a
    column could reach 10 tol): the driver test asserts ``pair_info[2] == 0`` on all of them, none is exempt."""
    op, mdl, ms = model_of(name, True)
    out = mdl.run(ms, op.W, max_steps=300, newZ_reltol=1e-12, woodbury=True)
    a = out["amplification"]
    print("[adi pairs] %s | amplification: first %.2f, largest %.2f at pair %d of %d" %
          (name, a[0], a.max(), int(a.argmax()), a.size))
    assert a.size == out["pairs"] and a.max() <= 8.0


@pytest.mark.parametrize("name", LADDER_OPS)
def test_the_ladder_makes_the_refinement_due(name):
    """At delta = 1e-3 the model's amplification is at least 100 on every column (the solves' residuals, at most tol,
    then exceed 10 tol unless they are a factor 10 better than asked) and the closed-loop reference is good to
    tol / 100; the imaginary part of the capacitance matrix stays below its delta real part."""
    op, p, rungs = ladder_of(name)
    assert p.real < 0 < p.imag and abs(p.imag / p.real + LADDER_ETA) < 1e-15
    for delta, U2, V in rungs:
        mdl = apm.PairsModel(*op.ops, U=U2, V=V)
        for m in LADDER_M:
            W = ladder_rhs(op, m)
            amp = apm.amplification(mdl, p, W)
            S = mdl.saddle(mdl.A, p)
            x = mdl._solve(S, W)
            rhs = np.zeros_like(x)
            rhs[:op.nv] = W
            rr = float(np.max(np.linalg.norm(S @ x - rhs, axis=0) / np.linalg.norm(W, axis=0)))
            XU = mdl._solve(mdl.saddle(mdl.A0, p), U2)[:op.nv]
            cap = np.eye(LADDER_Q) - V.T @ XU
            smin = float(np.linalg.svd(cap, compute_uv=False)[-1])
            print("[pair solve] ladder %s delta %g m %d | min amplification %.3g | reference residual %.2e | "
                  "sigma_min(cap) %.2e | max |Im cap| %.2e" % (name, delta, m, amp.min(), rr, smin,
                                                               np.abs(cap.imag).max()))
            assert rr <= LADDER_TOL / 100
            assert np.allclose(cap.real, delta * np.eye(LADDER_Q), atol=1e-9) and smin >= delta / 2
            if delta == 1e-3:
                assert amp.min() >= 100.0


def test_a_rule_that_fires_on_the_first_block_only_model():
    """fe3 with the first recipe pair's imaginary part times 20 and ``adi_newZ_reltol = 0.266``: the model's relative
    block norms are 1.0, 0.99 and 0.101, 0.701 -- the rule fires on the second pair's first block alone, a factor 2.6
    from the tolerance on either side --, and both blocks are kept."""
    op, mdl, lst = first_block_list()
    out = mdl.run(lst, op.W, max_steps=300, newZ_reltol=FIRST_BLOCK_TOL)
    r = out["rel_newZ"]
    print("[adi pairs] fe3 | first-block rule | rel_newZ %s" % r)
    assert (out["steps"], out["pairs"], out["rule"]) == (4, 2, "newZ") and out["Z"].shape[1] == 4 * op.W.shape[1]
    assert np.allclose(r, [1.0, 0.99, 0.101, 0.701], rtol=0.05)
    assert r[2] < FIRST_BLOCK_TOL / 2 and r[3] > 2 * FIRST_BLOCK_TOL


def test_signature_of_the_pair_solve_entry():
    hdr = open(os.path.join(ROOT, "include", "ricadi.h")).read()
    res, args = _lib.SIGNATURES["ricadi_adi_pair_solve_dev"]
    decl = re.search(r"\bint\s+ricadi_adi_pair_solve_dev\s*\(([^;]*)\)\s*;", hdr)
    assert decl is not None and len(decl.group(1).split(",")) == len(args) == 10
    assert len(_lib.Context.PAIR_SOLVE_REPORT) == 8
