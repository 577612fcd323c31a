"""The host arithmetic of the pair step's complex solve (``optconpy_amd/csrc/pair_smw.h``: the LU of the capacitance
matrix, the grouping of the ``m + q`` columns, the index map, the capacitance assembly and the real embedding of the
Woodbury coefficients) against NumPy.  A stand-alone probe that includes nothing but that header is compiled with
``g++`` and fed over stdin, as ``tests/test_adi_stop_cpu.py`` does for ``adi_stop.h``; the same probe is built once more
with ``-fsanitize=address,undefined`` and run as the program it is.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import adi_pairs_model as apm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
# (m, q) of the device test (tests/test_gpu_adi_pair_solve.py)
SHAPES = apm.PAIR_SOLVE_SHAPES

PROBE = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "pair_smw.h"
using ricadi::cdbl;
static bool rd(double& x) { return scanf("%la", &x) == 1; }
static bool rdc(cdbl& z) { double a, b; if (!rd(a) || !rd(b)) return false; z = cdbl(a, b); return true; }
static void pr(const cdbl& z) { printf("%a %a\n", z.real(), z.imag()); }
// stdin, by mode:
//   lu q w, a (q x q complex), y (q x w complex)   -> ok min_pivot_rel, piv[q], then (ok only) a^-1 y
//   map m q                                        -> ng mc, (group, column) of the m + q step columns, per group
//                                                     the columns of W and the range of U
//   embed m q, y (q x m complex)                   -> hm (ng x 2q x 2mc)
//   smw m q, ht (ng x q x 2mc real)                -> cap (q x q), ok min_pivot_rel, y = cap^-1 (V^T X_W), hm
//   coefs a b                                      -> delta gam gam2
int main() {
  char mode[16];
  if (scanf("%15s", mode) != 1) return 2;
  if (!strcmp(mode, "coefs")) {
    double a, b;
    if (!rd(a) || !rd(b)) return 2;
    const ricadi::PairCoefs pc(a, b);
    printf("%a %a %a\n", pc.delta, pc.gam, pc.gam2);
    return 0;
  }
  if (!strcmp(mode, "lu")) {
    int q, w;
    if (scanf("%d %d", &q, &w) != 2) return 2;
    std::vector<cdbl> a((size_t)q * q), y((size_t)q * w);
    for (cdbl& z : a) if (!rdc(z)) return 2;
    for (cdbl& z : y) if (!rdc(z)) return 2;
    std::vector<int> piv;
    double low = -1.0;
    const bool ok = ricadi::pair_lu(a, piv, q, &low);
    printf("%d %a\n", (int)ok, low);
    for (int k = 0; k < q; ++k) printf("%d\n", piv[k]);
    if (ok) {
      ricadi::pair_lu_solve(a, piv, q, y, w);
      for (const cdbl& z : y) pr(z);
    }
    return 0;
  }
  int m, q;
  if (scanf("%d %d", &m, &q) != 2) return 2;
  const ricadi::PairGroups pg(m + q);
  if (!strcmp(mode, "map")) {
    printf("%d %d\n", pg.ng, pg.mc);
    for (int j = 0; j < m + q; ++j) printf("%d %d\n", pg.group_of(j), pg.col_of(j));
    for (int g = 0; g < pg.ng; ++g) {
      const auto r = pg.u_range(g, m, m + q);
      printf("%d %d %d\n", pg.w_cols(g, m), r.first, r.second);
    }
    return 0;
  }
  if (!strcmp(mode, "embed")) {
    std::vector<cdbl> y((size_t)q * m);
    for (cdbl& z : y) if (!rdc(z)) return 2;
    std::vector<double> hm;
    ricadi::pair_embed(y, pg, m, q, hm);
    if (hm.size() != (size_t)pg.ng * 2 * q * pg.m2()) return 3;
    for (double v : hm) printf("%a\n", v);
    return 0;
  }
  if (!strcmp(mode, "smw")) {
    std::vector<double> ht((size_t)pg.ng * q * pg.m2());
    for (double& v : ht) if (!rd(v)) return 2;
    std::vector<cdbl> cap, y;
    ricadi::pair_capacitance(ht.data(), pg, m, q, cap);
    for (const cdbl& z : cap) pr(z);
    std::vector<int> piv;
    double low = -1.0;
    const bool ok = ricadi::pair_lu(cap, piv, q, &low);
    printf("%d %a\n", (int)ok, low);
    if (!ok) return 0;
    ricadi::pair_vtw(ht.data(), pg, m, q, y);
    ricadi::pair_lu_solve(cap, piv, q, y, m);
    for (const cdbl& z : y) pr(z);
    std::vector<double> hm;
    ricadi::pair_embed(y, pg, m, q, hm);
    for (double v : hm) printf("%a\n", v);
    return 0;
  }
  return 2;
}
"""


def _hex(a):
    return [float(x).hex() for x in np.asarray(a, dtype=float).ravel()]


def _cplx_words(a):
    a = np.ascontiguousarray(a, dtype=complex)
    return _hex(a.view(np.float64))


class Probe:
    def __init__(self, exe):
        self.exe = str(exe)

    def raw(self, words):
        r = subprocess.run([self.exe], input=" ".join(str(w) for w in words), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
        return r.stdout

    def _vals(self, words):
        return [l.split() for l in self.raw(words).splitlines()]

    def lu(self, A, Y):
        """-> (ok, min_pivot_rel, piv, A^-1 Y or None)"""
        q, w = A.shape[0], Y.shape[1]
        L = self._vals(["lu", q, w] + _cplx_words(A) + _cplx_words(Y))
        ok, low = bool(int(L[0][0])), float.fromhex(L[0][1])
        piv = [int(l[0]) for l in L[1:1 + q]]
        if not ok:
            assert len(L) == 1 + q
            return ok, low, piv, None
        y = np.array([complex(float.fromhex(l[0]), float.fromhex(l[1])) for l in L[1 + q:]]).reshape(q, w)
        return ok, low, piv, y

    def map(self, m, q):
        """-> (ng, mc, [(group, column)] of the m + q step columns, [(w_cols, u0, u1)] per group)"""
        L = self._vals(["map", m, q])
        ng, mc = int(L[0][0]), int(L[0][1])
        cols = [(int(l[0]), int(l[1])) for l in L[1:1 + m + q]]
        per = [tuple(int(x) for x in l) for l in L[1 + m + q:]]
        assert len(per) == ng
        return ng, mc, cols, per

    def embed(self, m, q, y):
        ng, mc = apm.groups(m + q)
        L = self._vals(["embed", m, q] + _cplx_words(y))
        return np.array([float.fromhex(l[0]) for l in L]).reshape(ng, 2 * q, 2 * mc)

    def smw(self, m, q, ht):
        """-> (cap, ok, min_pivot_rel, y, hm) from the ``V^T X`` products of the groups (ng, q, 2 mc)"""
        ng, mc = apm.groups(m + q)
        assert ht.shape == (ng, q, 2 * mc)
        L = self._vals(["smw", m, q] + _hex(ht))
        c = lambda rows: np.array([complex(float.fromhex(l[0]), float.fromhex(l[1])) for l in rows])
        cap = c(L[:q * q]).reshape(q, q)
        ok, low = bool(int(L[q * q][0])), float.fromhex(L[q * q][1])
        if not ok:
            return cap, ok, low, None, None
        at = q * q + 1
        y = c(L[at:at + q * m]).reshape(q, m)
        hm = np.array([float.fromhex(l[0]) for l in L[at + q * m:]]).reshape(ng, 2 * q, 2 * mc)
        return cap, ok, low, y, hm


def _build(d, flags):
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + flags +
                          ["-I", os.path.join(ROOT, "optconpy_amd", "csrc"), str(src), "-o", str(exe)])
    return Probe(exe)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pair_smw"), [])


@pytest.fixture(scope="module")
def probe_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pair_smw_san"),
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def test_the_header_has_no_hip_include():
    src = open(os.path.join(ROOT, "optconpy_amd", "csrc", "pair_smw.h")).read()
    incs = [l.split()[1] for l in src.splitlines() if l.startswith("#include")]
    assert incs and all(i.startswith("<") and "hip" not in i for i in incs), incs
    inl = open(os.path.join(ROOT, "optconpy_amd", "csrc", "solver_adi_pairs.inl")).read()
    assert '#include "pair_smw.h"' in inl and "bool pair_lu(" not in inl and "struct PairCoefs" not in inl


# ------------------------------------------------------------------------------------------------ LU and solve
LU_Q = (1, 2, 3, 7, 16)
LU_W = (1, 5, 24)


def _lu_matrices(q):
    """(tag, matrix): random, one with a zero leading entry, one that needs an exchange at every column (q > 1)."""
    rng = np.random.default_rng(100 + q)
    rnd = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    out = [("random", rnd(q, q))]
    if q > 1:
        A = rnd(q, q)
        A[0, 0] = 0.0
        out.append(("zero leading entry", A))
        # lower Hessenberg-like: a cyclic shift of a dominant diagonal puts the largest entry of column k in row k + 1
        # of the reduced matrix at every column, so every column but the last exchanges rows
        A = 0.05 * rnd(q, q)
        for k in range(q):
            A[(k + 1) % q, k] += 4.0 + k
        out.append(("exchange at every column", A))
    return out


@pytest.mark.parametrize("q", LU_Q)
def test_lu_and_solve_against_numpy(probe, q):
    """``pair_lu`` + ``pair_lu_solve`` against ``numpy.linalg.solve``: every column within ``8 q eps cond_2(A)`` of the
    reference, relative to the column's norm (normwise forward error of GEPP with the growth these matrices have)."""
    for tag, A in _lu_matrices(q):
        cond = np.linalg.cond(A)
        for w in LU_W:
            Y = np.random.default_rng(7 * q + w).standard_normal((q, w)) * (1 + 0.5j)
            ok, low, piv, X = probe.lu(A, Y)
            assert ok and 0.0 < low <= 1.0
            if tag == "exchange at every column":
                assert all(piv[k] != k for k in range(q - 1)), piv
            if tag == "zero leading entry":
                assert piv[0] != 0
            ref = np.linalg.solve(A, Y)
            err = float(np.max(np.linalg.norm(X - ref, axis=0) / np.linalg.norm(ref, axis=0)))
            bound = 8 * q * EPS * cond
            print("[pair smw] lu q %d w %d %s | error | %.3e | %.3e" % (q, w, tag, err, bound))
            assert err <= bound


def test_singular_return(probe):
    """Exactly singular, zero, and a pivot of 1e-14 max |a| are refused; a pivot of 1e-12 max |a| is accepted."""
    Y = np.ones((3, 1), dtype=complex)
    A = np.array([[1, 2, 3], [2, 4, 6], [1, 0, 1]], dtype=complex)          # row 1 = 2 row 0, exactly in binary
    ok, low, piv, X = probe.lu(A, Y)
    assert not ok and X is None and low == 0.0
    ok, low, piv, X = probe.lu(np.zeros((3, 3), dtype=complex), Y)
    assert not ok and low == 0.0
    ok, low, piv, X = probe.lu(np.zeros((1, 1), dtype=complex), Y[:1])
    assert not ok
    for piv_rel, want in ((1e-14, False), (1e-12, True)):
        # upper triangular with a dominant first row: no exchange, the pivots are the diagonal
        A = np.array([[4.0, 1.0, 1.0], [0.0, 1.0, 0.5], [0.0, 0.0, 4.0 * piv_rel]], dtype=complex) * (1 + 1j)
        ok, low, piv, X = probe.lu(A, Y)
        assert ok is want, piv_rel
        assert abs(low - piv_rel) <= 1e-3 * piv_rel
        if want:
            assert np.allclose(A @ X, Y, rtol=1e-3)


# ------------------------------------------------------------------------------------------------ grouping, index map
@pytest.mark.parametrize("m,q", SHAPES)
def test_grouping_and_index_map(probe, m, q):
    ng, mc, cols, per = probe.map(m, q)
    assert (ng, mc) == apm.groups(m + q) and ng * mc >= m + q and mc <= 8 and ng <= 16
    assert cols == [(j // mc, j % mc) for j in range(m + q)]
    assert len(set(cols)) == m + q and all(g < ng and c < mc for g, c in cols)
    ucols = []
    for g, (wc, u0, u1) in enumerate(per):
        assert wc == sum(1 for j in range(m) if j // mc == g)
        ucols += list(range(u0, u1))
        assert all(j // mc == g for j in range(u0, u1))
    assert ucols == list(range(m, m + q))


@pytest.mark.parametrize("m,q", [s for s in SHAPES if s[1] > 0])
def test_embedding_and_index_map(probe, m, q):
    """The real view of ``X_U`` times every group's embedded matrix, scattered through the map, is ``X_U y`` within
    ``(2q + 2) eps |X_U||y|`` entrywise; columns at or beyond ``m`` of every group are exact zeros."""
    rng = np.random.default_rng(1000 * m + q)
    n = 23
    XU = rng.standard_normal((n, q)) + 1j * rng.standard_normal((n, q))
    y = rng.standard_normal((q, m)) + 1j * rng.standard_normal((q, m))
    hm = probe.embed(m, q, y)
    ng, mc, cols, per = probe.map(m, q)
    xr = np.ascontiguousarray(XU).view(np.float64)                 # n x 2q
    got = np.zeros((n, m), dtype=complex)
    seen = np.zeros((ng, mc), dtype=bool)
    for g in range(ng):
        G = np.ascontiguousarray(xr @ hm[g]).view(np.complex128)     # n x mc
        for j in range(m):
            if cols[j][0] == g:
                got[:, j] = G[:, cols[j][1]]
                seen[g, cols[j][1]] = True
        for cc in range(mc):
            if not seen[g, cc]:
                assert np.all(hm[g][:, 2 * cc:2 * cc + 2] == 0.0) and np.all(G[:, cc] == 0.0)
    ref = XU @ y
    bound = (2 * q + 2) * EPS * ((np.abs(XU.real) + np.abs(XU.imag)) @ (np.abs(y.real) + np.abs(y.imag)))
    worst = float(np.max(np.abs(got - ref) / bound))
    print("[pair smw] embed m %d q %d | error / bound | %.3e | 1" % (m, q, worst))
    assert worst <= 1.0
    # the sign: the other embedding is far outside
    bad = (XU.real @ y.real + XU.imag @ y.imag) + 1j * (XU.real @ y.imag + XU.imag @ y.real)
    assert np.max(np.abs(bad - ref) / bound) > 1e6


@pytest.mark.parametrize("m,q", [s for s in SHAPES if s[1] > 0])
def test_capacitance_assembly(probe, m, q):
    """``cap = I - (V^T X)[:, m .. m + q)`` and ``y = cap^-1 (V^T X)[:, 0 .. m)`` from the groups' host array."""
    rng = np.random.default_rng(17 * m + q)
    ng, mc = apm.groups(m + q)
    T = 0.3 * (rng.standard_normal((q, ng * mc)) + 1j * rng.standard_normal((q, ng * mc)))
    ht = np.zeros((ng, q, 2 * mc))
    for j in range(ng * mc):
        ht[j // mc, :, 2 * (j % mc)] = T[:, j].real
        ht[j // mc, :, 2 * (j % mc) + 1] = T[:, j].imag
    cap, ok, low, y, hm = probe.smw(m, q, ht)
    want = np.eye(q) - T[:, m:m + q]
    assert ok and np.array_equal(cap, want)
    ref = np.linalg.solve(want, T[:, :m])
    err = float(np.max(np.linalg.norm(y - ref, axis=0) / np.linalg.norm(ref, axis=0)))
    assert err <= 8 * q * EPS * np.linalg.cond(want)
    assert np.array_equal(hm, probe.embed(m, q, y))


def test_pair_coefs(probe):
    for p in (-1 + 2j, -1 - 2j, -50 + 1j, -0.01 + 1j):
        got = tuple(float.fromhex(w) for w in probe.raw(["coefs", float(p.real).hex(), float(p.imag).hex()]).split())
        assert got == tuple(float(v) for v in apm.pair_coefs(p))


# ------------------------------------------------------------------------------------------------ sanitizers
def test_the_probe_under_address_and_undefined_sanitizers(probe, probe_san):
    """The same probe built with ``-fsanitize=address,undefined`` and run as a program: every mode at its extreme
    shapes ends with exit status 0, an empty stderr and the plain build's output."""
    rng = np.random.default_rng(3)
    rnd = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    jobs = [["coefs", float(-1.0).hex(), float(2.0).hex()]]
    for q in LU_Q:
        for tag, A in _lu_matrices(q):
            jobs.append(["lu", q, 24] + _cplx_words(A) + _cplx_words(rnd(q, 24)))
    jobs.append(["lu", 3, 1] + _cplx_words(np.zeros((3, 3))) + _cplx_words(rnd(3, 1)))
    for m, q in SHAPES:
        jobs.append(["map", m, q])
        if q > 0:
            ng, mc = apm.groups(m + q)
            jobs.append(["embed", m, q] + _cplx_words(rnd(q, m)))
            jobs.append(["smw", m, q] + _hex(0.3 * rng.standard_normal((ng, q, 2 * mc))))
    for words in jobs:
        assert probe_san.raw(words) == probe.raw(words), words[:3]
