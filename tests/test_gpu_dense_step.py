"""GPU tests of the dense layer of an ADI step (ricadi_dense.hip, solver_dense.inl), entry by entry against the
longdouble model of tests/dense_model.py: the MFMA GEMMs in all their launch forms, the sweep recombination (fused
kernel and per-block path through the one entry), the panel helpers, block QR at the panel and row-block edges, the
recompression branches and the factored Lyapunov residual.

Products are compared COMPONENTWISE at ``bound(2^-53) + bound(u_longdouble)`` with the bounds of the standard
dot-product analysis (dense_model.py; tests/test_dense_model_cpu.py shows that float64 NumPy meets them at every shape
used here and that the faults these tests exist for do not).  Every test prints its largest ``error / bound``.
"""
import numpy as np
import pytest
import scipy.sparse as sps

import dense_model as dm
from optconpy_amd import _lib
from oracle import proj_ric_utils as opru

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ contexts
@pytest.fixture(scope="module")
def dims_ctx():
    """``dims_ctx(nv)``: the module's dimension-only context for ``nv`` rows (one per distinct nv)."""
    made = {}

    def get(nv):
        if nv not in made:
            made[nv] = _lib.Context(0)
            made[nv].set_dims(nv)
        return made[nv]

    yield get
    for ctx in made.values():
        ctx.close()


@pytest.fixture(scope="module")
def ctx1(cfg1):
    pr = cfg1[0]
    ctx = _lib.Context(0)
    ctx.set_operator((-pr.A - pr.Nc).T.tocsr(), pr.M.T.tocsr(), pr.J)
    yield ctx
    ctx.close()


def _dev(a):
    """Device copy of a host array, complete before the library's own stream may touch it."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _nan(*shape):
    """Device buffer for a result, filled with NaN: whatever the entry does not write shows."""
    import torch
    t = torch.full(shape, float("nan"), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _check(name, got, ref, tolerance):
    r = dm.ratio(got, ref, tolerance)
    print("%s: error / bound %.3g" % (name, r))
    assert r <= 1.0, (name, r)


# ------------------------------------------------------------------------------------------------ a. Gram
def gram_form(c):
    return "thin" if c < 128 else ("wide+combine" if ((c + 63) // 64) * ((c + 63) // 64 + 1) // 2 <= 16 else "wide")


@pytest.mark.parametrize("nv,c", dm.GRAM_CASES)
def test_gram_elementwise(dims_ctx, nv, c):
    """launch_gemm_tn, symmetric forms: <2,2> thin (c < 128), <4,4> wide with the LDS combine (c <= 320: at most 15
    upper tile blocks) and without (c >= 321: 21 and more).  nv = 1 .. 1021 covers a single 4-row step, the row tail
    nv % 4, surplus waves (rbeg >= n) and several row slices."""
    ctx = dims_ctx(nv)
    Z = dm.panel(1, nv, c)
    Zd = _dev(Z)
    Gd = _nan(c, c)                    # the entry zeroes it itself
    ctx.time_gram_dev(Zd.data_ptr(), c, Gd.data_ptr(), 1)
    G = _host(Gd)
    _check("gram %s nv=%d c=%d" % (gram_form(c), nv, c), G, dm.gram(Z), dm.tol(dm.gram_bound, Z))
    if c < 128:
        # the thin form adds the SAME value v at (i, j) and (j, i); the wide forms mirror with independent atomics of
        # every wave and get the componentwise bound only
        assert np.array_equal(G, G.T), np.abs(G - G.T).max()


# ------------------------------------------------------------------------------------------------ b. general TN / NN
_MT = {}


def _gain_mt(nv, kind):
    if (nv, kind) not in _MT:
        _MT[nv, kind] = sps.identity(nv, format="csr") if kind == "identity" else dm.sparse_rows(nv, 5, seed=7)
    return _MT[nv, kind]


@pytest.mark.parametrize("nv,nb,c", dm.GAIN_CASES)
def test_gain_explicit_mt(dims_ctx, nv, nb, c):
    """gain = MT (Z (Z^T B)): the general (non-symmetric) gemm_tn -- thin, and wide from c >= 128 with nb = 128,
    512 / 513 on either side of the combine's 16 tiles -- then gemm_nn (p = c with its % 4 tail, q = nb with its
    % 32 tail, beta == 0 on an uninitialised target) and the CSR product."""
    ctx = dims_ctx(nv)
    Z, B = dm.panel(8, nv, c), dm.panel(9, nv, nb)
    st = dm.gain_stages(Z, B)
    for kind in ("identity", "sparse"):
        MT = _gain_mt(nv, kind)
        K = ctx.gain(B, Z=Z, MT=MT)
        _check("gain %s nv=%d nb=%d c=%d" % (kind, nv, nb, c), K, dm.gain(MT, Z, B, 1.0, st),
               dm.tol(dm.gain_bound, MT, Z, B, 1.0, stages=st))


@pytest.mark.parametrize("c,nb", [(5, 7), (64, 1), (129, 33), (130, 128)])
def test_gain_dev_padded_factor(ctx1, cfg1, c, nb):
    """ricadi_gain_dev with ldz = c + 5: the five unused columns hold NaN and must not be read; coef = -1."""
    pr = cfg1[0]
    E = pr.M.T.tocsr()
    Z, B = dm.panel(18, pr.NV, c), dm.panel(19, pr.NV, nb)
    Zp = np.full((pr.NV, c + 5), np.nan)
    Zp[:, :c] = Z
    Zd, Bd = _dev(Zp), _dev(B)
    Kd = _nan(pr.NV, nb)
    ctx1.gain_dev(-1.0, Zd.data_ptr(), c, c + 5, Bd.data_ptr(), nb, Kd.data_ptr())
    _check("gain_dev c=%d nb=%d" % (c, nb), _host(Kd), dm.gain(E, Z, B, -1.0), dm.tol(dm.gain_bound, E, Z, B, -1.0))


# ------------------------------------------------------------------------------------------------ c. panel norms
@pytest.mark.parametrize("nrows,m", dm.NORMS_CASES)
def test_panel_norms(ctx1, nrows, m):
    W = dm.panel(10, nrows, m)
    Wd = _dev(W)
    f, tr = ctx1.panel_norms_dev(Wd.data_ptr(), nrows, m)
    (rf, rtr), (tf, ttr) = dm.panel_norms(W), dm.tol(dm.panel_norms_bound, W)
    _check("panel_norms trace nrows=%d m=%d" % (nrows, m), tr, rtr, ttr)
    _check("panel_norms gram_fro nrows=%d m=%d" % (nrows, m), f, rf, tf)


# ------------------------------------------------------------------------------------------------ d. recombination
def _sweep_inputs(pr, nslot, G, m):
    E = pr.M.T.tocsr()
    coefz, coefw, pad = dm.sweep_tables(nslot, G, seed=11)
    Us = dm.panel(12, nslot, pr.NV, m)
    Us[pad] = 0.0                      # padding slots travel as exact zeros (include/ricadi.h)
    W = dm.panel(13, pr.NV, m)         # dW starts non-zero
    return Us, coefz, coefw, E, W


@pytest.mark.parametrize("nslot,G,m", dm.SWEEP_CASES)
def test_sweep_recombine_slots(ctx1, cfg1, nslot, G, m):
    """ricadi_sweep_recombine_slots_dev = the ADI driver's sweep_blocks: the fused sweep_combine_kernel +
    sweep_norms_kernel up to 16 slots and 16 blocks (256 % m idle threads at m = 7, 33, 100; the full 16 x 16
    coefficient table; m = 128 = RICADI_MAX_M), the per-block path at (17, 4, 16) and (4, 17, 8)."""
    pr = cfg1[0]
    Us, coefz, coefw, E, W = _sweep_inputs(pr, nslot, G, m)
    Ud = _dev(Us)
    ref = dm.recombine(Us, coefz, coefw, E, W)
    tZ, tW, tbn, ttot = dm.tol(dm.recombine_bound, Us, coefz, coefw, E, W, Z=ref[0])
    runs = []
    for _ in range(2):
        Zd = _nan(pr.NV, G * m)
        Wd = _dev(W)
        n2, bn = ctx1.sweep_recombine_slots_dev(nslot, G, Ud.data_ptr(), m, coefz, coefw, Zd.data_ptr(), Wd.data_ptr())
        runs.append((_host(Zd), _host(Wd), bn, n2))
    tag = "recombine %s (%d, %d, %d)" % ("fused" if dm.sweep_fused(nslot, G, m) else "per block", nslot, G, m)
    Z, Wn, bn, n2 = runs[0]
    _check(tag + " Z", Z, ref[0], tZ)
    _check(tag + " W", Wn, ref[1], tW)
    _check(tag + " block_n2", bn, ref[2], tbn)
    _check(tag + " n2", n2, ref[3], ttot)
    if dm.sweep_fused(nslot, G, m):
        # fixed-order sums: the ranks of a sharded run take the stopping decisions from these bits on their own
        assert np.array_equal(runs[0][2], runs[1][2]) and runs[0][3] == runs[1][3]
        assert np.array_equal(runs[0][0], runs[1][0])


def test_sweep_recombine_cauchy(ctx1, cfg1):
    """ricadi_sweep_recombine_dev with the Cauchy data of a real shift sweep (R^-1 upper triangular, C^-1 1)."""
    pr = cfg1[0]
    G, m = 4, 8
    rinv, cinv1 = _lib.host_cauchy([-1.0, -7.0, -50.0, -400.0])
    assert np.all(np.tril(rinv, -1) == 0)
    E = pr.M.T.tocsr()
    Us, W = dm.panel(20, G, pr.NV, m), dm.panel(21, pr.NV, m)
    Ud, Wd = _dev(Us), _dev(W)
    Zd = _nan(pr.NV, G * m)
    n2 = ctx1.sweep_recombine_dev(G, Ud.data_ptr(), m, rinv, cinv1, Zd.data_ptr(), Wd.data_ptr())
    ref = dm.recombine(Us, rinv, cinv1, E, W)
    tZ, tW, tbn, ttot = dm.tol(dm.recombine_bound, Us, rinv, cinv1, E, W, Z=ref[0])
    _check("recombine cauchy Z", _host(Zd), ref[0], tZ)
    _check("recombine cauchy W", _host(Wd), ref[1], tW)
    _check("recombine cauchy n2", n2, ref[3], ttot)


# ------------------------------------------------------------------------------------------------ e. lincomb
@pytest.mark.parametrize("nrows,m,nvec", dm.LINCOMB_CASES)
def test_lincomb(ctx1, nrows, m, nvec):
    """Panels ``nrows*m + 24`` doubles apart: the stride is not the panel size; the gaps hold NaN."""
    P, coef = dm.panel(14, nvec, nrows, m), dm.panel(15, nvec)
    stride = nrows * m + 24
    buf = np.full((nvec, stride), np.nan)
    buf[:, :nrows * m] = P.reshape(nvec, -1)
    Bd = _dev(buf)
    Od = _nan(nrows, m)
    ctx1.lincomb_dev(nrows, m, coef, Bd.data_ptr(), stride, Od.data_ptr())
    ctx1.synchronize()
    _check("lincomb nrows=%d m=%d nvec=%d" % (nrows, m, nvec), _host(Od), dm.lincomb(coef, P),
           dm.tol(dm.lincomb_bound, coef, P))


# ------------------------------------------------------------------------------------------------ f. apply_e
@pytest.mark.parametrize("m", [1, 16, 33])
@pytest.mark.parametrize("coef", [1.0, -0.5])
def test_apply_e(ctx1, cfg1, m, coef):
    """dV is an n x m panel whose pressure rows hold NaN: only the first NV rows may be read."""
    pr = cfg1[0]
    E = pr.M.T.tocsr()
    V, W = dm.panel(16, pr.NV, m), dm.panel(17, pr.NV, m)
    Vn = np.full((pr.NV + pr.NP, m), np.nan)
    Vn[:pr.NV] = V
    Vd, Wd = _dev(Vn), _dev(W)
    ctx1.apply_e_dev(coef, Vd.data_ptr(), m, Wd.data_ptr())
    ctx1.synchronize()
    _check("apply_e m=%d coef=%g" % (m, coef), _host(Wd), dm.apply_e(E, V, W, coef),
           dm.tol(dm.apply_e_bound, E, V, W, coef))


# ------------------------------------------------------------------------------------------------ g. block QR
def _qr_properties(Q, R, Z):
    c = Z.shape[1]
    assert np.all(np.tril(R, -1) == 0)
    res = np.linalg.norm(Q @ R - Z) / np.linalg.norm(Z)
    orth = np.linalg.norm(Q.T @ Q - np.eye(c))
    assert res <= 1e-13, res
    assert orth <= 1e-12, orth
    return res, orth


@pytest.mark.parametrize("nv,c", dm.QR_CASES)
def test_block_qr_against_householder(dims_ctx, nv, c):
    """Block QR (128-column CholQR2 panels, block Gram-Schmidt with re-orthogonalisation between them) at the panel
    edges c = 127 / 128 / 129 and 257, square (nv = c) and at the TSQR row-block edge 255 / 256 / 257, on matrices
    with singular values in [1, 10].  R is compared entry by entry with the longdouble Householder R; the tolerance
    is not derivable: it is QR_R_FACTOR = 10 times QR_R_DISTANCE = 9.3e-17 ||Z||_F, the largest distance of LAPACK's
    float64 Householder R from that reference over these same matrices (measured on the CPU,
    test_dense_model_cpu.py)."""
    Z = dm.qr_matrix(nv, c)
    Q, R = dims_ctx(nv).qr(Z)
    res, orth = _qr_properties(Q, R, Z)
    d = dm.r_distance(dm.fix_row_signs(R), dm.qr_reference_r(nv, c))
    print("block QR nv=%d c=%d: residual %.2e  orthogonality %.2e  R distance %.2e = %.2f of the allowance" %
          (nv, c, res, orth, d, d / (dm.QR_R_FACTOR * dm.QR_R_DISTANCE)))
    assert d <= dm.QR_R_FACTOR * dm.QR_R_DISTANCE, d


@pytest.mark.parametrize("nv,c", [(nv, c) for nv, c in dm.QR_CASES if c >= 2])
def test_block_qr_repeated_column(dims_ctx, nv, c):
    """Column 1 = column 0 exactly: the CholQR2 panel raises its flag and the factorisation is redone through the
    Householder TSQR tree (32-column panels; nv = 2049: 9 blocks, 288 rows, 2 blocks)."""
    Z = dm.qr_matrix(nv, c).copy()
    Z[:, 1] = Z[:, 0]
    Q, R = dims_ctx(nv).qr(Z)
    res, orth = _qr_properties(Q, R, Z)
    print("block QR, repeated column, nv=%d c=%d: residual %.2e  orthogonality %.2e  |R11| %.2e" %
          (nv, c, res, orth, abs(R[1, 1])))
    assert abs(R[1, 1]) <= 1e-14 * np.linalg.norm(Z)


# ------------------------------------------------------------------------------------------------ h. recompression
@pytest.mark.parametrize("nv,c", [(1100, 1024), (1100, 1025), (2100, 2049)])
def test_recompress_branches(dims_ctx, nv, c):
    """The assertions of test_recompress_pivoted_cholesky_route at the first pass's edge between one and two columns
    per thread (1024 / 1025) and at c + min(c, nv) = 4149 > 4096 columns, where the pivoted Cholesky does not apply
    and the Gram + eigensolver route serves (the smallest shape that reaches it; the slowest case of this file)."""
    from test_gpu_round3 import _graded_factor
    Z = _graded_factor(nv, c, 14, seed=c)
    Zc = dims_ctx(nv).recompress(Z)
    U, s, _ = np.linalg.svd(Z, full_matrices=False)
    k_opt = int((s > 3e-8 * s[0]).sum())
    X = Z @ Z.T
    err = np.linalg.norm(Zc @ Zc.T - X) / np.linalg.norm(X)
    print("recompress nv=%d c=%d: %d columns (optimal %d), ||Zc Zc^T - Z Z^T|| %.2e" % (nv, c, Zc.shape[1], k_opt, err))
    assert err <= 2e-14
    assert k_opt - 2 <= Zc.shape[1] <= k_opt + max(6, k_opt // 20), (Zc.shape[1], k_opt)
    U = U[:, :min(k_opt + 40, min(Z.shape))]
    assert np.linalg.norm(Zc - U @ (U.T @ Zc)) <= 1e-7 * np.linalg.norm(Zc)


# ------------------------------------------------------------------------------------------------ i. Lyapunov residual
@pytest.mark.parametrize("c", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("m", [1, 5])
def test_lyap_res_norm(ctx1, cfg1, c, m):
    """ricadi_lyap_res_norm (the SQUARED norm) against the oracle, with and without a low-rank term; c around the
    64-column chunks, 2 c + m > 128 columns in the final Gram matrix.  rtol 1e-7: the projection is an iterative
    solve (the bar of test_gpu_parity.py for this quantity)."""
    pr = cfg1[0]
    F = (-pr.A - pr.Nc).tocsr()
    Z, W = dm.panel(22, pr.NV, c), dm.panel(23, pr.NV, m)
    r_gpu = ctx1.lyap_res_norm(Z, W)
    r_ref = opru.comp_proj_lyap_res_norm(Z, F, pr.M, W, pr.J)
    print("lyap_res_norm c=%d m=%d: rel diff %.2e" % (c, m, abs(r_gpu - r_ref) / r_ref))
    assert r_ref > 0 and np.isclose(r_gpu, r_ref, rtol=1e-7)
    Ul, Vl = 0.1 * dm.panel(24, pr.NV, 3), dm.panel(25, pr.NV, 3)
    ctx1.set_lowrank(Ul, Vl)
    try:
        r_gpu = ctx1.lyap_res_norm(Z, W)
    finally:
        ctx1.set_lowrank(None, None)
    r_ref = opru.comp_proj_lyap_res_norm(Z, sps.csr_matrix(F.toarray() - Vl @ Ul.T), pr.M, W, pr.J)
    print("lyap_res_norm + low rank c=%d m=%d: rel diff %.2e" % (c, m, abs(r_gpu - r_ref) / r_ref))
    assert r_ref > 0 and np.isclose(r_gpu, r_ref, rtol=1e-7)
