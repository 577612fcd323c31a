"""The family of tiny and irregular operators (tests/small_ops.py) is fit for purpose -- no GPU needed:

* every operator meets the caps the device tests rely on (full row rank of J, cond S(p) <= 1e7 over the shifts
  used, block and Schur-block condition numbers <= 1e8, a stable projected pencil), each computed here;
* the dense Lyapunov and Riccati references agree with the CPU oracle on ``ricc_problem(2)``;
* the host entries of the setup behave on every operator: the tile format rebuilds S exactly, the blocks and
  aggregates are partitions, and the planned coarse space has ``kcp <= kcv``;
* every comparator the device tests use rejects a typical fault.
"""
import numpy as np
import pytest
import scipy.sparse as sps

import precond_model as pm
import saddle_model as sm
import small_ops as so
import test_saddle_tiles_cpu as tiles_cpu
from optconpy_amd import _lib
from oracle import proj_ric_utils as opru
from test_vanka_cpu import _check_records

PAIRS = [(p, 1.0) for p in so.SHIFTS + so.SHIFTS16] + [(1.0, 0.0)]


# ------------------------------------------------------------------------------------------------ the caps
@pytest.mark.parametrize("name", so.NAMES)
def test_operator_meets_the_caps(name):
    op = so.get(name)
    assert op.calA.shape == op.calE.shape == (op.nv, op.nv) and op.J.shape == (op.np, op.nv)
    assert op.np <= op.nv - 1 or op.nv == 1
    assert op.j_rank == op.np, "J has no full row rank"
    assert abs(op.calE - op.calE.T).max() == 0.0 and np.linalg.eigvalsh(op.Ed).min() > 0.0
    assert abs(op.calA - op.calA.T).max() > 0.0 or op.nv == 1, "calA is symmetric"
    conds = {ab: op.cond_S(*ab) for ab in PAIRS}
    blocks = {ab: op.block_conditioning(*ab) for ab in PAIRS}
    re_max = float(op.pencil_eigs.real.max())
    print("%s: nv %d np %d, cond S %.1e (cap %.0e), blocks %.1e (cap %.0e), max Re lambda %.2e, tol_fp64 %.1e" % (
        name, op.nv, op.np, max(conds.values()), so.COND_S_CAP, max(blocks.values()), so.COND_BLOCK_CAP, re_max,
        1e3 * pm.EPS64 * max(blocks.values())))
    assert max(conds.values()) <= so.COND_S_CAP, conds
    assert max(blocks.values()) <= so.COND_BLOCK_CAP, blocks
    assert 1e3 * pm.EPS64 * max(blocks.values()) < pm.TOL_ROUNDED
    assert re_max < 0.0, "the projected pencil is not stable"
    sh = op.shifts
    assert len(set(sh)) == len(sh) == 8 and max(sh) < 0.0
    # the dense references exist (both assert their own residual at 1e-12)
    for X in (op.lyap(), op.are(), op.are(old=True)):
        assert np.all(np.isfinite(X)) and np.linalg.norm(op.Jd @ X) <= 1e-12 * np.linalg.norm(X)
        assert np.linalg.eigvalsh(0.5 * (X + X.T)).min() >= -1e-12 * np.linalg.norm(X)


def test_family_covers_what_it_is_for():
    """The shapes and patterns the family is named for are there (computed, not assumed)."""
    ops = {n: so.get(n) for n in so.NAMES}
    plain32 = {o.nv for o in ops.values() if not o.opts and o.name.startswith("nv")}
    assert {1, 2, 15, 16, 17, 31, 32, 33, 63, 65} <= plain32
    assert {15, 16, 17} <= {o.nv for o in ops.values() if o.opts.get("bj_block") == 16}
    assert {63, 65} <= {o.nv for o in ops.values() if o.opts.get("bj_block") == 64}
    nps = {(o.np == 0, o.np == 1, o.np == o.nv - 1, 1 < o.np < o.nv - 1) for o in ops.values()}
    assert {(True, False, False, False), (False, True, False, False), (False, False, True, False),
            (False, False, False, True)} <= nps | {(False, True, True, False)}
    assert ops["fe2"].n == 18 + 8 and ops["fe3"].n == 50 + 15
    assert ops["lumped"].calE.nnz == ops["lumped"].nv
    pat = lambda m: sm._pattern(m)                                                          # noqa: E731
    out = pat(ops["e_outside"].calE) - pat(ops["e_outside"].calE).multiply(pat(ops["e_outside"].calA))
    assert out.nnz > 0, "calE lies inside calA's pattern"
    assert abs(pat(ops["unsym"].calA) - pat(ops["unsym"].calA).T).nnz > 0
    assert abs(pat(ops["nv31_np12"].calA) - pat(ops["nv31_np12"].calA).T).nnz == 0
    assert int((np.diff(ops["free_rows"].J.tocsc().indptr) == 0).sum()) >= ops["free_rows"].nv // 2
    assert np.diff(ops["dense_j_row"].J.indptr)[0] == ops["dense_j_row"].nv
    arrow = ops["arrow200"]
    assert np.diff(arrow.calA.indptr)[0] == 200 and np.diff(arrow.calA.tocsc().indptr)[0] == 200
    t = _lib.host_saddle_tiles(*arrow.ops)
    assert t["max_cols"] > tiles_cpu.MAX_COLS and not t["ms_ok"]
    # 16-column panels of the long row still fit the tile kernel's LDS budget; 32-column ones take the CSR kernel
    assert t["max_cols"] * 16 * 8 + 16 <= 40 * 1024 < t["max_cols"] * 32 * 8 + 16
    for name in ("disjoint_5_2", "disjoint_12_4"):
        J = pat(ops[name].J)
        assert abs((J @ J.T) - sps.diags((J @ J.T).diagonal())).nnz == 0, "the pressure graph has an edge"
    assert _lib.host_sa_criterion(ops["stiff_grid"].calA)[0]
    assert _lib.host_plan_levels(*ops["stiff_grid"].ops)["smoothed"]


# ------------------------------------------------------------------------------------------------ oracle
def test_dense_references_against_the_oracle():
    """``ricc_problem(2)``: the dense projected Lyapunov and Riccati solutions against the CPU oracle's iterations,
    at the bars of test_oracle.py -- the dense solution's residual, in the oracle's own residual formula, below
    1e-6 (Lyapunov, ``check_reference_identities``) and 1e-7 (Riccati, ``test_riccati_residual_small``) of the
    right-hand side; the oracle's converged iterate within 1e-6 of the dense solution."""
    op = so.get("fe2")
    F, M = sps.csr_matrix(op.calA.T), sps.csr_matrix(op.calE.T)
    d = dict(adi_max_steps=300, adi_newZ_reltol=1e-12, nwtn_max_steps=30, nwtn_upd_reltol=1e-11,
             nwtn_upd_abstol=1e-14, ms=op.shifts)
    P = op.leray
    PtW = P.T @ op.W
    rhs = np.linalg.norm(PtW @ PtW.T)
    # Lyapunov
    X = op.lyap()
    lam, U = np.linalg.eigh(X)
    L = U[:, lam > 0] * np.sqrt(lam[lam > 0])
    res = np.sqrt(abs(opru.comp_proj_lyap_res_norm(L, F, M, op.W, op.J)))
    Z = opru.solve_proj_lyap_stein(amat=F, mmat=M, jmat=op.J, wmat=op.W, adi_dict=d)["zfac"]
    print("Lyapunov: dense solution in the oracle's residual %.2e of the rhs, oracle iterate vs dense %.2e" %
          (res / rhs, so.rel(Z @ Z.T, X)))
    assert res < 1e-6 * rhs
    assert so.rel(Z @ Z.T, X) < 1e-6
    # Riccati (residual as test_oracle.py forms it)
    X = op.are()
    Md, Fd, B = M.toarray(), F.toarray(), op.B
    R = Fd.T @ X @ Md + Md.T @ X @ Fd - Md.T @ X @ B @ B.T @ X @ Md + op.W @ op.W.T
    res = np.linalg.norm(P.T @ R @ P)
    Z = opru.proj_alg_ric_newtonadi(mmat=M, amat=F, jmat=op.J, bmat=B, wmat=op.W, nwtn_adi_dict=d)["zfac"]
    print("Riccati: dense solution in the oracle's residual %.2e of the rhs, oracle iterate vs dense %.2e" %
          (res / rhs, so.rel(Z @ Z.T, X)))
    assert res < 1e-7 * rhs
    assert so.rel(Z @ Z.T, X) < 1e-6
    assert so.rel(opru.get_mTzzTtb(op.calE, Z, B), op.Ed @ X @ B) < 1e-6


# ------------------------------------------------------------------------------------------------ host entries
def _is_partition(labels, count, size):
    labels = np.asarray(labels)
    sizes = np.bincount(labels, minlength=count)
    return labels.min() >= 0 and labels.max() == count - 1 and sizes.min() >= 1 and sizes.max() <= size


@pytest.mark.parametrize("name", so.NAMES)
def test_host_entries(name):
    op = so.get(name)
    t = _lib.host_saddle_tiles(*op.ops, **op.opts)
    get = lambda _: (op.ops, t)                                                             # noqa: E731
    # perm is a permutation, every row is in exactly one row block of at most 32 rows, and the rest of the format
    tiles_cpu.test_tile_structure(get, name)
    # the tiles rebuild S(alpha, beta) exactly
    tiles_cpu.test_tile_values_rebuild_the_operator(get, name)
    assert np.array_equal(tiles_cpu._rebuild(t, -30.0 * t["src_e"][t["perm"]] + t["src_a"][t["perm"]]
                                             + t["src_j"][t["perm"]]).toarray(), op.S(-30.0, 1.0))
    # blocks and aggregates are partitions
    bs = op.opts.get("bj_block", 32)
    st = op.host_structure()
    assert not so.structure_problems(dict(st, kc=0, kcv=0, kcp=0)), so.structure_problems(st)
    for pattern, size in ((sm._pattern(op.calA) + sm._pattern(op.calE), bs), (sm._pattern(op.calE), 16),
                          (sm._pattern(op.calA), 1), (sm._pattern(op.calA), 1000)):
        blk, nb = _lib.host_aggregate(pattern.tocsr(), size)
        assert _is_partition(blk, nb, size), (name, size)
    if op.np:
        Jp = sm._pattern(op.J)
        blk, nb = _lib.host_aggregate((Jp @ Jp.T).tocsr(), 24)
        assert _is_partition(blk, nb, 24)
        _check_records(op.nv, op.J, _lib.host_vanka_patches(op.nv, op.J))
    # the planned coarse space
    for hierarchy in (0, 1):
        opts = dict(op.opts, hierarchy=hierarchy)
        plan = _lib.host_plan_levels(*op.ops, **opts)
        levels = _lib.host_plan_hierarchy(*op.ops, **opts)
        print("%s hierarchy=%d: %s" % (name, hierarchy, [(l["nv"], l["np"], l["kv"], l["kp"]) for l in levels]))
        assert plan["kc"] == plan["kcv"] + plan["kcp"] and plan["kcv"] <= op.nv and plan["kcp"] <= op.np
        assert (plan["kcv"], plan["kcp"]) == (levels[0]["kv"], levels[0]["kp"])
        assert (levels[0]["nv"], levels[0]["np"]) == (op.nv, op.np)
        for l in levels:
            if l["np"] > 0:
                assert l["kp"] <= l["kv"], (name, hierarchy, l)
            assert (l["kv"] > 0) == (l["kv"] + l["kp"] > 0)
        assert levels[-1]["dense_dim"] == levels[-1]["kv"] + levels[-1]["kp"] and not levels[-1]["has_child"]


# ------------------------------------------------------------------------------------------------ comparators
def test_comparators_reject_typical_faults():
    """Every check of tests/test_gpu_small_ops.py, fed a reference with one entry off by a relative 1e-6 or with two
    rows of one block swapped (the pattern of ``test_metric_catches_typical_kernel_bugs``)."""
    op = so.get("nv31_np12")
    rng = np.random.default_rng(0)

    def nudge(a, rel=1e-6):
        b = np.array(a, dtype=np.float64, copy=True)
        i = np.unravel_index(int(np.argmax(np.abs(b))), b.shape)
        b[i] *= 1.0 + rel
        return b

    def swap(a, i, j):
        b = np.array(a, dtype=np.float64, copy=True)
        b[[i, j]] = b[[j, i]]
        return b

    # the product: bound of saddle_model
    X = rng.standard_normal((op.n, 5))
    ref, bound = sm.reference(op.ops, -30.0, 1.0, X)
    assert sm.excess(ref, ref, bound).max() <= 1.0 < sm.excess(nudge(ref), ref, bound).max()
    assert sm.excess(swap(ref, 3, 4), ref, bound).max() > 1.0
    # the cycle: per-block errors at tol_fp64 and TOL_ROUNDED
    st = op.host_structure()
    model = pm.CycleModel(op.calA, op.calE, op.J, st)
    Zref = model.apply(-30.0, 1.0, X)
    t64 = pm.tol_fp64(model, -30.0, 1.0)
    assert t64 < pm.TOL_ROUNDED
    assert pm.worst_block_error(Zref, Zref, st) == 0.0
    assert pm.worst_block_error(nudge(Zref), Zref, st) > t64
    rows = st["bv_rows"][st["bv_ptr"][0]:st["bv_ptr"][1]]
    assert pm.worst_block_error(swap(Zref, rows[0], rows[1]), Zref, st) > pm.TOL_ROUNDED
    prows = op.nv + st["bp_rows"][st["bp_ptr"][0]:st["bp_ptr"][1]]
    assert pm.worst_block_error(swap(Zref, prows[0], prows[1]), Zref, st) > pm.TOL_ROUNDED
    # the solves: true residual and forward error
    R = rng.standard_normal((op.nv, 5))
    R[:, 2] = 0.0
    Xs = op.solve(-30.0, 1.0, np.vstack([R, np.zeros((op.np, 5))]))
    res, fwd = so.solve_ok(op, -30.0, 1.0, Xs, R)
    assert res <= 1e-13 and fwd <= 1e-13
    for bad in (nudge(Xs), swap(Xs, 3, 4), swap(Xs, op.nv, op.nv + 1)):
        with pytest.raises(AssertionError, match="residual"):
            so.solve_ok(op, -30.0, 1.0, bad, R)
    nonzero = Xs.copy()
    nonzero[5, 2] = 1e-300
    with pytest.raises(AssertionError, match="zero right-hand side"):
        so.solve_ok(op, -30.0, 1.0, nonzero, R)
    inf = Xs.copy()
    inf[0, 0] = np.inf
    with pytest.raises(AssertionError, match="not finite"):
        so.solve_ok(op, -30.0, 1.0, inf, R)
    # the iterations: Z Z^T at 1e-8, the gain at 1e-6
    Xl = op.lyap()
    assert so.rel(nudge(Xl), Xl) > 1e-8
    K = op.Ed @ op.are() @ op.B
    assert so.rel(swap(K, 0, 1), K) > 1e-6
    # the structure
    good = dict(st, kc=3, kcv=2, kcp=1, aggof=np.r_[np.arange(op.nv) % 2, np.full(op.np, 2)])
    assert not so.structure_problems(good)
    for change, word in ((dict(kcv=1, kcp=2, aggof=np.r_[np.zeros(op.nv, int), 1 + np.arange(op.np) % 2]), "kcp"),
                         (dict(aggof=np.r_[np.zeros(op.nv, int), np.full(op.np, 2)]), "empty"),
                         (dict(aggof=np.r_[np.arange(op.nv) % 3, np.full(op.np, 2)]), "outside"),
                         (dict(bv_rows=np.zeros(op.nv, np.int32)), "permutation"),
                         (dict(bs=8), "rows")):
        found = so.structure_problems(dict(good, **change))
        assert any(word in f for f in found), (change, found)
    # the smoothed prolongation at 1e-14
    sg = so.get("stiff_grid")
    vagg, kv = _lib.host_aggregate(sm._pattern(sg.calE), 16)
    pagg, kp = _lib.host_aggregate((sm._pattern(sg.J) @ sm._pattern(sg.J).T).tocsr(), 24)
    stg = dict(nv=sg.nv, np=sg.np, kc=kv + kp, aggof=np.r_[vagg, kv + pagg])
    P = so.smoothed_prolongation(sg.calA, stg)
    assert 0.0 < so.smoothing_omega(sg.calA) <= 0.5
    assert np.abs(P.sum(axis=1)[:sg.nv] - 1.0).max() > 1e-3, "nothing was smoothed"
    assert np.abs(nudge(P) - P).max() > 1e-14
