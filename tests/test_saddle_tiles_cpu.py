"""The row-block tile format of the saddle SpMM (``ricadi_host_saddle_tiles``: what ``ricadi_set_operator`` uploads
for the tile kernels ``spmm_blocked_kernel`` and ``spmm_blocked_ms_kernel``), checked on the host: its structural
rules, and the operator S(alpha, beta) rebuilt from the tile format alone, indexed as the kernels index it, against
the SciPy saddle matrix."""
import numpy as np
import pytest
import scipy.sparse as sps

from optconpy_amd import _lib
import saddle_model as sm

SHIFTS = [(-1.0, 1.0), (-37.5, 0.37), (-1500.0, 2.0), (0.0, 1.0), (1.0, 0.0)]
MAX_COLS = 152      # kSbMaxCols of the tile builder
MS_MAX_COLS = 160   # the multi-shift kernel's tile slots


def _operators(name):
    if name.startswith("th"):
        return sm.th_operators(int(name[2:]))
    base = sm.th_operators(15, 0.1)
    if name == "long100":
        return sm.long_rows(base, [49, 64, 100], p_target=60)[0]
    if name == "long250":
        return sm.long_rows(base, [49, 64, 100, 170, 250])[0]
    if name == "long400":
        return sm.long_rows(base, [400])[0]
    raise KeyError(name)


NAMES = ["th6", "th15", "th30", "long100", "long250", "long400"]


@pytest.fixture(scope="module")
def tiles():
    cache = {}

    def get(name):
        if name not in cache:
            ops = _operators(name)
            cache[name] = (ops, _lib.host_saddle_tiles(*ops))
        return cache[name]
    return get


def _blocks(t):
    """Per block: (global rows in local order, entry range per local row, columns)."""
    for b in range(t["nblk"]):
        rows = t["rows2"][b]
        nr = int(np.sum(rows >= 0))
        cols = t["cols2"][b]
        nc = int(np.sum(cols >= 0))
        yield b, rows, nr, t["rp2"][b], cols, nc


@pytest.mark.parametrize("name", NAMES)
def test_tile_structure(tiles, name):
    ops, t = tiles(name)
    n, nv, nnz = t["n"], t["nv"], t["nnz"]
    assert n == ops[0].shape[0] + ops[2].shape[0] and nv == ops[0].shape[0]
    assert t["sb_ok"]
    s_rp, s_ci, lidx, perm = t["s_rp"], t["s_ci"], t["lidx"], t["perm"]
    assert s_rp[-1] == nnz and np.all(np.diff(s_rp) >= 0)
    assert np.array_equal(np.diff(s_rp), sm.row_lengths(*ops))
    # the tile order is a permutation of the saddle CSR entries
    assert np.array_equal(np.sort(perm), np.arange(nnz))
    seen = []
    widest = 0
    prev_end = 0
    for b, rows, nr, rp2, cols, nc in _blocks(t):
        assert 1 <= nr <= 32, (b, nr)
        assert np.all(rows[:nr] >= 0) and np.all(rows[nr:] == -1), b
        # a velocity block never runs into the pressure rows
        vel = rows[:nr] < nv
        assert vel.all() or not vel.any(), b
        # entry ranges: contiguous over the blocks, monotone, padded with the block's end
        assert rp2[0] == prev_end, b
        assert np.all(np.diff(rp2) >= 0), b
        assert np.all(rp2[nr:] == rp2[nr]), b
        prev_end = rp2[32]
        # columns: sorted, distinct, padded with -1
        assert nc >= 1 and np.all(cols[nc:] == -1) and np.all(np.diff(cols[:nc]) > 0), b
        assert cols[0] >= 0 and cols[nc - 1] < n
        widest = max(widest, nc)
        if nc > MAX_COLS:
            # only the first row of a block is taken whatever its width: then it is the block's only row
            assert nr == 1 and s_rp[rows[0] + 1] - s_rp[rows[0]] == nc, (b, nr, nc)
        for q in range(nr):
            row = rows[q]
            ks = np.arange(rp2[q], rp2[q + 1])
            src = perm[ks]
            assert ks.size == s_rp[row + 1] - s_rp[row], (b, q)
            assert np.all((src >= s_rp[row]) & (src < s_rp[row + 1])), (b, q)
            l = lidx[ks].astype(np.int64)
            assert np.all(l < nc), (b, q)
            assert np.array_equal(cols[l], s_ci[src]), (b, q)
            # parity order: entries whose tile slot has the parity of the local row first, each part in CSR order
            first = (l & 1) == (q & 1)
            assert not np.any(first[1:] & ~first[:-1]), (b, q)
            assert np.all(np.diff(src[first]) > 0) and np.all(np.diff(src[~first]) > 0), (b, q)
            seen.append(row)
    assert prev_end == nnz
    # every saddle row exactly once
    assert np.array_equal(np.sort(seen), np.arange(n))
    assert t["max_cols"] == widest
    assert t["ms_ok"] == (t["max_cols"] <= MS_MAX_COLS)


def test_long_row_operators_reach_the_tile_limits(tiles):
    """The long-row operators of the GPU tests do what they are there for: rows of more than 48 entries inside a
    tile (the streamed part of both tile kernels), max_cols > 192 (second pass of the 16-byte tile fill) with tiles
    that still fit 16-column panels, and max_cols > 320 (16-column panels on the CSR kernel)."""
    lmax = {name: int(np.max(np.diff(tiles(name)[1]["rp2"], axis=1))) for name in NAMES}
    assert lmax["th6"] <= 48 and lmax["th15"] <= 48 and lmax["th30"] <= 48, lmax
    t100, t250, t400 = (tiles(k)[1] for k in ("long100", "long250", "long400"))
    assert lmax["long100"] == 100 and t100["ms_ok"] and t100["max_cols"] <= 152
    # the pressure row of 60 entries sits in a pressure block
    nv = t100["nv"]
    prow_len = [np.max(np.diff(rp2)) for _, rows, nr, rp2, _, _ in _blocks(t100) if rows[0] >= nv]
    assert max(prow_len) == 60
    assert lmax["long250"] == 250 and 192 < t250["max_cols"] <= 319 and not t250["ms_ok"]
    assert t400["max_cols"] > 320


def _rebuild(t, vals):
    """S from the tile format: entry k of local row q of block b is vals[k] at (rows2[b][q], cols2[b][lidx[k]])."""
    r, c, k = [], [], []
    for b, rows, nr, rp2, cols, nc in _blocks(t):
        for q in range(nr):
            ks = np.arange(rp2[q], rp2[q + 1])
            r.append(np.full(ks.size, rows[q]))
            c.append(cols[t["lidx"][ks].astype(np.int64)])
            k.append(ks)
    r, c, k = (np.concatenate(x) for x in (r, c, k))
    return sps.csr_matrix((vals[k], (r, c)), shape=(t["n"], t["n"]))


@pytest.mark.parametrize("name", NAMES)
def test_tile_values_rebuild_the_operator(tiles, name):
    """Per-group form: values alpha E + beta A + J gathered through ``perm`` (what assemble_shift and gather_vals
    build on the device) -- exactly the SciPy matrix.  Multi-shift form: fma(alpha, vE, (bit 15 ? beta : 1) vAJ) --
    within one rounding per entry; bit 15 set exactly on the velocity-velocity entries."""
    ops, t = tiles(name)
    perm, nv = t["perm"], t["nv"]
    a, e, j = t["src_a"][perm], t["src_e"][perm], t["src_j"][perm]
    if t["ms_ok"]:
        lm = t["lidx_ms"]
        assert np.array_equal(lm & 0x7FFF, t["lidx"])
        rows = np.repeat(np.arange(t["n"]), np.diff(t["s_rp"]))[perm]
        vv = (rows < nv) & (t["s_ci"][perm] < nv)
        assert np.array_equal((lm & 0x8000) != 0, vv)
        assert np.array_equal(t["vAJ"], a + j) and np.array_equal(t["vE"], e)
        # the two value sources have disjoint supports
        assert not np.any((a != 0) & (j != 0))
    else:
        assert t["lidx_ms"] is None
    for al, be in SHIFTS:
        S = sm.saddle(*ops, al, be)
        T = _rebuild(t, al * e + be * a + j)
        assert abs(T - S).max() == 0.0, (name, al, be)
        if t["ms_ok"]:
            flag = (t["lidx_ms"] & 0x8000) != 0
            Tm = _rebuild(t, al * t["vE"] + np.where(flag, be, 1.0) * t["vAJ"])
            Sabs = sm.saddle_abs(*ops, al, be)
            D = abs(Tm - S) - sm.EPS * Sabs
            assert D.max() <= 0.0, (name, al, be)
