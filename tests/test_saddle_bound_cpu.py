"""The per-element bound of the saddle product tests (tests/saddle_model.py, used by tests/test_gpu_saddle_spmm.py)
has teeth: each plausible kernel mistake, applied to the SciPy reference, exceeds it by at least 10x on the test
operators, while the same product summed in another order stays within it."""
import numpy as np
import pytest
import scipy.sparse as sps

import saddle_model as sm

TEETH = 10.0
GROUPS = [(-37.5, 0.37), (-3.0, 1.0), (-900.0, 1.0)]   # one DRE-style shift (beta != 1)


@pytest.fixture(scope="module")
def ops():
    base = sm.th_operators(15, 0.1)
    return {"cfg1": base, "long100": sm.long_rows(base, [49, 64, 100], p_target=60)[0]}


def _x(n, m=16, seed=0, x32=False):
    X = np.random.default_rng(seed).standard_normal((n, m))
    return X.astype(np.float32).astype(np.float64) if x32 else X


def _worst(Y, ref, bound, y32=False):
    return float(np.max(sm.excess(Y, ref, bound, y32)))


@pytest.mark.parametrize("name", ["cfg1", "long100"])
@pytest.mark.parametrize("x32", [False, True], ids=["x64", "x32"])
def test_other_summation_order_passes(ops, name, x32):
    o = ops[name]
    n = o[0].shape[0] + o[2].shape[0]
    X = _x(n, x32=x32)
    for a, b in GROUPS:
        ref, bound = sm.reference(o, a, b, X)
        S = sm.saddle(*o, a, b)
        # reversed column order: every row summed the other way round
        rev = S[:, ::-1].tocsr() @ X[::-1]
        assert _worst(rev, ref, bound) <= 1.0
        assert _worst(rev.astype(np.float32).astype(np.float64), ref, bound, y32=True) <= 1.0


def _mistakes(o, a, b, X, other):
    """name -> the wrong product of one group."""
    calA, calE, J = o
    S = sm.saddle(calA, calE, J, a, b)
    out = {}
    S32 = S.copy()
    S32.data = S32.data.astype(np.float32).astype(np.float64)
    out["values_fp32"] = S32 @ X
    St = S.copy()
    for i in range(St.shape[0]):
        lo, hi = St.indptr[i], St.indptr[i + 1]
        if hi - lo > 48:
            St.data[lo + 48:hi] = 0.0
    out["long_row_past_48_dropped"] = St @ X
    out["other_group_shift"] = sm.saddle(calA, calE, J, *other) @ X
    m = X.shape[1]
    shifted = np.arange(m)
    shifted = (shifted // 16) * 16 + (shifted % 16 + 1) % min(16, m)
    out["column_shift_in_pass"] = S @ X[:, shifted]
    out["bit15_ignored"] = sps.bmat([[b * calA + a * calE, b * J.T], [b * J, None]], format="csr") @ X
    return out


@pytest.mark.parametrize("name", ["cfg1", "long100"])
@pytest.mark.parametrize("x32", [False, True], ids=["x64", "x32"])
def test_kernel_mistakes_exceed_the_bound(ops, name, x32):
    o = ops[name]
    n = o[0].shape[0] + o[2].shape[0]
    X = _x(n, seed=3, x32=x32)
    a, b = GROUPS[0]
    ref, bound = sm.reference(o, a, b, X)
    seen = {}
    for what, Y in _mistakes(o, a, b, X, GROUPS[1]).items():
        if what == "long_row_past_48_dropped" and name == "cfg1":
            assert np.array_equal(Y, sm.saddle(*o, a, b) @ X)   # no row that long: nothing to drop
            continue
        seen[what] = (_worst(Y, ref, bound), _worst(Y.astype(np.float32).astype(np.float64), ref, bound, True))
    print("[saddle bound] %s/%s: worst error over bound per mistake (FP64 out, FP32 out): %s" %
          (name, "x32" if x32 else "x64", {k: "%.1e, %.1e" % v for k, v in seen.items()}))
    for what, (w64, w32) in seen.items():
        assert w64 >= TEETH, (what, w64)
        if what != "values_fp32":       # an FP32 output panel cannot tell FP32-rounded values apart
            assert w32 >= TEETH, (what, w32)
