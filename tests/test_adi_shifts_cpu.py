"""Automatic ADI shifts (``ms='auto'``) without a GPU: Penzl's selection, the Cauchy admissibility of the list,
the ``adi_dict`` contract, and the recipe on the oracle's ADI (``adi_shift_model``)."""
import numpy as np
import pytest

from optconpy_amd import _lib, adi_shifts as ads, problems as pb, proj_ric_utils as pru


def _worst(ms, cands):
    c = np.asarray(cands, dtype=float)
    return float(np.max(np.prod([np.abs((c - p) / (c + p)) for p in ms], axis=0)))


def _clustered():
    rng = np.random.default_rng(3)
    return np.concatenate([-rng.uniform(0.8, 1.2, 20), -rng.uniform(30.0, 36.0, 20), -rng.uniform(700.0, 1000.0, 20)])


def _all_windows_pass(ms, width=16):
    n = len(ms)
    for g in range(2, min(width, n) + 1):
        for s in range(n):
            _lib.host_cauchy([ms[(s + i) % n] for i in range(g)])      # raises on a failing window
    return True


def test_penzl_one_candidate_gives_itself():
    assert ads.penzl_select([-3.5], 8) == [-3.5]
    assert ads.penzl_select([-3.5, -3.51], 8) == [-3.5]                  # merged within 1 %


def test_penzl_two_clusters_one_pick_each_first():
    lo = [-1.0, -1.05, -1.1, -0.97]
    hi = [-100.0, -104.0, -110.0, -96.0]
    picks = ads.penzl_select(lo + hi, 4)
    assert len(picks) == 4
    first_two = picks[:2]
    assert sum(p in lo for p in first_two) == 1 and sum(p in hi for p in first_two) == 1


@pytest.mark.parametrize("num", [4, 6, 8])
def test_penzl_minmax_not_worse_than_logshifts(num):
    c = _clustered()
    picks = ads.penzl_select(c, num)
    assert len(picks) == num and all(p < 0 for p in picks)
    lo, hi = float(np.abs(c).min()), float(np.abs(c).max())
    assert _worst(picks, c) <= _worst(pb.logshifts(lo, hi, num), c)


@pytest.mark.parametrize("cands", [
    -np.logspace(0, 3, 200),                                     # dense: eight picks, all kept
    _clustered(),
    -np.linspace(0.5, 0.65, 40),                                 # narrow: close picks, some must go
    np.concatenate([-np.linspace(1.0, 1.3, 30), -np.logspace(1, 4, 12)]),
])
def test_auto_style_list_passes_every_cauchy_window(cands):
    ms = ads.admissible_order(ads.penzl_select(cands, 8))
    assert 1 <= len(ms) <= 8
    assert len(set(ms)) == len(ms) and all(p < 0 for p in ms)
    assert ms == sorted(ms, key=abs)                              # logshifts order (<= 16 entries)
    assert _all_windows_pass(ms)


def test_narrow_candidates_are_thinned():
    picks = ads.penzl_select(-np.linspace(0.5, 0.65, 40), 8)
    with pytest.raises(RuntimeError):
        _all_windows_pass(sorted(picks, key=abs))                 # the raw picks would break a sweep
    assert len(ads.admissible_order(picks)) < len(picks)


def test_shifts_accepts_auto_and_still_rejects_the_rest():
    assert pru._shifts({"ms": "auto"}) == "auto"
    assert pru._shifts({}) == pru.DEFAULT_MS
    assert pru._shifts({"ms": [-1, -2]}) == [-1.0, -2.0]
    for bad in ("foo", [1.0], [-1, 2]):
        with pytest.raises((ValueError, TypeError)):
            pru._shifts({"ms": bad})


def test_initial_shift():
    assert ads.initial_shift(np.array([0.25, 4.0, 1.0])) == -1.0
    assert ads.initial_shift(None) == -1.0


@pytest.mark.parametrize("tau", [1e-4, 1e-3, 1e-2])
def test_model_shifts_cut_oracle_adi_steps(tau):
    """The recipe on the oracle's ADI, DRE time-step operator at N = 20, nu = 0.05: at most 0.6 x the ADI steps
    of DEFAULT_MS."""
    from identities import dre_step_inputs
    from oracle import proj_ric_utils as opru
    from adi_shift_model import model_shifts
    pr = pb.ricc_problem(20, 0.05)
    kw, _ = dre_step_inputs(pr, tau=tau)
    calA, calE, J, W = kw["amat"], kw["mmat"], kw["jmat"], kw["wmat"]
    ms = model_shifts(calA, calE, J, W)
    assert 1 <= len(ms) <= 8 and all(p < 0 for p in ms)
    assert _all_windows_pass(ms)
    a = dict(adi_newZ_reltol=1e-8)
    base = opru.solve_proj_lyap_stein(amat=calA, mmat=calE, jmat=J, wmat=W, transposed=True, adi_dict=a)
    auto = opru.solve_proj_lyap_stein(amat=calA, mmat=calE, jmat=J, wmat=W, transposed=True,
                                      adi_dict=dict(a, ms=ms))
    assert auto["adi_rel_newZ"] < 1e-8
    assert auto["adi_steps"] <= 0.6 * base["adi_steps"], (auto["adi_steps"], base["adi_steps"], ms)
