"""The step model of the Arnoldi / Givens layer (tests/arnoldi_model.py) against a float64 NumPy implementation of
the same steps: at every shape, form and scenario of tests/test_gpu_arnoldi_steps.py the float64 implementation
meets every bound (and keeps the stored vectors inside the boundary-straddling limit), and each of the faults the
bounds exist for does not."""
import numpy as np
import pytest

import arnoldi_model as am


def _run(case, mutation=None, form=None):
    form = form or am.nominal_form(case["switch"], case["m"])
    n = am.N_ROWS[case["op"]]
    dev = am.Float64Device(n, case["restart"], am.TOL, form, mutation)
    return am.run_case(dev, case, n, form)


@pytest.mark.parametrize("case", am.CASES, ids=[c["name"] for c in am.CASES])
def test_float64_meets_every_bound(case):
    rep = _run(case)
    print(case["name"], "worst %.3g" % rep.worst(), {k: "%.2g" % v for k, v in rep.items() if v > 0.25}, rep.stats)
    assert rep.ok(), ({k: v for k, v in rep.items() if v > 1.0}, rep.stats)
    assert rep.stats.straddle == 0 or rep.stats.straddle * 10 ** 6 < rep.stats.total
    if case["frozen"]:
        assert rep.inert >= 3, rep.inert


def test_case_list_covers_the_issue():
    """Every (switch, width) on the two small operators, one and three groups, both k_g sets, the default restart."""
    names = {c["name"] for c in am.CASES}
    assert len(names) == len(am.CASES)
    for op in ("th3", "th4"):
        assert {(c["switch"], c["m"]) for c in am.CASES if c["op"] == op} >= set(am.COMBOS)
    assert {c["ks"] for c in am.CASES if c["ng"] == 3} == {am.KS_A, am.KS_B}
    assert any(c["restart"] == 30 and c["op"] == "cfg1" for c in am.CASES)
    assert sorted({am.N_ROWS[c["op"]] % 64 for c in am.CASES}) == [1, 17, 58]


# which case shows which fault: three groups with early leavers for the back substitution, the frozen scenario for
# the |g_j| half of the rule, the one-reduction form for the parity of the pending column
THREE = dict(am._case("th4", "cgs2", 16, ng=3, leave=am.LEAVE_B, ks=am.KS_B))
UNFUSED = dict(am._case("th4", "default", 8))
KEPT = dict(am._case("th4", "fuseh0", 16))           # separate Hessenberg kernel, w kept
LOWSYNC = dict(am._case("th4", "default", 16, ng=3, leave=am.LEAVE_B, ks=am.KS_B))
FROZEN3 = dict(am._case("th4", "cgs2", 16, frozen=True))
FROZENL = dict(am._case("th4", "default", 16, frozen=True))
FAULTS = [("drop_last_vector", THREE, "h1"), ("drop_last_vector", UNFUSED, "h1"),
          ("swap_cs_sn", THREE, "H column"), ("swap_cs_sn", LOWSYNC, "completed H column"),
          ("h1_only", THREE, "H column"), ("h1_only", UNFUSED, "H column"), ("h1_only", KEPT, "H column"),
          ("skip_second_pass", KEPT, "scale"),
          ("skip_second_pass", THREE, "H column"), ("skip_second_pass", UNFUSED, "scale"),
          ("rotation_wrong_pair", THREE, "H column"), ("rotation_wrong_pair", LOWSYNC, "completed H column"),
          ("stale_parity", LOWSYNC, "completed H column"),
          ("backsolve_extra_column", THREE, "back substitution"),
          ("backsolve_extra_column", LOWSYNC, "back substitution"),
          ("ignore_g_frozen", FROZEN3, "H column"), ("ignore_g_frozen", FROZENL, "completed H column")]


@pytest.mark.parametrize("mutation,case,quantity", FAULTS, ids=["%s-%s" % (m, c["name"]) for m, c, _ in FAULTS])
def test_fault_misses_its_bound(mutation, case, quantity):
    clean = _run(case)
    assert clean.ok()
    rep = _run(case, mutation)
    print(mutation, case["name"], {k: "%.3g" % v for k, v in rep.items() if v > 1.0}, rep.stats)
    assert rep.get(quantity, 0.0) > 1.0, (quantity, rep.get(quantity))
    assert not rep.ok()


def test_every_mutation_is_exercised():
    assert {m for m, _, _ in FAULTS} == set(am.MUTATIONS)


def test_stored_vector_rule():
    """check_stored: exact where the interval holds no boundary; a neighbour one unit away only where it straddles one;
    RN16(RN32(x)) accepted beside RN16(x) for the FP16 basis."""
    f16 = am.nominal_form("default", 8)
    x = np.array([[0.1, 0.2503, 1.0 + 2.0 ** -11]])
    st = am.StoreStats()
    assert am.check_stored(am.to_fp16(x), x, np.zeros_like(x), f16, st) == 0.0 and st.straddle == 0
    up = am.to_fp16(x) + np.array([[2.0 ** -14, 0.0, 0.0]])
    st = am.StoreStats()
    assert am.check_stored(up, x, 1e-17 * np.ones_like(x), f16, st) == np.inf and st.bad == 1
    # a value half a unit above a boundary of FP32 rounds down through FP32 and up directly
    y = np.array([[1.0 + 2.0 ** -11 + 2.0 ** -30]])
    assert am.to_fp16(y)[0, 0] != am.to_fp16(am.to_fp32(y))[0, 0]
    for held in (am.to_fp16(y), am.to_fp16(am.to_fp32(y))):
        st = am.StoreStats()
        assert am.check_stored(held, y, np.zeros_like(y), f16, st) == 0.0 and st.straddle == 0
        assert st.direct + st.via32 == 1
    # the tie itself is a boundary: with a bound either neighbour is accepted, counted as straddling
    z = np.array([[1.0 + 2.0 ** -11]])
    st = am.StoreStats()
    assert am.check_stored(np.array([[1.0 + 2.0 ** -10]]), z, 1e-16 * np.ones_like(z), f16, st) == 0.0
    assert st.straddle == 1 and st.far == 0 and not st.ok()
