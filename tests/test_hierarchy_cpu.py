"""The fine hierarchy (``ricadi_opts::hierarchy = 1``), host side (no GPU): the rule of ``ricadi_host_plan_hierarchy``,
the default rule seen through the same entry, the new option field in the built library, and the FP64 model of a
four-level cycle (tests/hierarchy_model.py) inside a right-preconditioned GMRES.

The shapes are the Taylor-Hood cavity at N = 15 and N = 30 with ``coarse_max`` forced small: with the base aggregates
(16, 24) the coarse dimensions are 120 and 484, and a child halves the velocity part each time --
N = 15: 120 -> 68 -> 42 -> 28;  N = 30: 484 -> 264 -> 156 -> 102 -> 53 -> 29 (the pressure is coarsened as well from the fifth level on).  The cap of a child chain is
``coarse_max * 9 / 8``."""
import numpy as np
import pytest

from optconpy_amd import _lib, problems as pb
import hierarchy_model as hm
import vanka_model as vm

CM = hm.COARSE_MAX


@pytest.fixture(scope="module")
def cavity():
    out = {}
    for N in (15, 30):
        pr = pb.ricc_problem(N, 0.05)
        out[N] = (pr, (-pr.A - pr.Nc).T.tocsr(), pr.M.T.tocsr(), pr.J.tocsr())
    return out


def _check_fine_plan(plan, agg, cm):
    assert 1 <= len(plan) <= _lib.MAX_HIERARCHY_LEVELS
    assert (plan[0]["agg_v"], plan[0]["agg_p"]) == agg                      # level 0 never grows its aggregates
    cap = cm + cm // 8 if len(plan) > 1 else cm
    for up, low in zip(plan, plan[1:]):
        assert up["has_child"] and up["dense_dim"] == 0 and not up["smoothed"]   # plain aggregation above a child
        assert up["kv"] + up["kp"] > (cm if up is plan[0] else cap)         # ... which it has because it needs it
        assert (low["nv"], low["np"]) == (up["kv"], up["kp"])
    for lev in plan:
        # a coarse saddle matrix needs more velocity than pressure unknowns; the rule keeps a quarter of margin
        assert lev["kp"] == 0 or 4 * lev["kv"] >= 5 * lev["kp"], lev
    for lev in plan[1:]:
        # gentle: pairs, pressure 1 : 1 -- unless 1 : 1 would leave too few velocity aggregates beside the pressure's
        assert lev["agg_p"] == 1 or 4 * lev["kv"] < 5 * lev["np"] or lev is plan[-1], lev
    for lev in plan[1:-1]:
        assert lev["agg_v"] == 2
    last = plan[-1]
    assert not last["has_child"] and last["dense_dim"] == last["kv"] + last["kp"]
    grew = len(plan) > 1 and last["agg_v"] != 2
    # only the last level of a full chain grows its aggregates (the bottom fallback), and it stops where it fits
    assert not grew or len(plan) == _lib.MAX_HIERARCHY_LEVELS
    assert last["dense_dim"] <= max(16, cap)
    return grew


def test_fine_plan_properties(cavity):
    seen = set()
    for N, cms in ((15, (400, 100, 60, 30, 20)), (30, (4096, 300, 150, 100, 80, 30, 16))):
        pr, calA, calE, J = cavity[N]
        for cm in cms:
            plan = _lib.host_plan_hierarchy(calA, calE, J, hierarchy=1, coarse_max=cm)
            again = _lib.host_plan_hierarchy(calA, calE, J, hierarchy=1, coarse_max=cm)
            assert plan == again                                             # deterministic
            assert (plan[0]["nv"], plan[0]["np"]) == (pr.NV, pr.NP)
            grew = _check_fine_plan(plan, (16, 24), cm)
            seen.add((len(plan), grew))
            print("N = %d coarse_max = %d: %d levels, coarse dimensions %s%s" % (
                N, cm, len(plan), [r["kv"] + r["kp"] for r in plan], ", last level grown" if grew else ""))
    # the cases cover one level, every depth up to the most, and the bottom fallback
    assert {n for n, _ in seen} == set(range(1, _lib.MAX_HIERARCHY_LEVELS + 1)) and (6, True) in seen and (6, False) in seen
    # other base aggregates are kept as well
    pr, calA, calE, J = cavity[15]
    _check_fine_plan(_lib.host_plan_hierarchy(calA, calE, J, hierarchy=1, coarse_max=60, agg_v=8, agg_p=12), (8, 12), 60)


def test_forced_coarse_max_gives_three_and_four_levels(cavity):
    for N in (15, 30):
        _, calA, calE, J = cavity[N]
        for want, cm in CM[N].items():
            plan = _lib.host_plan_hierarchy(calA, calE, J, hierarchy=1, coarse_max=cm)
            assert len(plan) == want and all((r["agg_v"], r["agg_p"]) == (2, 1) for r in plan[1:]), (N, cm, plan)


def test_fine_plan_ignores_the_two_level_rule_and_max_levels(cavity):
    """A stiffness-dominated operator keeps two levels under the default rule and grows its aggregates for it; the fine
    rule sends it down a chain, whatever ``max_levels`` says."""
    _, calA, calE, J = cavity[30]
    assert _lib.host_sa_criterion(calA)[0]
    old = _lib.host_plan_hierarchy(calA, calE, J, coarse_max=150)
    assert len(old) == 1 and old[0]["agg_v"] > 16 and old[0]["smoothed"]
    for ml in (2, 3):
        assert len(_lib.host_plan_hierarchy(calA, calE, J, hierarchy=1, coarse_max=150, max_levels=ml)) == 3
    # no coarse space, no pressure: one level
    assert len(_lib.host_plan_hierarchy(calA, calE, J, hierarchy=1, use_coarse=0)) == 1
    with pytest.raises(ValueError):
        _lib.host_plan_hierarchy(calA, calE, J, hierarchy=2)


def test_default_rule_through_the_new_entry_equals_plan_levels(cavity):
    """``hierarchy = 0``: the first level is what ``ricadi_host_plan_levels`` reports (its level count includes the dense
    coarse problem), for N = 15 / 30 and for the operators of the existing plan test (N = 40, stiffness dominated and
    convection dominated)."""
    cases = [(cavity[N][1], cavity[N][2], cavity[N][3], dict(coarse_max=cm)) for N in (15, 30) for cm in (4096, 150, 60)]
    pr = pb.ricc_problem(40, 0.05)
    calE = pr.M.T.tocsr()
    cases += [((-pr.A - pr.Nc).T.tocsr(), calE, pr.J, dict(coarse_max=cm)) for cm in (4096, 400, 150, 60)]
    pc = pb.ricc_problem(40, 0.0005)
    calAc = (-pc.A - pc.Nc).T.tocsr()
    cases += [(calAc, calE, pc.J, dict(coarse_max=400)), (calAc, calE, pc.J, dict(coarse_max=400, max_levels=2)),
              (calAc, calE, pc.J, dict(use_coarse=0))]
    depths = set()
    for calA, cE, J, opts in cases:
        five = _lib.host_plan_levels(calA, cE, J, **opts)
        plan = _lib.host_plan_hierarchy(calA, cE, J, hierarchy=0, **opts)
        assert plan == _lib.host_plan_hierarchy(calA, cE, J, **opts)           # 0 is the default
        top = plan[0]
        got = dict(levels=len(plan) + (1 if top["kv"] + top["kp"] > 0 else 0), kc=top["kv"] + top["kp"], kcv=top["kv"],
                   kcp=top["kp"], smoothed=top["smoothed"])
        assert got == five, (opts, got, five)
        assert len(plan) <= 2 and bool(top["has_child"]) == (five["levels"] == 3)
        if len(plan) == 2:
            assert (plan[1]["nv"], plan[1]["np"]) == (five["kcv"], five["kcp"]) and not plan[1]["has_child"]
            assert plan[1]["dense_dim"] <= opts["coarse_max"] * 9 // 8
        depths.add(five["levels"])
    assert depths == {1, 2, 3}


def test_option_field_in_the_built_library():
    lib = _lib.load()
    o = _lib.default_opts()
    assert o.hierarchy == 0 and _lib.default_opts(hierarchy=1).hierarchy == 1
    names = [f for f, _ in _lib.RicadiOpts._fields_]
    sig = dict(part.split(":") for part in lib.ricadi_struct_signature().decode().split(";"))["ricadi_opts"]
    assert "hierarchy" in names and len(sig) == len(names) and sig[names.index("hierarchy")] == "i"
    import ctypes as C
    assert lib.ricadi_sizeof_opts() == C.sizeof(_lib.RicadiOpts) and lib.ricadi_version() == _lib.ABI_VERSION >= 403
    assert "ricadi_host_plan_hierarchy" in _lib.SIGNATURES and hasattr(lib, "ricadi_host_plan_hierarchy")
    # the field sits where the library reads it: the plan follows it
    pr = pb.ricc_problem(15, 0.05)
    ops = ((-pr.A - pr.Nc).T.tocsr(), pr.M.T.tocsr(), pr.J)
    assert len(_lib.host_plan_hierarchy(*ops, coarse_max=60, hierarchy=1)) == 3
    assert len(_lib.host_plan_hierarchy(*ops, coarse_max=60)) == 1


@pytest.mark.parametrize("smoother", [0, 1])
def test_four_level_model_converges(cavity, smoother):
    """FP64 GMRES on the N = 15 saddle system, preconditioned by the model of the four-level V-cycle (SIMPLE or coloured
    Vanka children), to 1e-10 at p = -1 and p = -30."""
    pr, calA, calE, J = cavity[15]
    plan = _lib.host_plan_hierarchy(calA, calE, J, hierarchy=1, coarse_max=CM[15][4])
    sts, ops = hm.host_structures(calA, calE, J, plan)
    # the library's aggregation reproduces the plan's sizes level by level
    assert [(s["nv"], s["np"], s["kcv"], s["kcp"]) for s in sts] == [(r["nv"], r["np"], r["kv"], r["kp"]) for r in plan]
    patches = [None] + [_lib.host_vanka_patches(o[0].shape[0], o[2]) if smoother else None for o in ops[1:]]
    model = hm.compose(calA, calE, J, sts, patches)
    levels = hm.chain(model)
    assert len(levels) == 4 and all(isinstance(l, vm.VankaModel) == bool(smoother) for l in levels[1:])
    b = np.r_[np.random.default_rng(1).standard_normal(pr.NV), np.zeros(pr.NP)]
    cap = 300
    for p in (-1.0, -30.0):
        S = model.saddle(p, 1.0)
        x, its, res = vm.gmres_right(S, lambda r: model.apply(p, 1.0, r), b, maxit=cap)
        print("four-level model, child smoother %d, p = %g: %d iterations" % (smoother, p, its))
        assert res <= 1e-10 and its < cap, (p, its, res)
        assert np.linalg.norm(S @ x - b) <= 1e-8 * np.linalg.norm(b)
