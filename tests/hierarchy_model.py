"""FP64 SciPy model of the cycle of a deep hierarchy (``ricadi_opts::hierarchy = 1``), composed
level by level from the existing one-level models: ``precond_model.CycleModel`` (SIMPLE sweep; always level 0) and
``vanka_model.VankaModel`` (a child level with the coloured Vanka sweep).  A level's coarse stage is its child's whole
cycle -- one visit per level, a V-cycle -- and the last level applies the dense inverse of its coarse matrix; a Vanka
child that has a child itself takes its coarse correction through it first and sweeps after.

The inputs are ``Context.precond_structure``-shaped dicts, one per level (and per level the dict of
``Context.precond_vanka`` / ``_lib.host_vanka_patches`` or None): from a device context (``from_context``), or built
on the host from the rows of ``_lib.host_plan_hierarchy`` with the library's own aggregation (``host_structures``).
"""
import numpy as np
import scipy.sparse as sps

from optconpy_amd import _lib
import precond_model as pm
import vanka_model as vm


# coarse_max that forces exactly 3 / 4 levels under hierarchy = 1 with the base aggregates (16, 24) on the Taylor-Hood
# cavity of optconpy_amd.problems (nu = 0.05) at N = 15 / 30: the coarse dimensions are 120 -> 68 -> 42 -> 28 and
# 484 -> 264 -> 156 -> 102 -> 53 -> 29 (the pressure is coarsened as well from the fifth level on), the cap of a child chain is coarse_max * 9 / 8 (tests/test_hierarchy_cpu.py
# asserts the level counts)
COARSE_MAX = {15: {3: 60, 4: 30}, 30: {3: 150, 4: 100}}


def _labels(pattern, size):
    blk, _ = _lib.host_aggregate(sps.csr_matrix(pattern), size)
    return np.asarray(blk)


def host_structures(calA, calE, J, plan, bs=32):
    """One plain-aggregation structure per row of ``plan`` (``_lib.host_plan_hierarchy``), with the operators of every
    level: velocity aggregates of the plan's size on the graph of cal E (the union pattern where cal E is not
    mass-like), pressure aggregates on J J^T, 32-row blocks by the same greedy rule.  Returns (structures, operators)."""
    sts, ops = [], []
    A, E, Jl = sps.csr_matrix(calA), sps.csr_matrix(calE), sps.csr_matrix(J)
    for row in plan:
        nv = A.shape[0]
        union = abs(A) + abs(E)
        graph = E if E.nnz > 2 * nv else union
        pgraph = abs(Jl) @ abs(Jl).T
        st = pm.plain_structure(A, E, Jl, _labels(union, bs), _labels(pgraph, bs), _labels(graph, row["agg_v"]),
                                _labels(pgraph, row["agg_p"]), bs=bs)
        st["child"] = bool(row["has_child"])
        sts.append(st)
        ops.append((A, E, Jl))
        if row["has_child"]:
            A, E, Jl = vm.child_operators(st, A, E, Jl)
    return sts, ops


def compose(calA, calE, J, structures, patches=None, omega=0.7):
    """The model of level 0 over the models of all levels below it.  ``patches[l]``: the Vanka records of level l
    (None, or a dict without pressure patches: the level smooths with the SIMPLE sweep)."""
    patches = patches or [None] * len(structures)
    ops = [(sps.csr_matrix(calA), sps.csr_matrix(calE), sps.csr_matrix(J))]
    for st in structures[:-1]:
        assert st["child"], "a level above the last one must hand its coarse problem to a child"
        ops.append(vm.child_operators(st, *ops[-1]))
    assert not structures[-1]["child"]
    model = None
    for l in range(len(structures) - 1, -1, -1):
        vp = patches[l]
        if l > 0 and vp is not None and vp["pressure_patches"] > 0:
            model = vm.VankaModel(*ops[l], structures[l], vp, omega, child=model)
        else:
            model = pm.CycleModel(*ops[l], structures[l], child=model)
    return model


def from_context(ctx, calA, calE, J, omega=0.7):
    """Model of a device context's whole hierarchy, from the structure and the patches the device reports."""
    sts = [ctx.precond_structure(0)]
    while sts[-1]["child"]:
        sts.append(ctx.precond_structure(len(sts)))
    return compose(calA, calE, J, sts, [None] + [ctx.precond_vanka(l) for l in range(1, len(sts))], omega), sts


def chain(model):
    """The models of all levels, top down."""
    out = [model]
    while out[-1].child is not None:
        out.append(out[-1].child)
    return out
