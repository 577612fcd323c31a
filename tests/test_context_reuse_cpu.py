"""The host half of tests/test_gpu_context_reuse.py: the sequences contain the flips they are named for, the header
states the contract of an operator replacement, the control table is well formed, and the source keeps the order of
the ``has_op`` writes.  No GPU.

Flips asserted from the host entries (``small_ops.SmallOp.host_structure``, ``_lib.host_saddle_tiles``,
``_lib.host_plan_levels`` / ``host_plan_hierarchy``): np zero / non-zero, nv strictly growing and shrinking, ``ms_ok``
and ``smoothed`` taking both values, a coarse space and none, one and several velocity blocks, levels 3 and 2.

Flips the host entries cannot show, listed and not asserted here:

* ``sb_ok``: every operator of the family fits the tile format (``host_saddle_tiles`` reports True for all 27);
* ``rect`` and ``folded``: decided on the device side of the setup (``cycle_form``); the GPU file asserts ``folded``
  from ``precond_structure`` in the sequence ``pressure`` and prints ``rect`` with the facts of every sequence.
"""
import os
import re

import context_battery as cb
import small_ops as so
import test_gpu_context_reuse as gpu_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _facts(name):
    opts, keys = cb.SEQUENCES[name]
    return [cb.host_facts(k, opts) for k in keys]


def test_sequences_contain_their_flips():
    f = _facts("grow")
    nv = [x["nv"] for x in f]
    assert nv == sorted(set(nv)) and f[0]["np"] == 0 and all(x["np"] > 0 for x in f[1:])
    assert {x["ms_ok"] for x in f} == {True, False} and {x["kc"] > 0 for x in f} == {True, False}
    assert {x["nbv"] > 1 for x in f} == {True, False}
    f = _facts("shrink")
    nv = [x["nv"] for x in f]
    assert nv == sorted(set(nv), reverse=True) and nv[-1] == 1 and f[-1]["np"] == 0
    assert all(x["np"] > 0 for x in f[:-1]) and {x["ms_ok"] for x in f} == {True, False}
    f = _facts("pressure")
    assert [x["np"] > 0 for x in f] == [True, False, True]
    f = _facts("values")
    assert [x["smoothed"] for x in f] == [False, False, False, True, True]
    assert len({(x["nv"], x["np"]) for x in f[:3]}) == 1 and len({(x["nv"], x["np"]) for x in f[3:]}) == 1
    for name in ("hierarchy", "hierarchy_vanka"):
        assert [x["levels"] for x in _facts(name)] == [3, 2, 3]
    f = _facts("dims")
    assert [x["dims"] for x in f] == [False, True, False, True, False] and [x["nv"] for x in f] == [33, 50, 33, 33, 65]
    for name, bs in (("block16", 16), ("block64", 64)):
        opts, keys = cb.SEQUENCES[name]
        assert opts == dict(bj_block=bs) and all(so.FAMILY[k][2] == opts for k in keys)
        nv = [x["nv"] for x in _facts(name)]
        assert nv[0] < nv[1] > nv[2] and {x["kc"] > 0 for x in _facts(name)} == {True, False}
    # every operator of the family with that option is in its sequence
    for bs in (16, 64):
        assert {k for k, v in so.FAMILY.items() if v[2].get("bj_block") == bs} == set(cb.SEQUENCES["block%d" % bs][1])
    assert all(cb.host_facts(k, {})["sb_ok"] for k in so.NAMES if not so.FAMILY[k][2])      # (the docstring's claim)


def test_same_pattern_other_values():
    """``values``: the transpose keeps J, sizes and the symmetric part; the scaled operator keeps the pattern."""
    a, t = cb.get_op("unsym"), cb.get_op("unsym_T")
    assert abs(a.calA - t.calA.T).nnz == 0 and abs(a.J - t.J).nnz == 0 and abs(a.calA - t.calA).nnz > 0
    g, s = cb.get_op("stiff_grid"), cb.get_op("stiff_grid_x3")
    assert (g.calA.indices == s.calA.indices).all() and abs(3.0 * g.calA - s.calA).nnz == 0
    assert abs(g.calE - s.calE).nnz == 0 and abs(g.J - s.J).nnz == 0


def test_deepest_smallest_hierarchy():
    """``fe6`` at ``coarse_max=16`` is the smallest ``ricc_problem(N, 0.05)`` with a child level."""
    from optconpy_amd import _lib
    for N in range(2, 6):
        assert len(_lib.host_plan_hierarchy(*so.finite_element(N), hierarchy=1, coarse_max=1)) == 1, N
    assert len(_lib.host_plan_hierarchy(*cb.get_op("fe6").ops, **cb.HIERARCHY)) == 2
    assert len(_lib.host_plan_hierarchy(*cb.get_op("fe3").ops, **cb.HIERARCHY)) == 1


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "ricadi.h")).read()
    flat = re.sub(r"[\s*]+", " ", hdr)
    at_set_operator = flat[:flat.index("int ricadi_set_operator(")]
    for sentence in ("A replacement forgets everything tied to the resident operator",
                     "A replacement keeps the settings",
                     "after a replacement the context computes what a fresh context with the same options computes",
                     "A replacement refused during validation leaves the old operator intact",
                     "A replacement that fails after it began leaves no operator",
                     'refuses with "set the operator first"'):
        assert sentence in at_set_operator, sentence
    between = flat[flat.index("int ricadi_set_operator("):flat.index("int ricadi_set_dims(")]
    assert "ricadi_clear_cache forgets the per-shift data and the recycled right-hand sides" in between
    assert "ricadi_set_dims forgets exactly what ricadi_set_operator forgets" in between
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "what a context remembers" in design.lower()


def test_control_table_is_well_formed():
    names = cb.names()
    assert len(names) == len(set(names))
    for k, (cause, applies) in gpu_file.CONTROL_TABLE.items():
        assert k in names, k
        assert not k.startswith(cb.BITWISE_FAMILIES), k
        assert k in cb.BOUNDS, k
        assert "gemm_tn_kernel" in cause or "rocSOLVER" in cause, (k, cause)
        assert callable(applies)
    # the entries read from the code apply only where their cause does: on the small operators the recycled solves, the
    # sweep-form ADI and the gain must be bitwise (this is what guards the ring's slot order on the GPU)
    small, large = cb.get_op("nv33_np1"), cb.get_op("arrow200")
    for k in ("shift_solve.recycle.X16", "lyap_adi.sweep.Z", "lyap_adi.sweep.info", "resident.gain"):
        assert not gpu_file.allowed(k, small, {}) and gpu_file.allowed(k, large, {}), k
    assert not any(k.startswith("lyap_adi.step.") for k in gpu_file.CONTROL_TABLE)
    assert all(k in names and k in cb.BOUNDS for k in gpu_file.RING_KEPT)
    # each of the four families exists in the battery
    for fam in cb.BITWISE_FAMILIES:
        assert any(n.startswith(fam) for n in names), fam
    # every sequence has its flips and its positions are operators the battery can build
    assert set(gpu_file.FLIPS) == set(cb.SEQUENCES)
    for opts, keys in cb.SEQUENCES.values():
        for k in keys:
            assert isinstance(k, tuple) or cb.get_op(k).nv > 0


def _body(src, head):
    """The body of the function whose definition starts with ``head`` (to the closing brace in column 0)."""
    i = src.index(head)
    return src[i:src.index("\n}\n", i)]


def test_source_order_of_the_has_op_writes():
    """The CPU-visible half of the failed-replacement contract, from the source of ``ricadi_set_operator``: the
    validation (the column checks, the checked host setup) comes before the helper that forgets the old operator; the
    helper clears ``has_op``; the child level and the uploads follow; ``has_op = true`` is written once, after them, as
    the last statement.  ``ricadi_set_dims`` forgets through the same helper."""
    capi = open(os.path.join(ROOT, "optconpy_amd", "csrc", "solver_capi.inl")).read()
    assert "c->has_op = false;" in _body(capi, "static void forget_operator(ricadi_ctx* c) {")
    body = _body(capi, "int ricadi_set_operator(ricadi_ctx* c, int nv, int np,")
    assert body.count("c->has_op = true;") == 1 and "c->has_op = false;" not in body
    order = [body.index(x) for x in ("column index out of range", "build_setup_checked(", "forget_operator(c);",
                                     "ricadi_set_operator(ch.get()", ".upload(", "c->has_op = true;")]
    assert order == sorted(order), order
    tail = [ln.strip() for ln in body[order[-1]:].splitlines() if ln.strip()]
    assert tail == ["c->has_op = true;", "API_END"], tail
    assert "forget_operator(c);" in _body(capi, "int ricadi_set_dims(ricadi_ctx* c, int nv) {")
