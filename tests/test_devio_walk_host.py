"""The device I/O walk harness (tests/apiwalk.py's devio_* and the lists of
tests/test_gpu_devio_walk.py), on the oracle alone: no GPU.

a. every new list and walk is legal and finite on the oracle: no abort(), and
   after every step no stored value of phi, rhs, old or res is NaN or Inf or
   reaches 1e12 in magnitude; the oracle's half of every device I/O kind is
   driven, and numpy's statement of every get is formed (its count is the
   number of output elements that differ from what the output started as);
b. across the seeds every device I/O kind occurs at least once per tree class,
   and at least every third step of a walk is a cycle;
c. the harness is sharp, oracle against oracle: one flipped mantissa bit of a
   face ghost of phi changes what a face-centred get_boxes_grad /
   get_boxes_flux without a fill must return, in one element; a put made on
   one side only fails the comparison after it and names the level and the
   variable; a put changes exactly as many cells as the plan-only context
   (OMG_DEVICE_NONE) returns for the same call;
d. the walks that existed before the device I/O kinds are unchanged: A.walk
   for WALK_TREES x WALK_SEEDS against tests/golden/api_walks.json, generated
   before DEVIO_KINDS was added."""
import json
import os

import numpy as np
import pytest

from tests import apiwalk as A
from tests import denseutil as U
from tests import test_gpu_devio_walk as G
from tests.apiwalk import C4, RING, TREES, V0, V1
from tests.mgdriver import OracleBackend, parse, setup_problem

LIMIT = 1e12
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_walks.json")


def _oracle(args, n_ranks=1):
    orc = OracleBackend(parse(args), n_ranks)
    setup_problem(orc)
    A.devio_setup(orc)
    return orc


def _checked_step(orc, meth, n, step, steps):
    rec = {}
    r = A.apply_step(orc, meth, step, rec=rec)
    assert r is None or np.isfinite(r), (n, step, r)
    if step[0] in A.DEVIO_KINDS and step[0] not in A.DEVIO_PUTS:
        base, want, count = A.devio_expected(orc, step, rec)
        comps = 1 if step[0] in ("get_dense", "get_boxes") else 3
        assert count > 0 and base.shape == want.shape, (n, step)
        if not (step[0] == "get_boxes_flux" and step[7]):   # (accumulating: a term of zero leaves the bits)
            assert int((want != base).sum()) == comps * count, (n, step)
        assert np.isfinite(want.view(np.float64)[want != base]).all(), (n, step)
    for iv in (1, 2, 3, 4):   # (every cell of every box; False for a NaN)
        assert orc.o.max_abs(iv) < LIMIT, (n, step, iv, steps)


def _run_checked(args, steps, n_ranks=1):
    orc = _oracle(args, n_ranks)
    meth = A.Methods(orc.cfg)
    for n, step in enumerate(steps):
        _checked_step(orc, meth, n, step, steps)


# -- a. legal and finite ---------------------------------------------------------
def _lists():
    out = []
    hi_c4 = A.tree_levels(C4)[1]
    for n, put in enumerate(G.below_boundary_puts(hi_c4)):
        out.append(pytest.param(C4, [V0, put, V1], 1, id=f"below-boundary-{n}"))
    mx2 = TREES["mx2_helm64_box16"]
    out.append(pytest.param(mx2, G.stored_bc_list(A.tree_levels(mx2)[1]), 1, id="stored-bc-mx2"))
    out.append(pytest.param(mx2, G.stored_bc_host_writers_list(A.tree_levels(mx2)[1]), 1, id="stored-bc-host-mx2"))
    out.append(pytest.param(RING, A.ring_devio_writers_list(A.tree_levels(RING)[1]), 1, id="writers-ring"))
    for tree in ("per128_box16", "ref3_gs_box8"):
        for name, steps in G.chains(parse(TREES[tree]), A.tree_levels(TREES[tree])[1]).items():
            out.append(pytest.param(TREES[tree], steps, 1, id=f"chain-{name}-{tree}"))
    for tree in sorted(TREES):
        for name, steps in sorted(G.fill_after_lists(parse(TREES[tree]), *A.tree_levels(TREES[tree])).items()):
            out.append(pytest.param(TREES[tree], steps, 1, id=f"fill-after-{name}-{tree}"))
    for name, args, ranks, parts in G.RANK_CASES:
        out.append(pytest.param(args, G.rank_fill_after_list(args), ranks, id=f"ranks-fill-after-{name}"))
    for tree in sorted(A.WALK_TREES):
        lv = A.tree_levels(A.WALK_TREES[tree])
        for seed in A.WALK_SEEDS:
            out.append(pytest.param(A.WALK_TREES[tree], A.devio_walk(tree, seed, levels=lv), 1,
                                    id=f"walk-{tree}-{seed}"))
    for name, args, ranks, parts in G.RANK_CASES:
        lo, hi = A.tree_levels(args)
        for part in range(parts):
            out.append(pytest.param(args, G.rank_list(parse(args), lo, hi, part, parts), ranks,
                                    id=f"ranks-{name}-{part}"))
    return out


@pytest.mark.parametrize("tree", sorted(TREES))
def test_each_device_io_kind_after_two_cycles_is_legal_and_finite(tree):
    lo, hi = A.tree_levels(TREES[tree])
    kinds = A.devio_directed_kinds(parse(TREES[tree]), lo, hi)
    assert {k[0] for k in kinds} == set(A.DEVIO_KINDS)
    for k in kinds:
        _run_checked(TREES[tree], [V0, V0, k, V1])


@pytest.mark.parametrize("args,steps,n_ranks", _lists())
def test_list_is_legal_and_finite_on_the_oracle(args, steps, n_ranks):
    _run_checked(args, steps, n_ranks)


def test_directed_kinds_cover_the_argument_space():
    """What the issue of the device I/O walk lists: variables, centrings,
    scales, fill, coefficient, accumulate, block lists and windows."""
    for tree in sorted(TREES):
        cfg = parse(TREES[tree])
        ks = A.devio_directed_kinds(cfg, *A.tree_levels(TREES[tree]))
        by = {kind: [k for k in ks if k[0] == kind] for kind in A.DEVIO_KINDS}
        for kind in ("get_dense", "get_dense_grad", "get_boxes", "get_boxes_grad", "get_boxes_flux"):
            assert {k[2] for k in by[kind]} == {1, 2, 4}, kind
        for kind in A.DEVIO_PUTS:
            assert {k[2] for k in by[kind]} == {1, 2}, kind
        for kind in ("get_boxes_grad", "get_boxes_flux"):
            assert {k[3] for k in by[kind]} == {"cell", "face"} and {k[4] for k in by[kind]} == {1.0, -1.0, 0.37}
            assert {k[5] for k in by[kind]} == {False, True}
        assert {k[4] for k in by["get_dense_grad"]} == {1.0, -1.0, 0.37}
        assert {k[5] for k in by["get_dense_grad"]} == {False, True}
        assert {k[4] for k in by["get_boxes"]} == {False, True} and {k[3] for k in by["get_boxes"]} == {False, True}
        assert {k[6] for k in by["get_boxes_flux"]} == {0, A.I_COEF} and {k[7] for k in by["get_boxes_flux"]} == {False, True}
        assert {k[3] for k in by["put_boxes_div"]} == {"cell", "face"}
        assert {k[3] for k in by["put_dense"] + by["get_dense"] + by["get_dense_grad"]} == {"whole", "cut"}
        sels = {k[1][0] for kind in A.DEVIO_KINDS[3:] for k in by[kind]}
        assert sels == ({"perm", "subset", "leaves"} if cfg["n_levels"] > 1 else {"perm", "subset"})


def test_block_lists_are_what_their_names_say():
    for tree in sorted(A.WALK_TREES):
        t = U.host_tree(A.WALK_TREES[tree])
        lo, hi = t.lowest_lvl, t.highest_lvl
        all_hi = [int(i) for i in t.lvls[hi].ids]
        perm, sub = A.devio_ids(t, ("perm", hi, 1)), A.devio_ids(t, ("subset", hi, 2))
        assert sorted(perm) == sorted(all_hi) and perm != all_hi
        assert 0 < len(sub) < len(all_hi) and set(sub) < set(all_hi)
        low = A.devio_ids(t, ("perm", lo + 2, 4))
        assert lo + 2 <= 0 and t.box_size_lvl[lo + 2] == 8 and len(low) == len(t.lvls[lo + 2].ids)
        if t.highest_lvl > 1:
            leaves = A.devio_ids(t, ("leaves",))
            assert {int(t.lvl[i]) for i in leaves} == set(range(1, hi + 1))
            assert len(leaves) == sum(len(t.lvls[l].leaves) for l in range(1, hi + 1))
    t = U.host_tree(RING)
    slab = A.devio_ids(t, ("slab", t.highest_lvl))
    assert len(slab) == 8 * 16   # (one z-slab of the 8 x 16 x 16 boxes)


# -- b. reach ----------------------------------------------------------------------
def test_walks_reach_every_device_io_kind_of_every_tree_class():
    seen = {}
    for tree in sorted(A.WALK_TREES):
        cfg = parse(A.WALK_TREES[tree])
        lo, hi = lv = A.tree_levels(A.WALK_TREES[tree])
        for seed in A.WALK_SEEDS:
            steps = A.devio_walk(tree, seed, levels=lv)
            assert len(steps) == A.walk_steps(tree)
            assert steps == A.devio_walk(tree, seed, levels=lv)
            for g in range(0, len(steps), 3):
                assert any(A.is_cycle(s) for s in steps[g:g + 3]), steps
            seen.setdefault(A.tree_class(cfg), set()).update(s[0] for s in steps)
            for s in steps:
                assert s[0] in A.DEVIO_KINDS + A.NEW_KINDS + ["vcycle"], s
                if s[0] in A.DEVIO_KINDS[:3]:
                    assert lo <= s[1] <= hi, s
                elif s[0] in A.DEVIO_KINDS and s[1][0] != "leaves":
                    assert lo <= s[1][1] <= hi, s
    assert set(seen) == {"per", "ref", "phys"}
    for cls, kinds in seen.items():
        missing = set(A.DEVIO_KINDS) - kinds
        assert not missing, (cls, missing)


# -- c. the harness is sharp -----------------------------------------------------
@pytest.fixture(scope="module")
def two_oracles():
    pair = []
    for _ in range(2):
        orc = _oracle(TREES["ref3_gs_box8"])
        orc.vcycle(True)
        pair.append(orc)
    A._assert_same(pair[0], pair[1], "unchanged")
    return pair


def _flip(orc, lvl, iv, box, cell, bit=0):
    """Flip one mantissa bit of one cell; returns the undo."""
    a = orc.get_level(lvl, iv)
    keep = a.copy()
    k, j, i = cell
    a[box:box + 1, k, j, i].view(np.uint64)[...] ^= np.uint64(1 << bit)
    assert a[box, k, j, i] != keep[box, k, j, i]
    orc.set_level(lvl, iv, a)
    return lambda: orc.set_level(lvl, iv, keep)


FACE_GETS = [("get_boxes_grad", ("perm", 3, 1), 1, "face", 1.0, False),
             ("get_boxes_flux", ("perm", 3, 1), 1, "face", -1.0, False, A.I_COEF, False),
             ("get_boxes_flux", ("subset", 3, 1), 1, "face", 0.37, False, 0, True)]


@pytest.mark.parametrize("step", FACE_GETS, ids=["grad", "flux", "flux-accumulating"])
def test_one_flipped_bit_of_a_face_ghost_changes_the_expected_output(two_oracles, step):
    """The ghost below the box in x is read by the face 0 of the x component
    and by nothing else of a face-centred gradient."""
    a, b = two_oracles
    box = A._rows(b, 3, A.devio_ids(b.tree, step[1])[:1])[0]
    undo = _flip(b, 3, 1, box, (4, 5, 0), bit=20)
    try:
        got = []
        for orc in (a, b):
            rec = {}
            A.devio_oracle(orc, step, rec)
            got.append(A.devio_expected(orc, step, rec))
    finally:
        undo()
    (base_a, want_a, n_a), (base_b, want_b, n_b) = got
    assert n_a == n_b and np.array_equal(base_a, base_b)
    diff = np.argwhere(want_a != want_b)
    assert diff.tolist() == [[0, 0, 4, 5, 0]], diff   # (component x, the first box listed, its face 0)
    A._assert_same(a, b, "restored")


PUTS = [("put_dense", 2, 1, "cut"), ("put_dense", 3, 2, "whole"), ("put_boxes", ("subset", 2, 5), 1, False),
        ("put_boxes", ("leaves",), 2, True), ("put_boxes", ("perm", -1, 3), 1, True),
        ("put_boxes_div", ("perm", 1, 7), 2, "cell", -1.0), ("put_boxes_div", ("leaves",), 1, "face", 0.37)]


def _plan_count(tree, ctx, step):
    """What the plan-only context returns for the put (no device: the pointer
    is never dereferenced)."""
    ptr = 4096
    if step[0] == "put_dense":
        lo, n = A.devio_window(tree, step[1], step[3])
        return ctx.put_dense(step[1], step[2], ptr, lo, n, U.contiguous(n))
    ids = A.devio_ids(tree, step[1])
    m = tree.box_size_lvl[int(tree.lvl[ids[0]])] + 2
    off = np.arange(len(ids), dtype=np.int64) * m ** 3 + (1 + m + m * m)
    if step[0] == "put_boxes":
        return ctx.put_boxes(step[2], ids, ptr, off, (1, m, m * m), int(step[3]))
    ptrs = (ptr, ptr + (1 << 30), ptr + (2 << 30))
    return ctx.put_boxes_div(step[2], ids, ptrs, off, (1, m, m * m), step[4], int(step[3] == "face"))


@pytest.fixture(scope="module")
def plan():
    tree = U.host_tree(TREES["ref3_gs_box8"])
    ctx = U.plan_context(tree)
    yield tree, ctx
    ctx.close()


@pytest.mark.parametrize("step", PUTS, ids=[f"{s[0]}-{n}" for n, s in enumerate(PUTS)])
def test_a_put_on_one_side_only_fails_and_changes_the_plans_count_of_cells(two_oracles, plan, step):
    a, b = two_oracles
    meth = A.Methods(a.cfg)
    iv = step[2]
    before = {lvl: a.get_level(lvl, iv) for lvl in a.levels()}
    A.apply_step(a, meth, step, rec={})
    changed = {lvl: int((a.get_level(lvl, iv).view(np.uint64) != before[lvl].view(np.uint64)).sum())
               for lvl in a.levels()}
    # (half of a value plus noise differs from the value in every cell the entry defines)
    assert sum(changed.values()) == _plan_count(*plan, step) > 0, changed
    lvls = [lvl for lvl, n in changed.items() if n]
    with pytest.raises(AssertionError) as ex:
        A._assert_same(a, b, "a put on one side only")
    assert ex.value.args[0][:2] == (min(lvls), iv)
    # the same step on the other side: the same data, the same cells
    A.apply_step(b, meth, step, rec={})
    A._assert_same(a, b, "both sides")


# -- d. the walks from before the device I/O kinds ----------------------------------
def test_existing_walks_are_unchanged():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(f"{t}-{s}" for t in A.WALK_TREES for s in A.WALK_SEEDS)
    for tree in sorted(A.WALK_TREES):
        lv = A.tree_levels(A.WALK_TREES[tree])
        for seed in A.WALK_SEEDS:
            steps = json.loads(json.dumps(A.walk(tree, seed, levels=lv)))   # (tuples as lists, as the file has them)
            assert steps == golden[f"{tree}-{seed}"], (tree, seed)
