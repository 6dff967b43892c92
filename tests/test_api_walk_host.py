"""The walk harness itself (tests/apiwalk.py), on the oracle alone: no GPU.

a. every list and walk of tests/test_gpu_api_walk.py is legal and finite on
   the oracle: no abort(), and after every step no stored value of phi, rhs,
   old or res is NaN or Inf or reaches 1e12 in magnitude;
b. across the seeds of the walks every kind occurs at least once per tree
   class (periodic, refined, physical faces) on which it is allowed, and at
   least every third step of a walk is a cycle;
c. the comparison is sharp: one flipped mantissa bit of a face ghost, or of an
   interior cell of `old` on a coarse level, fails it and names the level and
   the variable; a flipped edge or corner ghost does not (unstored cells)."""
import numpy as np
import pytest

from tests import apiwalk as A
from tests import test_gpu_api_walk as G
from tests.apiwalk import PER128, RING, TREES, V0, V1
from tests.mgdriver import OracleBackend, parse, setup_problem

LIMIT = 1e12


def _run_checked(args, steps, n_ranks=1):
    cfg = parse(args)
    orc = OracleBackend(cfg, n_ranks)
    setup_problem(orc)
    meth = A.Methods(cfg)
    for n, step in enumerate(steps):
        r = A.apply_step(orc, meth, step)
        assert r is None or np.isfinite(r), (n, step, r)
        for iv in (1, 2, 3, 4):   # (every cell of every box; False for a NaN)
            assert orc.o.max_abs(iv) < LIMIT, (n, step, iv, steps)


def _lists():
    out = []
    out.append(pytest.param(PER128, [V0, V0, ("subtract_mean", 1, 0), ("residual_lvl", 1), V1, V0, V0,
                                     ("subtract_mean", 1, 1), ("residual_lvl", 1), V1], 1, id="subtract-mean-phi"))
    out.append(pytest.param(PER128, [V0, V0, ("bc", 3, A.T.MG_BC_DIRICHLET, 0.375), V1], 1, id="set-bc-per128"))
    for name, args, _ in G.PARTIAL[1:]:
        lo, hi = A.tree_levels(args)
        for want in (False, True):
            for sa in (False, True):
                steps = []
                for k in range(lo, hi + 1):
                    steps += [V0, ("vcycle_to", k, want, sa)]
                out.append(pytest.param(args, steps + [V1], 1, id=f"cycle-to-{name}-{want}-{sa}"))
    out.append(pytest.param(PER128, A.METHODS_LIST, 1, id="methods-per128"))
    out.append(pytest.param(RING, A.ring_methods_list(), 1, id="methods-ring"))
    out.append(pytest.param(RING, A.ring_writers_list(A.tree_levels(RING)[1]), 1, id="writers-ring"))
    for tree in sorted(A.WALK_TREES):
        lv = A.tree_levels(A.WALK_TREES[tree])
        for seed in A.WALK_SEEDS:
            out.append(pytest.param(A.WALK_TREES[tree], A.walk(tree, seed, levels=lv), 1, id=f"walk-{tree}-{seed}"))
    for name, args, ranks, rep, switch, parts in G.RANK_CASES:
        if switch:   # (the same lists as without it)
            continue
        lo, hi = A.tree_levels(args)
        for part in range(parts):
            out.append(pytest.param(args, G._rank_list(parse(args), lo, hi, part, parts), ranks,
                                    id=f"ranks-{name}-{part}"))
        out.append(pytest.param(args, A.walk(G.RANK_TREE[args], A.WALK_SEEDS[0], n_steps=8, levels=(lo, hi)), ranks,
                                id=f"ranks-walk-{name}"))
    return out


@pytest.mark.parametrize("tree", sorted(TREES))
def test_each_entry_after_two_cycles_is_legal_and_finite(tree):
    lo, hi = A.tree_levels(TREES[tree])
    for k in A.directed_kinds(parse(TREES[tree]), lo, hi):
        _run_checked(TREES[tree], [V0, V0, k, V1])


@pytest.mark.parametrize("args,steps,n_ranks", _lists())
def test_list_is_legal_and_finite_on_the_oracle(args, steps, n_ranks):
    _run_checked(args, steps, n_ranks)


def test_walks_reach_every_kind_of_every_tree_class():
    seen = {}
    for tree in sorted(A.WALK_TREES):
        cfg = parse(A.WALK_TREES[tree])
        lv = A.tree_levels(A.WALK_TREES[tree])
        for seed in A.WALK_SEEDS:
            steps = A.walk(tree, seed, levels=lv)
            assert len(steps) == A.walk_steps(tree)
            for g in range(0, len(steps), 3):
                assert any(A.is_cycle(s) for s in steps[g:g + 3]), steps
            seen.setdefault(A.tree_class(cfg), set()).update(s[0] for s in steps)
            lo, hi = lv
            for s in steps:   # legal: what the oracle would abort() on
                if s[0] == "prolong" or s[0] == "correct_children":
                    assert lo <= s[1] < hi, s
                if s[0] == "restrict_lvl":
                    assert lo < s[2] <= hi, s
                if s[0] == "update_coarse":
                    assert lo < s[1] <= hi, s
                if s[0] in ("bc", "phi_bc_store"):
                    assert cfg["bc"] != "per", s
            assert sum(s[0] == "phi_bc_store" for s in steps) <= 1
    assert set(seen) == {"per", "ref", "phys"}
    for cls, kinds in seen.items():
        missing = set(A.allowed_kinds(cls)) - kinds
        assert not missing, (cls, missing)


# -- c. the comparison is sharp -------------------------------------------------
@pytest.fixture(scope="module")
def two_oracles():
    cfg = parse(TREES["ref3_gs_box8"])
    pair = []
    for _ in range(2):
        orc = OracleBackend(cfg)
        setup_problem(orc)
        orc.vcycle(True)
        pair.append(orc)
    A._assert_same(pair[0], pair[1], "unchanged")
    return pair


def _flip(orc, lvl, iv, box, k, j, i):
    """Flip the lowest mantissa bit of one cell; returns the undo."""
    a = orc.get_level(lvl, iv)
    keep = a.copy()
    a[box:box + 1, k, j, i].view(np.uint64)[...] ^= np.uint64(1)
    assert a[box, k, j, i] != keep[box, k, j, i] or np.isnan(a[box, k, j, i])
    orc.set_level(lvl, iv, a)
    return lambda: orc.set_level(lvl, iv, keep)


@pytest.mark.parametrize("lvl,iv,cell", [(3, 1, (4, 5, 0)), (1, 1, (9, 2, 3)), (0, 3, (2, 3, 4)), (-2, 3, (1, 2, 2))],
                         ids=["face-ghost-top", "face-ghost-lvl1", "old-interior-lvl0", "old-interior-lvl-2"])
def test_one_flipped_bit_fails_the_comparison(two_oracles, lvl, iv, cell):
    a, b = two_oracles
    undo = _flip(b, lvl, iv, 0, *cell)
    try:
        with pytest.raises(AssertionError) as ex:
            A._assert_same(a, b, "flipped")
        assert ex.value.args[0][:2] == (lvl, iv)
    finally:
        undo()
    A._assert_same(a, b, "restored")


@pytest.mark.parametrize("cell", [(0, 0, 3), (0, 9, 9), (9, 4, 0), (0, 0, 0)], ids=["edge", "corner", "edge2", "corner0"])
def test_flipped_unstored_ghost_passes(two_oracles, cell):
    a, b = two_oracles
    undo = _flip(b, 3, 1, 1, *cell)
    try:
        A._assert_same(a, b, "unstored")
    finally:
        undo()
