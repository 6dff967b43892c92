"""Every C-ABI entry point against the oracle between cycles (tests/apiwalk.py).

1. each entry meets what a cycle leaves: set-up, two cycles without the max
   residual and without a download between (a pending phi shift, deferred
   ghosts, cached rhs sums, proxies' rhs), then the entry, then a cycle;
2. cycles to a level below the top and cycles that are not stand-alone,
   called from outside (fas_vcycle's `!full` branch);
3. smoother, operator, lambda and subtract_mean changed between cycles, on the
   block passes' tree and on the register ring's, and the writers of rhs
   other than an upload between ring sweeps;
4. seeded walks over the whole vocabulary;
5. the same on two to four ranks through the loopback transport, against the
   oracle at the same rank count.

Every comparison is bitwise: every stored cell of phi, rhs, old and res on
every level after every step, and every scalar a call returns.

Time.  The oracle's share of each case, in seconds of wall time: its set-up,
its steps and its downloads (or per-box digests) alone, measured on a CPU-only
machine, the slowest case of each group.  The GPU's own share of these cases
has not been measured by anyone; the lists are sized by the oracle's.

  1. entry after two cycles     per128 1.2   per32 0.0   ref3 0.1   mx2 0.1
     subtract_mean of phi       per128 0.9   c4 1.3      omg_set_bc  per128 0.7
  2. cycle to every level       per128 2.6   ref3 0.2   c4 4.7
  3. methods                    per128 2.4   ring (shortened list) 4.2
     rhs writers, ring          4.2
  4. walks                      per128 1.3   per32 0.1   ref3 0.2   mx2 0.3   c4 2.6
  5. entries on ranks           per128 x2 4.4 (3 parts)   per128 x4 4.5 (3 parts)
                                ref3 x3 0.8 (1 part)   c4 x3 4.7 (8 parts)
     walk on ranks              per128 x2 1.8   per128 x4 1.7   ref3 x3 0.2   c4 x3 4.7"""
import pytest

from tests import apiwalk as A
from tests.apiwalk import C4, PER128, RING, TREES, V0, V1, Pair
from tests.mgdriver import OracleBackend, parse, run_loopback, setup_problem

pytestmark = pytest.mark.gpu


def _bound(monkeypatch, bound="64"):
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", bound)
    monkeypatch.delenv("OMG_BLOCK3_COLUMN", raising=False)


def _levels(p):
    return p.orc.tree.lowest_lvl, p.orc.tree.highest_lvl


def _profiled(p):
    """Count the device's launches by kernel family (omg_kernel_stats)."""
    p.dev.mg.ctx.call("set_profiling", 1)
    return p


def _launches(p, name):
    p.dev.mg.ctx.call("synchronize")
    return p.dev.mg.ctx.kernel_stats(name)[0]


# -- 1. each entry after two cycles ------------------------------------------------
def _kind_ids():
    out = []
    for tree in sorted(TREES):
        cfg = parse(TREES[tree])
        for n, k in enumerate(A.directed_kinds(cfg, *A.tree_levels(TREES[tree]))):
            out.append(pytest.param(tree, n, id=f"{tree}-{n}-{k[0]}"))
    return out


@pytest.mark.parametrize("tree,n", _kind_ids())
def test_entry_meets_what_two_cycles_leave(monkeypatch, tree, n):
    """per128 at a bound of 64: the two cycles leave a pending shift and
    deferred ghosts; per32: the LDS tail with a pending shift; ref3: refinement
    boundaries (rb_stale_above); mx2: physical faces.  No download before the
    entry's own comparison."""
    _bound(monkeypatch)
    p = Pair(TREES[tree])
    k = A.directed_kinds(p.cfg, *_levels(p))[n]
    p.run([V0, V0, k, V1], lazy=True)


@pytest.mark.parametrize("ghosts", [0, 1])
def test_subtract_mean_of_phi_after_deferred_ghosts(monkeypatch, ghosts):
    """omg_subtract_mean(phi) right after two stand-alone cycles: the shift is
    pending and the finest level's ghosts are deferred.  With ghosts = 0 the
    reference keeps the ghosts of the last fill, so deferred ghosts are filled
    before the interior is subtracted; then the ghosts are read (a fill of res
    changes nothing of phi) and a cycle follows."""
    _bound(monkeypatch)
    p = _profiled(Pair(PER128))
    p.run([V0, V0, ("subtract_mean", 1, ghosts), ("residual_lvl", 1), V1], lazy=True)
    # (the cycles ended in k_gsrb4's correction form, the one that defers the ghosts)
    assert _launches(p, "smoother_gsrb4p@1") >= 2


def test_set_bc_after_deferred_ghosts(monkeypatch):
    """omg_set_bc makes every level's ghosts stale; ghosts a cycle deferred are
    filled first, as the reference's last fill left them (no physical face on
    this tree: the condition itself changes nothing)."""
    _bound(monkeypatch)
    p = _profiled(Pair(PER128))
    p.run([V0, V0, ("bc", 3, A.T.MG_BC_DIRICHLET, 0.375), V1], lazy=True)
    assert _launches(p, "smoother_gsrb4p@1") >= 2


@pytest.mark.parametrize("ghosts", [0, 1])
def test_subtract_mean_of_phi_below_a_refinement_boundary(monkeypatch, ghosts):
    """omg_subtract_mean(phi) between two cycles on the refined GSRB tree:
    the finest level's substeps keep the coarse parts of their
    refinement-boundary ghosts from one substep to the next (Level::rbgv_ok),
    and the subtraction changes the level below them."""
    _bound(monkeypatch)
    Pair(C4).run([V0, ("subtract_mean", 1, ghosts), V1], lazy=True)


# -- 2. partial-height and non-stand-alone cycles -----------------------------------
PARTIAL = [("per128-512", PER128, "512"), ("per128-64", PER128, "64"), ("ref3_gs_box8", TREES["ref3_gs_box8"], "64"),
           ("c4_ref2_box16", C4, "64")]


@pytest.mark.parametrize("standalone", [False, True])
@pytest.mark.parametrize("want", [False, True])
@pytest.mark.parametrize("name,args,bound", PARTIAL, ids=[x[0] for x in PARTIAL])
def test_cycle_to_every_level(monkeypatch, name, args, bound, want, standalone):
    _bound(monkeypatch, bound)
    p = Pair(args)
    lo, hi = _levels(p)
    steps = []
    for k in range(lo, hi + 1):   # (each meets what a stand-alone cycle left: no download after V0)
        steps += [V0, ("vcycle_to", k, want, standalone)]
    p.run(steps + [V1], lazy=True)


# -- 3. methods changed between cycles --------------------------------------------
def test_methods_changed_between_cycles_block_passes(monkeypatch):
    _bound(monkeypatch)
    p = _profiled(Pair(PER128))
    p.run(A.METHODS_LIST, lazy=True)
    # (the finest level took the block passes under GSRB and none under GS: 9 of the 11 cycles)
    assert _launches(p, "smoother_gsrb4@1") >= 1 and _launches(p, "smoother_gsrb4p@1") >= 1
    assert _launches(p, "smoother_gs@1") >= 1


def test_methods_changed_between_cycles_ring(monkeypatch):
    monkeypatch.delenv("OMG_BLOCK3_MIN_BOXES", raising=False)
    p = _profiled(Pair(RING))
    p.run(A.ring_methods_list(), lazy=True)
    # (the register ring served the finest level: its ring-order copy of rhs was built)
    assert _launches(p, "rhs_lex@1") >= 1


def test_rhs_writers_between_ring_sweeps(monkeypatch):
    """The ring-order copy of rhs (rhs_lex_ok) follows every writer of rhs:
    the finest level's is rebuilt for the first cycle and after each of the
    five writers (every entry that may write rhs drops every level's copy)."""
    monkeypatch.delenv("OMG_BLOCK3_MIN_BOXES", raising=False)
    p = _profiled(Pair(RING))
    hi = _levels(p)[1]
    p.run(A.ring_writers_list(hi), skip=A.RHS_WRITERS)
    assert _launches(p, f"rhs_lex@{hi}") >= 6


# -- 4. seeded walks ------------------------------------------------------------
@pytest.mark.parametrize("seed", A.WALK_SEEDS)
@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("tree", sorted(A.WALK_TREES))
def test_walk_over_entry_points_matches_oracle(monkeypatch, tree, lazy, seed):
    _bound(monkeypatch)
    p = Pair(A.WALK_TREES[tree])
    p.run(A.walk(tree, seed, levels=_levels(p)), lazy)


# -- 5. more than one rank -----------------------------------------------------
@pytest.fixture
def _check_collective(monkeypatch):
    monkeypatch.setenv("OMG_CHECK_COLLECTIVE", "1")


# (name, tree, ranks, coarse replication in cells, switch, parts the list of kinds is run in)
RANK_CASES = [("per128-2", PER128, 2, 0, None, 3), ("per128-4", PER128, 4, 0, None, 3),
              ("per128-2-nodeep", PER128, 2, 0, "OMG_NO_DEEP", 3), ("per128-4-nodeep", PER128, 4, 0, "OMG_NO_DEEP", 3),
              ("ref3-3", TREES["ref3_gs_box8"], 3, 0, None, 1), ("c4-3-rep", C4, 3, 64 * 16 ** 3, None, 8)]
RANK_TREE = {PER128: "per128_box16", TREES["ref3_gs_box8"]: "ref3_gs_box8", C4: "c4_ref2_box16"}


def _run_ranks(args, ranks, rep, steps, lazy, deep=None):
    """deep: whether every rank must have made deep-halo rounds on level 1
    (True), none (False), or either (None)."""
    cfg = parse(args)

    def body(be, rank, reduce):
        for lvl in range(1, be.tree.highest_lvl + 1):
            assert len(be.my_ids(lvl)), f"rank {rank} owns no box of level {lvl}"
        be.mg.ctx.call("set_profiling", 1)
        out = A.run_rank(be, steps, lazy)
        be.mg.ctx.call("synchronize")
        n_deep = be.mg.ctx.kernel_stats("deep_phi@1")[0]
        assert deep is None or (n_deep > 0) == deep, f"rank {rank}: {n_deep} deep-halo rounds"
        return out

    res = run_loopback(args, ranks, body, timeout=120, rep_cells=rep)
    orc = OracleBackend(cfg, ranks)
    setup_problem(orc)
    o_scalars, o_boxes = A.run_rank(orc, steps, lazy)
    seen = set()
    # (max_residual_lvl is a rank's own maximum, as the reference's; the oracle's is the tree's)
    local = [n for n in o_scalars if steps[n][0] == "max_residual_lvl"]
    for n in local:
        assert max(r[0][n] for r in res) == o_scalars[n], (n, steps[n], steps)
    for rank, (scalars, boxes) in enumerate(res):
        assert {n: v for n, v in scalars.items() if n not in local} == \
            {n: v for n, v in o_scalars.items() if n not in local}, (rank, scalars, o_scalars, steps)
        for key, h in boxes.items():
            n, lvl, id_, iv = key
            assert h == o_boxes[key], f"rank {rank} step {n} {steps[n]} level {lvl} box {id_} variable {iv} of {steps}"
        seen |= set(boxes)
    assert seen == set(o_boxes)


def _rank_list(cfg, lo, hi, part, parts):
    steps = []
    for k in A.directed_kinds(cfg, lo, hi)[part::parts]:
        steps += [V0, V0, k]   # (the next kind's two cycles are this one's cycle after)
    return steps + [V1]


RANK_PARTS = [pytest.param(*c[:5], part, c[5], id=f"{c[0]}-{part}") for c in RANK_CASES for part in range(c[5])]


@pytest.mark.parametrize("name,args,ranks,rep,switch,part,parts", RANK_PARTS)
def test_entries_after_cycles_on_ranks(monkeypatch, _check_collective, name, args, ranks, rep, switch, part, parts):
    """Every kind once (a part of them per case, so that the oracle's replay
    stays within a few seconds), each after two cycles without a download; the
    128^3 trees with the block passes' bound at one box, so that the split
    finest level takes them with the deep halo (the proxies' rhs under every
    writer of rhs) or, OMG_NO_DEEP, without."""
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", "1")
    if switch:
        monkeypatch.setenv(switch, "1")
    lo, hi = A.tree_levels(args)
    _run_ranks(args, ranks, rep, _rank_list(parse(args), lo, hi, part, parts), lazy=True,
               deep=None if args != PER128 else not switch)


@pytest.mark.parametrize("name,args,ranks,rep,switch", [c[:5] for c in RANK_CASES], ids=[x[0] for x in RANK_CASES])
def test_walk_on_ranks(monkeypatch, _check_collective, name, args, ranks, rep, switch):
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", "1")
    if switch:
        monkeypatch.setenv(switch, "1")
    steps = A.walk(RANK_TREE[args], A.WALK_SEEDS[0], n_steps=8, levels=A.tree_levels(args))
    # (a walk may change the smoother before its first cycle over the top level:
    # only the absence of deep-halo rounds under OMG_NO_DEEP is sure)
    _run_ranks(args, ranks, rep, steps, lazy=True, deep=False if switch else None)
