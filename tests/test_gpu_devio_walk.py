"""The device I/O entry points against the oracle between cycles (tests/apiwalk.py):
omg_put_dense, omg_get_dense, omg_get_dense_grad, omg_put_boxes, omg_get_boxes,
omg_get_boxes_grad, omg_put_boxes_div and omg_get_boxes_flux, each applied to
the device through the MG mirrors on torch tensors and to the C oracle through
numpy on get_level / set_level (apiwalk.devio_oracle, devio_device).

Every comparison is bitwise: every element of a get's output (what the call
defines, and the sentinel or the random bits everywhere else), every count a
call returns, and every stored cell of phi, rhs, old and res on every level
after the step.

Group, the lazy mechanism it meets (omg_lazy.cpp), the kernel_stats counter
that proves it was met:

1. each kind after two cycles: a pending phi mean, deferred ghosts, an
   unstored res, pending rhs shifts on per128 (smoother_gsrb4p@1 >= 2: the
   cycles ended in the pass that defers them); rb_stale_above on ref3;
   physical faces on mx2 (no counter: the trees' own property);
2. a put of phi below a refinement boundary on c4: phi_dirty / phi_dirty_all
   against rbgv_ok, the coarse parts kept between GSRB substeps
   (smoother_gsrb@2 >= 1: the refined level took the substeps that keep them);
3. stored boundary data in rhs's ghost slots on mx2 after phi_bc_store, kept by
   a put without ghosts, overwritten by one with them and by a fill of rhs
   (boxes_put >= 2 and boxes_grad >= 1: the entries ran);
4. the ring-order copy of rhs (rhs_lex_ok) under the device writers of rhs
   (rhs_lex@hi: one rebuild for the first cycle and one per writer);
5. the entries meeting each other without a download between, and a get
   with fill=True right after subtract_mean, set_bc, correct_children, a
   partial-height cycle and a change of methods: phi_gc_ok and the skipped
   fill of enter_get (smoother_gsrb4p@1 on per128 for the chains);
6. seeded walks: all of the above between subtract_mean, methods, vcycle_to,
   correct_children, set_rhs and the other entries (none: the walks are drawn);
7. two and three loopback ranks: the proxies' copies of rhs (prox_rhs_ok)
   under every device writer of rhs with the deep halo on (deep_phi@1 > 0 on
   per128 x2), enter_get's fill decision falling alike on every rank
   (OMG_CHECK_COLLECTIVE=1).

Time.  The oracle's share of each case in seconds of wall time (its set-up,
its steps, numpy's statement of the entry and the downloads or digests),
measured on a CPU-only machine, the slowest case of each group; after the
slash the slowest case's whole wall time on an MI355X's host, oracle and numpy
included (pytest's call duration; that host runs the oracle faster than the
CPU-only machine did).  The first case of a session adds about 1.8 s to
either figure (the import of torch, the first context); it is left out.

  1. kind after two cycles      per128 1.1 / 0.5   per32 0.0 / 0.0   ref3 0.1 / 0.1   mx2 0.1 / 0.1
  2. put below a boundary       c4 1.3 / 0.6
  3. stored boundary data       mx2 0.1 / 0.1
  4. rhs writers, ring          4.4 / 1.9
  5. chains                     per128 1.5 / 0.5   ref3 0.1 / 0.1
     get with fill after        per128 0.7 / 0.3   per32 0.0 / 0.4   ref3 0.1 / 0.1   mx2 0.1 / 0.0
  6. walks                      per128 0.9 / 0.4   per32 0.1 / 0.0   ref3 0.2 / 0.1   mx2 0.2 / 0.1
                                c4 1.9 / 1.1
  7. entries on ranks           per128 x2 4.2 / 1.9 (5 parts)   ref3 x3 0.6 / 0.6 (2 parts)
     get with fill after        per128 x2 3.5 / 1.5   ref3 x3 0.3 / 0.5

The whole file: 184 cases in 42 s on the MI355X's host."""
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


# -- 1. each device I/O kind after two cycles ---------------------------------------
def _kind_ids():
    out = []
    for tree in sorted(TREES):
        cfg = parse(TREES[tree])
        for n, k in enumerate(A.devio_directed_kinds(cfg, *A.tree_levels(TREES[tree]))):
            out.append(pytest.param(tree, n, id=f"{tree}-{n}-{k[0]}"))
    return out


@pytest.mark.parametrize("tree,n", _kind_ids())
def test_device_io_meets_what_two_cycles_leave(monkeypatch, tree, n):
    """No download between the two cycles and the entry: on per128 at a bound
    of 64 boxes it meets a pending shift, deferred ghosts and an unstored res."""
    _bound(monkeypatch)
    p = _profiled(Pair(TREES[tree], devio=True))
    k = A.devio_directed_kinds(p.cfg, *_levels(p))[n]
    p.run([V0, V0, k, V1], lazy=True)
    if tree == "per128_box16":
        # (the cycles ended in k_gsrb4's correction form, the one that defers the ghosts)
        assert _launches(p, "smoother_gsrb4p@1") >= 2


# -- 2. a put of phi below a refinement boundary ------------------------------------
def below_boundary_puts(hi):
    lvl = hi - 1
    return [("put_dense", lvl, 1, "whole"), ("put_boxes", ("perm", lvl, 1), 1, False),
            ("put_boxes", ("subset", lvl, 2), 1, True), ("put_boxes_div", ("perm", lvl, 3), 1, "face", 1.0)]


@pytest.mark.parametrize("n", range(4), ids=["put_dense", "put_boxes", "put_boxes-ghosts", "put_boxes_div"])
def test_put_of_phi_below_a_refinement_boundary(monkeypatch, n):
    """A device put of phi on level 1 between two cycles on the refined GSRB
    tree: the finest level's substeps keep the coarse parts of their
    refinement-boundary ghosts (Level::rbgv_ok), and the put changes the level
    below them (test_subtract_mean_of_phi_below_a_refinement_boundary's
    analogue)."""
    _bound(monkeypatch)
    p = _profiled(Pair(C4, devio=True))
    hi = _levels(p)[1]
    p.run([V0, below_boundary_puts(hi)[n], V1], lazy=True)
    # (the refined level's substeps are the ones that store and reuse the coarse parts)
    assert _launches(p, f"smoother_gsrb@{hi}") >= 1


# -- 3. stored boundary data --------------------------------------------------------
def stored_bc_list(hi):
    perm = ("perm", hi, 1)
    return [("phi_bc_store",), V0, ("put_boxes", perm, 2, False), V1, ("put_boxes", perm, 2, True), V1,
            ("get_boxes_grad", perm, 2, "face", 1.0, True), V1]


def test_rhs_ghost_slots_after_phi_bc_store(monkeypatch):
    """After mg_phi_bc_store rhs's ghost slots hold the boundary data: a put
    of rhs without ghosts keeps it, one with ghosts overwrites it, and so does
    a get that fills rhs; a cycle follows each."""
    _bound(monkeypatch)
    p = _profiled(Pair(TREES["mx2_helm64_box16"], devio=True))
    p.run(stored_bc_list(_levels(p)[1]), lazy=True)
    assert _launches(p, "boxes_put") >= 2 and _launches(p, "boxes_grad") >= 1


def stored_bc_host_writers_list(hi):
    """The entries of the original C-ABI that write rhs's ghost slots."""
    return [("phi_bc_store",), V0, ("upload", 2, hi), V1, ("fill_lvl", hi, 2), V1, ("subtract_mean", 2, 1), V1]


def test_host_writers_of_rhs_ghost_slots_after_phi_bc_store(monkeypatch):
    """What test_rhs_ghost_slots_after_phi_bc_store found, for the older
    entries: after mg_phi_bc_store a write of rhs's ghost slots changes phi's
    boundary values, so the next stand-alone cycle's fill of phi must not be
    skipped (an upload of rhs, a fill of rhs, subtract_mean with the ghosts)."""
    _bound(monkeypatch)
    p = Pair(TREES["mx2_helm64_box16"])
    p.run(stored_bc_host_writers_list(_levels(p)[1]), lazy=True)


# -- 4. device writers of rhs between ring sweeps -----------------------------------
def test_device_rhs_writers_between_ring_sweeps(monkeypatch):
    """The ring-order copy of rhs (rhs_lex_ok) follows every device writer of
    rhs: the finest level's is rebuilt for the first cycle and after each of
    the four writers."""
    monkeypatch.delenv("OMG_BLOCK3_MIN_BOXES", raising=False)
    p = _profiled(Pair(RING, devio=True))
    hi = _levels(p)[1]
    p.run(A.ring_devio_writers_list(hi), skip=A.DEVIO_RHS_WRITERS)
    assert _launches(p, f"rhs_lex@{hi}") >= 5


# -- 5. the entries meeting each other ----------------------------------------------
def chains(cfg, hi):
    perm = ("perm", hi, 1)
    return {"blocks": [V0, ("put_boxes_div", perm, 2, "face", 1.0),
                       ("get_boxes_flux", perm, 1, "face", -1.0, True, A.I_COEF, True), V0,
                       ("get_boxes", perm, 1, True, True), V1],
            "dense": [("put_dense", hi, 2, "whole"), V0, ("get_dense_grad", hi, 1, "whole", -1.0, True), V1]}


@pytest.mark.parametrize("chain", ["blocks", "dense"])
@pytest.mark.parametrize("tree", ["per128_box16", "ref3_gs_box8"])
def test_chains_without_a_download_between(monkeypatch, tree, chain):
    """put, solve, get as an AMR host calls them: no host download between the
    steps (what a get returns is still compared inside its step)."""
    _bound(monkeypatch)
    p = _profiled(Pair(TREES[tree], devio=True))
    p.run(chains(p.cfg, _levels(p)[1])[chain], lazy=True, skip=A.DEVIO_KINDS)
    if tree == "per128_box16":
        assert _launches(p, "smoother_gsrb4p@1") >= 1


def fill_after_lists(cfg, lo, hi):
    """{name: steps}: a get with fill=True right after an entry that changes
    what a fill of phi gives or whether it still stands (enter_get skips phi's
    fill where phi_gc_ok stands), no download between the two."""
    perm, sub = ("perm", hi, 1), ("subset", hi, 2)
    leaves = ("leaves",) if cfg["n_levels"] > 1 else ("perm", hi, 3)
    gets = [("get_boxes", perm, 1, True, True), ("get_dense_grad", hi, 1, "whole", -1.0, True),
            ("get_boxes_flux", sub, 1, "face", -1.0, True, A.I_COEF, False),
            ("get_boxes_grad", leaves, 1, "cell", 0.37, True)]
    pres = {"subtract_mean": ("subtract_mean", 1, 0), "subtract_mean-ghosts": ("subtract_mean", 1, 1),
            "correct_children": ("correct_children", hi - 1), "partial-cycle": ("vcycle_to", hi - 1, False, True),
            "smoother": ("methods", {"smoother": "gs" if cfg["smoother"] == "gsrb" else "gsrb"}),
            "operator": ("methods", {"op": "lpl" if cfg["op"] == "helm" else "helm", "lam": 0.5})}
    if cfg["bc"] != "per":
        pres["set_bc"] = ("bc", 3, A.T.MG_BC_DIRICHLET, 0.375)
    return {name: [V0, pre, gets[q % len(gets)], V1] for q, (name, pre) in enumerate(sorted(pres.items()))}


FILL_AFTER_SKIP = ("subtract_mean", "correct_children", "vcycle_to", "methods", "bc")
FILL_AFTER = [pytest.param(tree, name, id=f"{tree}-{name}") for tree in sorted(TREES)
              for name in sorted(fill_after_lists(parse(TREES[tree]), -1, 1))]


@pytest.mark.parametrize("tree,name", FILL_AFTER)
def test_get_with_fill_right_after_an_entry(monkeypatch, tree, name):
    _bound(monkeypatch)
    p = Pair(TREES[tree], devio=True)
    p.run(fill_after_lists(p.cfg, *_levels(p))[name], lazy=True, skip=FILL_AFTER_SKIP)


# -- 6. seeded walks ----------------------------------------------------------------
@pytest.mark.parametrize("seed", A.WALK_SEEDS)
@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("tree", sorted(A.WALK_TREES))
def test_walk_over_device_io_and_entry_points_matches_oracle(monkeypatch, tree, lazy, seed):
    _bound(monkeypatch)
    p = Pair(A.WALK_TREES[tree], devio=True)
    p.run(A.devio_walk(tree, seed, levels=_levels(p)), lazy)


# -- 7. more than one rank ----------------------------------------------------------
# (name, tree, ranks, parts the list of kinds is run in)
RANK_CASES = [("per128-2", PER128, 2, 5), ("ref3-3", TREES["ref3_gs_box8"], 3, 2)]


def rank_list(cfg, lo, hi, part, parts):
    steps = []
    for k in A.devio_directed_kinds(cfg, lo, hi)[part::parts]:
        steps += [V0, V0, k]   # (the next kind's two cycles are this one's cycle after)
    return steps + [V1]


def _run_ranks(args, ranks, steps, deep, skip=()):
    """The oracle at the same rank count first (its records are the device
    ranks' data and expectations), then the ranks; deep: every rank must have
    made deep-halo rounds on level 1."""
    assert ranks <= 4
    cfg = parse(args)
    orc = OracleBackend(cfg, ranks)
    setup_problem(orc)
    A.devio_setup(orc)
    recs = {}
    o_scalars, o_boxes = A.run_rank(orc, steps, True, recs, skip)

    def body(be, rank, reduce):
        for lvl in range(1, be.tree.highest_lvl + 1):
            assert len(be.my_ids(lvl)), f"rank {rank} owns no box of level {lvl}"
        A.devio_setup(be)
        be.mg.ctx.call("set_profiling", 1)
        out = A.run_rank(be, steps, True, recs, skip)
        be.mg.ctx.call("synchronize")
        n_deep = be.mg.ctx.kernel_stats("deep_phi@1")[0]
        assert not deep or n_deep > 0, f"rank {rank}: {n_deep} deep-halo rounds"
        return out

    res = run_loopback(args, ranks, body, timeout=120)
    seen = set()
    for rank, (scalars, boxes) in enumerate(res):
        assert scalars == o_scalars, (rank, scalars, o_scalars, steps)
        for key, h in boxes.items():
            n, lvl, id_, iv = key
            assert h == o_boxes[key], f"rank {rank} step {n} {steps[n]} level {lvl} box {id_} variable {iv} of {steps}"
        seen |= set(boxes)
    assert seen == set(o_boxes)


def rank_fill_after_list(args):
    steps = []
    for _, lst in sorted(fill_after_lists(parse(args), *A.tree_levels(args)).items()):
        steps += lst[:3]   # (the next list's first cycle is this one's cycle after)
    return steps + [V1]


RANK_PARTS = [pytest.param(*c[:3], part, c[3], id=f"{c[0]}-{part}") for c in RANK_CASES for part in range(c[3])]


@pytest.mark.parametrize("name,args,ranks,part,parts", RANK_PARTS)
def test_device_io_after_cycles_on_ranks(monkeypatch, name, args, ranks, part, parts):
    """Every directed kind once (a part of them per case), each after two
    cycles without a download, every rank listing its own boxes of the kind's
    selection and making every call; per128 with the block passes' bound at
    one box, so that the split finest level takes them with the deep halo (the
    proxies' rhs under every device writer of rhs).  What a get returns is
    compared per box on the rank that listed it, the box checkpoints as
    digests."""
    monkeypatch.setenv("OMG_CHECK_COLLECTIVE", "1")
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", "1")
    monkeypatch.delenv("OMG_BLOCK3_COLUMN", raising=False)
    lo, hi = A.tree_levels(args)
    _run_ranks(args, ranks, rank_list(parse(args), lo, hi, part, parts), deep=args == PER128)


@pytest.mark.parametrize("name,args,ranks", [c[:3] for c in RANK_CASES], ids=[c[0] for c in RANK_CASES])
def test_get_with_fill_after_entries_on_ranks(monkeypatch, name, args, ranks):
    """fill_after_lists on ranks: enter_get's decision to skip phi's fill is
    made from flags that every rank must have changed alike
    (OMG_CHECK_COLLECTIVE=1 checks the cycles' own), and what the get returns
    must be a real fill's, across rank boundaries too."""
    monkeypatch.setenv("OMG_CHECK_COLLECTIVE", "1")
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", "1")
    monkeypatch.delenv("OMG_BLOCK3_COLUMN", raising=False)
    steps = rank_fill_after_list(args)
    _run_ranks(args, ranks, steps, deep=args == PER128, skip=FILL_AFTER_SKIP)
