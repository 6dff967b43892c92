"""Walks over the C-ABI's entry points, the device and the C oracle side by side.

libomg.so keeps part of its state lazily (a pending phi shift, deferred
ghosts, derived copies of rhs, refinement-boundary ghosts known to be stale,
DESIGN.md §5); every entry of include/omg.h either honours that state or drops
it.  A walk is a list of steps, one kind per entry point, each applied alike
to the device (octree-mg_amd's mirrors or ctx.call) and to the oracle
(oracle/pyoracle.py); after every step every stored cell of phi, rhs, old and
res on every level is compared on its bits, and so is every returned scalar.

Steps are tuples, the kind first:

  ("vcycle", want)                      stand-alone cycle over the whole tree
  ("vcycle_to", k, want, standalone)    mg_fas_vcycle(highest_lvl=k, ...)
  ("fmg",)                              FMG cycle with a guess, max residual
  ("counts", (down, up))                n_cycle_down / n_cycle_up
  ("apply_op",) / ("apply_op", i_out)   mg_apply_op into res / into i_out
  ("fill",)                             mg_fill_ghost_cells(phi)
  ("fill_lvl", lvl, iv)                 mg_fill_ghost_cells_lvl
  ("upload",) / ("upload", iv, lvl)     half of phi on every level / of iv on lvl
  ("prolong", lvl, iv, iv_to, add)      mg_prolong
  ("restrict_lvl", iv, lvl)             mg_restrict_lvl
  ("residual_lvl", lvl), ("max_residual_lvl", lvl)
  ("smooth_boxes", lvl, n_cycle), ("update_coarse", lvl), ("correct_children", lvl)
  ("subtract_mean", iv, ghosts), ("get_sum", iv), ("set_rhs", f1, f2)
  ("methods", {"smoother": "gs"|"gsrb", "op": "lpl"|"helm", "lam": x, "sub": bool})
  ("bc", nb, type, value)               omg_set_bc of phi, one face
  ("phi_bc_store",)

The generator (walk) draws only calls that are legal on the tree: the oracle
abort()s where the reference has an error stop (prolong of the highest level,
restriction of the lowest).

The lists are sized by the oracle's wall time (a few seconds per case at the
most), recorded in tests/test_gpu_api_walk.py.
"""
import hashlib
import random

import numpy as np

from tests.mgdriver import OPS, SOLVER_DEFAULTS, DeviceBackend, OracleBackend, T, omg, parse, setup_problem

V0, V1 = ("vcycle", False), ("vcycle", True)

PER128 = "16 128 128 128 1 v gsrb lpl 0 per sol 1 lb 0"
C4 = "16 128 128 128 1 v gsrb lpl 0 sol sol 2 lb 0"
RING = "16 128 256 256 1 v gs lpl 0 d0 sol 1 lb 0"
TREES = {"per128_box16": PER128,
         "per32_box8": "8 32 32 32 1 v gsrb lpl 0 per sol 1 lb 0",
         "ref3_gs_box8": "8 32 32 32 1 v gs lpl 0 sol sol 3 lb 0",
         "mx2_helm64_box16": "16 64 64 64 1 v gsrb helm 2 mx2 sol 1 lb 0"}


def _stored_mask(nc):
    """Interior and face ghosts: edge and corner ghosts are not stored."""
    s = nc + 2
    ix = np.arange(s)
    bnd = ((ix == 0) | (ix == s - 1)).astype(int)
    return (bnd[:, None, None] + bnd[None, :, None] + bnd[None, None, :]) < 2


def _assert_same(dev, orc, msg, ivs=(1, 2, 3, 4)):
    for lvl in dev.levels():
        if not len(dev.my_ids(lvl)):
            continue
        u = ~_stored_mask(dev.tree.box_size_lvl[lvl])
        for iv in ivs:
            a, b = dev.get_level(lvl, iv), orc.get_level(lvl, iv)
            a[:, u] = b[:, u] = 0.0   # (the few unstored cells out of the way: no gather of all the others)
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (lvl, iv, msg)


def _is_oracle(be):
    return isinstance(be, OracleBackend)


def _scalar(be, name, *a):
    if _is_oracle(be):
        return float(getattr(be.o, name)(*a))
    return be.mg.ctx.scalar(name, *a)


def _put(be, lvl, iv, data):
    """set_level of this rank's boxes; a rank without boxes still calls where
    the upload is collective (mgdriver.setup_problem's put)."""
    if len(be.my_ids(lvl)):
        be.set_level(lvl, iv, data)
    elif be.collective(lvl, iv):
        nc = be.tree.box_size_lvl[lvl]
        be.set_level(lvl, iv, np.zeros((0, nc + 2, nc + 2, nc + 2)))


class Methods:
    """What mg_set_methods and the solver parameters hold, pushed alike to
    either backend."""

    def __init__(self, cfg):
        self.smoother, self.op, self.lam = cfg["smoother"], cfg["op"], cfg["lam"]
        self.sub = cfg["bc"] == "per"
        self.params = list(cfg.get("cycles") or SOLVER_DEFAULTS[:2]) + list(cfg.get("coarse") or SOLVER_DEFAULTS[2:])

    def change(self, d):
        for k, v in d.items():
            if k not in ("smoother", "op", "lam", "sub"):
                raise ValueError(k)
            setattr(self, k, v)

    def push(self, be, oracle_cycles=None):
        down, up, cmax, cabs, crel = self.params
        if _is_oracle(be):
            import pyoracle  # on sys.path once OracleBackend exists (checker only)
            if oracle_cycles is not None:
                down, up = oracle_cycles
            sm = pyoracle.GSRB if self.smoother == "gsrb" else pyoracle.GS
            be.o.configure(op=OPS[self.op], lam=self.lam, smoother=sm, n_cycle_down=down, n_cycle_up=up,
                           max_coarse_cycles=cmax, res_abs=cabs, res_rel=crel, subtract_mean=self.sub)
            return
        mg = be.mg
        mg.smoother_type = T.MG_SMOOTHER_GSRB if self.smoother == "gsrb" else T.MG_SMOOTHER_GS
        mg.n_smoother_substeps = 2 if self.smoother == "gsrb" else 1
        mg.operator_type, mg.helmholtz_lambda, mg.subtract_mean = OPS[self.op], self.lam, self.sub
        mg.n_cycle_down, mg.n_cycle_up = down, up
        mg.max_coarse_cycles, mg.residual_coarse_abs, mg.residual_coarse_rel = cmax, cabs, crel
        mg._push_methods()


def apply_step(be, meth, step, src=None):
    """One step on one backend; the scalar the call returns, or None.  src:
    the backend an upload takes its data from (the same cells on either)."""
    kind, a = step[0], step[1:]
    src = be if src is None else src
    if kind == "vcycle":
        return be.vcycle(a[0])
    if kind == "vcycle_to":
        k, want, sa = a
        return be.vcycle_to(k, want, sa)
    if kind == "fmg":
        return be.fmg(True, True)
    if kind == "counts":
        meth.params[:2] = a[0]
        meth.push(be)
    elif kind == "methods":
        meth.change(a[0])
        meth.push(be)
    elif kind == "apply_op":
        be.apply_op(a[0] if a else 4)
    elif kind == "fill":
        be.fill_ghost_cells(1)
    elif kind == "fill_lvl":
        be.call("fill_ghost_cells_lvl", *a)
    elif kind == "upload":
        # another phi (or rhs), interior and ghosts (the ghosts no fill's result)
        iv = a[0] if a else 1
        for lvl in ([a[1]] if a else be.levels()):
            _put(be, lvl, iv, 0.5 * src.get_level(lvl, iv) if len(be.my_ids(lvl)) else None)
    elif kind in ("prolong", "restrict_lvl", "residual_lvl", "smooth_boxes", "update_coarse", "correct_children",
                  "subtract_mean", "set_rhs"):
        be.call(kind, *a)
    elif kind in ("max_residual_lvl", "get_sum"):
        return _scalar(be, kind, *a)
    elif kind == "bc":
        nb, t, v = a
        if _is_oracle(be):
            be.o.set_bc(1, nb, t, v)
        else:
            be.mg.bc[nb][1] = omg.BC(t, v)
            be.mg.ctx.call("set_bc", 1, nb, int(t), float(v))
    elif kind == "phi_bc_store":
        if _is_oracle(be):
            be.o.phi_bc_store()
        else:
            omg.mg_phi_bc_store(be.mg)
    else:
        raise ValueError(kind)
    return None


def is_cycle(step):
    return step[0] in ("vcycle", "vcycle_to", "fmg")


def _lazy_skip(step):
    """No download after these in lazy mode: a stand-alone cycle over the whole
    tree without the max residual (it may leave a pending shift and deferred
    ghosts) or a change of the settings (it reads no cell)."""
    return step == V0 or step[0] in ("counts", "methods")


class Pair:
    """The device and the oracle over one problem, given every change alike.
    device=False: the oracle alone (the walks' legality, on a CPU)."""

    def __init__(self, args, device=True):
        self.cfg = cfg = parse(args)
        self.orc = OracleBackend(cfg)
        self.dev = DeviceBackend(cfg) if device else None
        self.meth = Methods(cfg)
        self.params = self.meth.params
        for be in (self.dev, self.orc):
            if be is not None:
                setup_problem(be)

    def set(self, cycles=None, coarse=None, oracle_cycles=None):
        if cycles is not None:
            self.params[:2] = cycles
        if coarse is not None:
            self.params[2:] = coarse
        if self.dev is not None:
            self.meth.push(self.dev)
        self.meth.push(self.orc, oracle_cycles)

    def step(self, step, msg):
        # (an upload's data comes from the oracle, before either takes the step)
        if step[0] == "upload":
            lvls = [step[2]] if len(step) > 1 else list(self.orc.levels())
            iv = step[1] if len(step) > 1 else 1
            for lvl in lvls:
                a = 0.5 * self.orc.get_level(lvl, iv)
                for be in (self.dev, self.orc):
                    if be is not None:
                        be.set_level(lvl, iv, a)
            return
        # (a change of the settings is made in self.meth twice, to the same values)
        r_orc = apply_step(self.orc, self.meth, step)
        if self.dev is not None:
            r_dev = apply_step(self.dev, self.meth, step)
            assert r_dev == r_orc, (r_dev, r_orc, msg)

    def run(self, steps, lazy=False, skip=()):
        """lazy: no comparison right after a cycle without the max residual
        or a change of the counts.  The download is a reader of phi's ghosts
        like any other and fills deferred ones first, so only then does the
        cycle's deferral meet the step after it.  skip: kinds of step that no
        comparison follows either (the next step's covers them)."""
        for n, step in enumerate(steps):
            msg = f"step {n} {step} of {steps}"
            self.step(step, msg)
            if self.dev is None:
                continue
            if step[0] in skip and n + 1 < len(steps):
                continue
            if not (lazy and _lazy_skip(step) and n + 1 < len(steps)):
                _assert_same(self.dev, self.orc, msg)


# -- the generator --------------------------------------------------------------
def tree_class(cfg):
    return "per" if cfg["bc"] == "per" else "ref" if cfg["n_levels"] > 1 else "phys"


# one fixed argument choice per kind (the directed lists), as a function of the
# tree's lowest and highest level; subtract_mean of phi with and without the
# ghosts, and of rhs (whose leaf sums a cycle leaves cached)
def directed_kinds(cfg, lo, hi):
    ks = [("vcycle_to", hi - 1, False, True), ("vcycle_to", hi, True, False),
          ("prolong", hi - 1, 1, 2, 0), ("restrict_lvl", 2, hi), ("fill_lvl", hi, 4),
          ("residual_lvl", hi), ("max_residual_lvl", hi), ("smooth_boxes", hi, 1),
          ("update_coarse", hi), ("correct_children", hi - 1),
          ("subtract_mean", 1, 0), ("subtract_mean", 1, 1), ("subtract_mean", 2, 0),
          ("get_sum", 1), ("set_rhs", 0.5, -1.25), ("apply_op", 2), ("upload", 2, hi),
          ("methods", {"smoother": "gs" if cfg["smoother"] == "gsrb" else "gsrb"}),
          ("methods", {"op": "lpl" if cfg["op"] == "helm" else "helm", "lam": 0.5}),
          ("methods", {"sub": cfg["bc"] != "per"})]
    if cfg["bc"] != "per":
        ks += [("bc", 3, T.MG_BC_DIRICHLET, 0.375), ("phi_bc_store",)]
    return ks


NEW_KINDS = ["vcycle_to", "prolong", "restrict_lvl", "fill_lvl", "residual_lvl", "max_residual_lvl", "smooth_boxes",
             "update_coarse", "correct_children", "subtract_mean", "get_sum", "set_rhs", "apply_op", "upload",
             "methods"]
OLD_KINDS = ["fmg", "counts", "fill"]
NONPER_KINDS = ["bc", "phi_bc_store"]


def allowed_kinds(cls):
    return NEW_KINDS + OLD_KINDS + (NONPER_KINDS if cls != "per" else [])


def _draw(rng, kind, cfg, lo, hi, meth):
    """A legal argument choice of one kind; meth: the methods the walk has set
    so far (a dict, updated by a methods step)."""
    r = rng.randrange
    if kind == "vcycle_to":
        return (kind, lo + r(hi - lo + 1), bool(r(2)), bool(r(2)))
    if kind == "prolong":
        return (kind, lo + r(hi - lo)) + rng.choice([(4, 1, 1), (1, 3, 0), (1, 2, 0), (2, 4, 1)])
    if kind == "restrict_lvl":
        return (kind, rng.choice([1, 2, 4]), lo + 1 + r(hi - lo))
    if kind == "fill_lvl":
        return (kind, lo + r(hi - lo + 1), rng.choice([1, 4]))
    if kind in ("residual_lvl", "max_residual_lvl"):
        return (kind, lo + r(hi - lo + 1))
    if kind == "smooth_boxes":
        return (kind, lo + r(hi - lo + 1), r(5))
    if kind == "update_coarse":
        return (kind, lo + 1 + r(hi - lo))
    if kind == "correct_children":
        return (kind, lo + r(hi - lo))
    if kind == "subtract_mean":
        return (kind, 1 + r(2), r(2))
    if kind == "get_sum":
        return (kind, 1 + r(2))
    if kind == "set_rhs":
        return (kind, rng.choice([0.5, -1.25, 0.0, 2.0]), rng.choice([0.5, -1.25, 0.0, 2.0]))
    if kind == "apply_op":
        return (kind, rng.choice([2, 4]))
    if kind == "upload":
        return (kind, 1 + r(2), hi - r(2))
    if kind == "methods":
        what = rng.choice(["smoother", "op", "sub"])
        if what == "smoother":
            d = {"smoother": "gs" if meth["smoother"] == "gsrb" else "gsrb"}
        elif what == "op":
            d = {"op": "lpl"} if meth["op"] == "helm" else {"op": "helm", "lam": rng.choice([0.5, 3.0])}
        else:
            d = {"sub": not meth["sub"]}
        meth.update(d)
        return (kind, d)
    if kind == "counts":
        return (kind, (r(5), r(5)))
    if kind == "bc":
        return (kind, 1 + r(6), rng.choice([T.MG_BC_DIRICHLET, T.MG_BC_NEUMANN, T.MG_BC_CONTINUOUS]),
                rng.choice([0.375, -0.5, 1.25, 0.0]))
    return (kind,)


# (tree, seed) of the seeded walks in the order their kinds are dealt: every
# class's deck of kinds, shuffled once, is dealt round and round over the
# class's walks in this order, so that the three seeds between them reach
# every kind the class allows (tests/test_api_walk_host.py checks it)
WALK_SEEDS = (11, 12, 13)
WALK_TREES = dict(TREES, c4_ref2_box16=C4)
DECK_SEED = 2


def walk_steps(tree):
    return 8 if max(parse(WALK_TREES[tree])["domain"]) >= 128 else 14


def _n_other(n_steps):
    return n_steps - (n_steps + 2) // 3


def _deal(tree, seed):
    """The kinds other than cycles of one walk."""
    cls = tree_class(parse(WALK_TREES[tree]))
    deck = allowed_kinds(cls)
    random.Random(DECK_SEED).shuffle(deck)
    pos = 0
    for t in sorted(WALK_TREES):
        if tree_class(parse(WALK_TREES[t])) != cls:
            continue
        for s in WALK_SEEDS:
            n = _n_other(walk_steps(t))
            if (t, s) == (tree, seed):
                return [deck[(pos + i) % len(deck)] for i in range(n)]
            pos += n
    raise KeyError((tree, seed))


def walk(tree, seed, n_steps=None, levels=None):
    """The seeded walk of one tree: in every three steps one, at a drawn
    place, is a cycle (stand-alone with or without the max residual, to a
    drawn level, or FMG); the others are the walk's share of its class's
    kinds with drawn arguments.  levels = (lowest, highest) of the tree."""
    cfg = parse(WALK_TREES[tree])
    n_steps = walk_steps(tree) if n_steps is None else n_steps
    lo, hi = levels
    rng = random.Random(seed)
    meth = {"smoother": cfg["smoother"], "op": cfg["op"], "sub": cfg["bc"] == "per"}
    others = _deal(tree, seed)
    if len(others) < _n_other(n_steps):
        raise ValueError("walk longer than its deal")
    rng.shuffle(others)
    steps = []
    for g in range(0, n_steps, 3):
        size = min(3, n_steps - g)
        at = rng.randrange(size)
        for i in range(size):
            if i == at:
                c = rng.choices([V0, V1, "vcycle_to"], [3, 2, 2])[0]
                steps.append(c if c != "vcycle_to" else _draw(rng, c, cfg, lo, hi, meth))
            else:
                steps.append(_draw(rng, others.pop(), cfg, lo, hi, meth))
    return steps


def tree_levels(args):
    """(lowest, highest) level of a configuration's tree."""
    from tests.mgdriver import build_tree
    t = build_tree(parse(args), T.MGTree())
    return t.lowest_lvl, t.highest_lvl


# -- the directed lists -----------------------------------------------------------
GS, GSRB = {"smoother": "gs"}, {"smoother": "gsrb"}
METHODS_LIST = [V0, ("methods", GS), V0, V1, ("methods", GSRB), V0, V1, ("methods", {"op": "helm", "lam": 3.0}), V0,
                V1, ("methods", {"op": "lpl", "sub": False}), V1, ("methods", {"sub": True}), V0, V1]


def ring_methods_list():
    """METHODS_LIST for the 128 x 256 x 256 register-ring tree (lexicographic
    GS, Dirichlet: subtract_mean off is its own setting), shortened to what
    the oracle runs in a few seconds: every change of methods once, each met
    by one cycle."""
    return [V0, ("methods", GSRB), V0, ("methods", GS), ("methods", {"op": "helm", "lam": 3.0}), V1,
            ("methods", {"op": "lpl", "sub": True}), V0, ("methods", {"sub": False}), V1]


def ring_writers_list(hi):
    """The writers of rhs other than an upload between ring sweeps, each
    followed by two sweeps of the level it wrote (the comparison after the
    sweeps covers rhs too: none after the writer itself, RHS_WRITERS)."""
    sm = ("smooth_boxes", hi, 2)
    # (restrict_lvl writes rhs of the level below the top: that level is swept after it)
    return [V0, ("prolong", hi - 1, 1, 2, 0), sm, ("restrict_lvl", 2, hi), ("smooth_boxes", hi - 1, 2), sm,
            ("apply_op", 2), sm, ("set_rhs", 0.5, -1.25), sm, ("subtract_mean", 2, 0), sm]


RHS_WRITERS = ("prolong", "restrict_lvl", "apply_op", "set_rhs", "subtract_mean")


# -- several ranks: checkpoints as digests ------------------------------------------
def checkpoint(be, out, n, ids_of=None):
    """{(step, lvl, id, iv): sha256 of the box's stored cells} of this rank's
    boxes into out."""
    for lvl in be.levels():
        ids = be.my_ids(lvl)
        if not len(ids):
            continue
        u = ~_stored_mask(be.tree.box_size_lvl[lvl])
        for iv in (1, 2, 3, 4):
            a = np.ascontiguousarray(be.get_level(lvl, iv))
            a[:, u] = 0.0
            for q, id_ in enumerate(ids):
                out[(n, lvl, int(id_), iv)] = hashlib.sha256(a[q].tobytes()).digest()


def run_rank(be, steps, lazy=False):
    """A rank's (or the oracle's) run of a step list: ({step: scalar},
    {(step, lvl, id, iv): digest}); every rank makes the same calls."""
    meth = Methods(be.cfg)
    scalars, boxes = {}, {}
    for n, step in enumerate(steps):
        r = apply_step(be, meth, step)
        if r is not None:
            scalars[n] = r
        if not (lazy and _lazy_skip(step) and n + 1 < len(steps)):
            checkpoint(be, boxes, n)
    return scalars, boxes
