"""Smoothing counts and coarse-solve limits other than the defaults.

The reference reads mg%n_cycle_down, n_cycle_up, max_coarse_cycles and
residual_coarse_abs / _rel afresh every cycle (m_multigrid.f90:187,203-207,
223), so they may change between cycles, and a count of 0 is a zero-trip loop.
fas_vcycle (octree-mg_amd/csrc/omg_cycle.cpp) chooses its kernels by the counts:
k_gsrb4 down passes where the substeps are a multiple of four, k_smooth_resid
where there is a last down substep to fuse, k_gsrb3 / k_gsrb4's correction
forms where the up-smoothing has three / four substeps, an even number of ring
sweeps without a fill in between, and ghosts deferred after a cycle that ends
in k_gsrb4's correction form.  Here:

a. the reference's own runs at such counts (tests/golden/golden.json, cyc_*)
   with the block passes' level bound lowered, history and final phi;
b. counts changed between cycles, every stored cell of phi, rhs, old and res
   against the C oracle after each step: the sequence that left deferred
   ghosts unread-but-unwritten (a cycle that defers, then n_cycle_down = 0),
   its mirror, and seeded walks over cycles, FMG, count changes and the other
   readers of phi's ghosts;
c. the coarse solve's cap and relative tolerance changed between cycles, on a
   tree whose coarse levels run in the single-workgroup tail and on one whose
   coarse solve runs level by level from the host (vlpl);
d. the launches of the top level in the steady state of back-to-back cycles.

Every comparison is bitwise."""
import json
import os
import random

import pytest

from tests.apiwalk import Pair, _assert_same, _stored_mask  # noqa: F401  (the walk vocabulary lives there)
from tests.mgdriver import SOLVER_DEFAULTS, DeviceBackend, _cycles, hexbits, measure, parse, phi_digest, setup_problem

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))["configs"]

# OMG_BLOCK3_MIN_BOXES[-colOMG_BLOCK3_COLUMN], as tests/test_gpu_block3.py: at
# 512 the 128^3 trees' finest level alone takes the block passes, at 64 the
# 64-box level below it too (its last up pass stores res, the finest level's
# correction is then k_gsrb4's form, which defers the ghosts)
BOUNDS = ["512", "64", "64-col8"]


def _set_bound(monkeypatch, param):
    bound, _, col = param.partition("-col")
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", bound)
    if col:
        monkeypatch.setenv("OMG_BLOCK3_COLUMN", col)
    else:
        monkeypatch.delenv("OMG_BLOCK3_COLUMN", raising=False)
    return int(bound)


# -- a. the reference's runs, block passes under the lowered level bounds ------
BLOCK_GOLDENS = ["cyc_per128_box16_0_2", "cyc_per128_box16_4_2", "cyc_per128_box16_2_4", "cyc_per128_box16_1_1",
                 "cyc_per128_box16_2_3", "cyc_mx1_128_box16_0_2", "cyc_mx1_128_box16_4_1",
                 "cyc_mx1_96x128x64_0_2", "cyc_mx1_96x128x64_4_1"]
PASSES = ("smoother_gsrb3", "smoother_gsrb4", "smoother_gsrb3r", "smoother_gsrb3p", "smoother_gsrb4p")


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("name", BLOCK_GOLDENS)
def test_block_passes_match_reference_at_other_counts(monkeypatch, name, bound):
    """History and final phi of the reference's run.  The launch counts show
    which form served the finest level: a block pass holds three or four
    consecutive substeps of one smoothing leg, so it runs where a leg has at
    least three (down or up >= 2: every case here with down + up >= 2 but
    1:1, whose legs have two substeps each and take none)."""
    min_boxes = _set_bound(monkeypatch, bound)
    e = GOLDEN[name]
    cfg = parse(e["args"])
    dev = DeviceBackend(cfg)
    setup_problem(dev)
    dev.mg.ctx.call("set_profiling", 1)
    hist = _cycles(dev, cfg, None)
    dev.mg.ctx.call("synchronize")
    run = e["runs"]["1"]
    assert hist == run["history"]
    assert phi_digest(dev) == run["phi_sha256"]
    top = dev.tree.highest_lvl
    n = {f: dev.mg.ctx.kernel_stats(f"{f}@{top}")[0] for f in PASSES}
    print(name, bound, n)
    down, up = cfg["cycles"]
    if len(dev.my_ids(top)) >= min_boxes:
        if max(down, up) >= 2:
            assert sum(n.values()) > 0, n
        else:
            assert sum(n.values()) == 0, n
    # the same cycles back to back: the history's downloads fill deferred
    # ghosts after every cycle, here each cycle meets what the last one left
    dev = DeviceBackend(cfg)
    setup_problem(dev)
    for _ in range(cfg["n_its"]):
        dev.vcycle(cfg["maxres"])
    err, res = measure(dev)
    last = run["history"][-1]
    assert (hexbits(err), hexbits(res)) == (last["err"], last["res"])
    assert phi_digest(dev) == run["phi_sha256"]


def test_default_level_bound_at_other_counts(monkeypatch):
    """256^3: the 4096-box finest level takes the passes at the default bound."""
    monkeypatch.delenv("OMG_BLOCK3_MIN_BOXES", raising=False)
    monkeypatch.delenv("OMG_BLOCK3_COLUMN", raising=False)
    e = GOLDEN["cyc_per256_box16_0_2"]
    cfg = parse(e["args"])
    dev = DeviceBackend(cfg)
    setup_problem(dev)
    dev.mg.ctx.call("set_profiling", 1)
    hist = _cycles(dev, cfg, None)
    dev.mg.ctx.call("synchronize")
    assert hist == e["runs"]["1"]["history"]
    assert phi_digest(dev) == e["runs"]["1"]["phi_sha256"]
    top = dev.tree.highest_lvl
    n = {f: dev.mg.ctx.kernel_stats(f"{f}@{top}")[0] for f in PASSES}
    assert sum(n.values()) >= cfg["n_its"], n


# -- b. counts changed between cycles -----------------------------------------
PER128 = "16 128 128 128 1 v gsrb lpl 0 per sol 1 lb 0"
V0, V1 = ("vcycle", False), ("vcycle", True)


@pytest.mark.parametrize("bound", BOUNDS)
def test_deferred_ghosts_then_no_down_smoothing(monkeypatch, bound):
    """Two cycles without the max residual at (2, 2) leave the finest level's
    ghosts deferred (bounds of 64: k_gsrb4's correction form); the next cycle
    has n_cycle_down = 0, so nothing smooths before update_coarse's residual
    reads them."""
    _set_bound(monkeypatch, bound)
    p = Pair(PER128)
    p.set(cycles=(2, 2))
    p.run([V0, V0, ("counts", (0, 2)), V0], lazy=True)   # (no download before the last step's)
    p.run([V1])


@pytest.mark.parametrize("bound", BOUNDS)
def test_deferred_ghosts_then_no_up_smoothing(monkeypatch, bound):
    """The mirror: deferred ghosts, then (2, 0): the down pass consumes the
    deferral, and the up leg corrects and fills without a substep after."""
    _set_bound(monkeypatch, bound)
    p = Pair(PER128)
    p.set(cycles=(2, 2))
    p.run([V0, V0, ("counts", (2, 0)), V0], lazy=True)
    p.run([V1])


KINDS = [V0, V1, ("fmg",), ("counts",), ("apply_op",), ("fill",), ("upload",)]
WEIGHTS = [3, 2, 1, 3, 1, 1, 1]   # (mostly cycles and count changes: each change should meet a cycle)


def _walk(seed, n_steps=12):
    rng = random.Random(seed)
    steps = []
    for _ in range(n_steps):
        k = rng.choices(KINDS, WEIGHTS)[0]
        steps.append(("counts", (rng.randrange(5), rng.randrange(5))) if k == ("counts",) else k)
    return steps


WALK_TREES = {"per128_box16": PER128,
              "mx2_helm64_box16": "16 64 64 64 1 v gsrb helm 2 mx2 sol 1 lb 0",
              "per32_box8": "8 32 32 32 1 v gsrb lpl 0 per sol 1 lb 0",
              "ref3_gs_box8": "8 32 32 32 1 v gs lpl 0 sol sol 3 lb 0"}


# (seeds whose walks run a cycle after every change of the counts and draw a
# count of 0 on either leg)
@pytest.mark.parametrize("seed", [5, 7, 8])
@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("tree", sorted(WALK_TREES))
def test_walk_over_counts_matches_oracle(monkeypatch, tree, lazy, seed):
    """12 seeded steps, each a cycle with or without the max residual, an FMG
    cycle with a guess, new counts from {0..4}^2, mg_apply_op into res, a fill
    of phi, or an upload of phi; full state after every step, and the same
    walk again with deferred ghosts left to the next step (Pair.run's lazy)."""
    _set_bound(monkeypatch, "64")
    p = Pair(WALK_TREES[tree])
    p.run(_walk(seed), lazy)


def test_negative_count_is_no_smoothing(monkeypatch):
    """omg_set_smoother stores a negative count as 0 (include/omg.h): (-1, 2)
    on the device is the oracle's (0, 2)."""
    _set_bound(monkeypatch, "64")
    p = Pair("8 32 32 32 1 v gsrb lpl 0 d0 sol 1 lb 1")
    p.set(cycles=(-1, 2), oracle_cycles=(0, 2))
    p.run([V1, V0, V1])


# -- c. coarse limits changed between cycles ----------------------------------
COARSE_TREES = {"tail": "8 32 32 32 1 v gsrb lpl 0 d0 sol 1 lb 1",
                "host_loop_vlpl": "8 32 32 32 1 v gs vlpl 0 d0 sol 1 lb 1"}
DEFAULT_COARSE = SOLVER_DEFAULTS[2:]


@pytest.mark.parametrize("limit", [(1, 1e-8, 1e-8), (1000, 1e-8, 0.5)], ids=["cap1", "rel0.5"])
@pytest.mark.parametrize("tree", sorted(COARSE_TREES))
def test_coarse_limits_changed_between_cycles(tree, limit):
    p = Pair(COARSE_TREES[tree])
    p.set(coarse=limit)
    p.run([V1, V0])
    p.set(coarse=DEFAULT_COARSE)
    p.run([V1, V0])
    p.set(coarse=limit)
    p.run([V1])


# -- d. the steady state of back-to-back cycles --------------------------------
STEADY = {"subtract": 0, "fill_gc": 0, "residual": 0, "smoother_gsrb": 0, "smoother_gsrb4": 1,
          "smoother_gsrb4p": 1, "resid_restrict": 1}


def test_steady_state_launches_on_the_top_level(monkeypatch):
    """Stand-alone cycles at (2, 2) without the max residual, back to back:
    from the third on, everything a cycle leaves unwritten (the phi mean, the
    rhs shifts, the top level's res and ghost faces) is taken up by the next
    cycle's own passes, so the top level sees one k_gsrb4 down pass, one
    residual + restriction and one k_gsrb4 correction pass per cycle, and
    no launch that writes any of it out."""
    _set_bound(monkeypatch, "64")
    cfg = parse(PER128)
    cfg["cycles"] = (2, 2)
    dev = DeviceBackend(cfg)
    setup_problem(dev)
    ctx = dev.mg.ctx
    for _ in range(2):
        dev.vcycle(False)
    ctx.call("synchronize")
    ctx.call("set_profiling", 1)
    top = dev.tree.highest_lvl
    for cycle in (3, 4):
        ctx.call("reset_stats")
        dev.vcycle(False)
        ctx.call("synchronize")
        n = {f: ctx.kernel_stats(f"{f}@{top}")[0] for f in STEADY}
        print("cycle", cycle, n)
        assert n == STEADY, (cycle, n)
