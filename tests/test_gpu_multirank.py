"""Multi-rank parity on one GPU: the golden runs the reference made at 2, 4
and 8 MPI ranks (tests/golden/golden.json), replayed by as many device
contexts exchanging through the loopback transport (include/omg.h,
omg_loopback_unique_id).  Same tree partition (mg_load_balance), same halo /
restriction / prolongation plans and kernels as the RCCL path; the periodic
cases pin the MPICH pairwise order of the get_sum allreduce per rank count."""
import json
import os

import pytest

from tests.mgdriver import OPS, OracleBackend, _cycles, omg, parse, phi_digest, run_loopback, run_problem, \
    run_problem_loopback, setup_problem

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))["configs"]
MULTI = [(n, int(r)) for n, e in sorted(GOLDEN.items()) if not e.get("big") for r in e["runs"] if int(r) > 1]
# the BASELINE C3 configuration itself (512^3, box 16, periodic, GSRB) as the
# reference ran it on 2, 4 and 8 MPI ranks
BIG_MULTI = [(n, int(r)) for n, e in sorted(GOLDEN.items()) if e.get("big") for r in e["runs"] if int(r) > 1]

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _check_collective(monkeypatch):
    """Every multi-rank run here also agrees, over the transport, on the
    decisions the library makes without communication (the stand-alone fill
    skip) and fails if a rank differs (OMG_CHECK_COLLECTIVE)."""
    monkeypatch.setenv("OMG_CHECK_COLLECTIVE", "1")


def _check(out, run):
    """History bit for bit, and the final phi of every box (gathered from its
    owner) against the reference's own per-rank dump where it made one."""
    assert out["history"] == run["history"]
    if "phi_sha256" in run:
        assert out["phi_sha256"] == run["phi_sha256"]
    if "mid_sha256" in run:   # cycle a: what its calls between the cycles wrote
        assert out["mid_sha256"] == run["mid_sha256"]


@pytest.mark.parametrize("name,ranks", MULTI)
def test_multirank_matches_reference_golden(name, ranks):
    e = GOLDEN[name]
    out = run_problem_loopback(e["args"], ranks)
    _check(out, e["runs"][str(ranks)])


# bench.py's replication bound (64 boxes of 16^3) and none: the 8-GPU bench
# configuration, every level's exchange through the same plans RCCL runs
@pytest.mark.parametrize("rep", [0, 64 * 16 ** 3])
@pytest.mark.parametrize("name,ranks", BIG_MULTI)
def test_c3_512_multirank_matches_reference_golden(name, ranks, rep):
    e = GOLDEN[name]
    out = run_problem_loopback(e["args"], ranks, rep_cells=rep)
    _check(out, e["runs"][str(ranks)])


# Replicated coarse levels (omg_set_coarse_replication): every coarse level
# on every rank (1 << 40 cells), or only the smallest ones (4096 cells, so the
# restriction into a replicated level from a distributed one is exercised at
# several box sizes).  Same bits as the reference's distributed coarse levels.
@pytest.mark.parametrize("rep", [1 << 40, 4096])
@pytest.mark.parametrize("name,ranks", MULTI)
def test_multirank_replicated_coarse_matches_golden(name, ranks, rep):
    e = GOLDEN[name]
    out = run_problem_loopback(e["args"], ranks, rep_cells=rep)
    _check(out, e["runs"][str(ranks)])


# Box-16 periodic levels where only the boxes without a face on another rank
# take the fused last down-substep (k_smooth_resid over a box list) and the
# others the unfused substep + residual, with the colour-0 halo unpacked
# while the fused boxes run; per128x64 at 6 ranks leaves ranks 1 and 4 with
# no such box (they stay unfused, their peers fuse).  History against the
# reference, final phi of every box against the oracle at the same rank
# count (the reference dumps phi at one rank only).
FUSED = [("per128_box16_gsrb_v", 2), ("per128_box16_gsrb_v", 8), ("per128x64_box16_mixed", 6)]


@pytest.mark.parametrize("name,ranks", FUSED)
def test_multirank_fused_down_step_phi_matches_oracle(name, ranks):
    e = GOLDEN[name]
    out = run_problem_loopback(e["args"], ranks)
    _check(out, e["runs"][str(ranks)])
    orc = run_problem(e["args"], backend="oracle", n_ranks=ranks)
    assert orc["history"] == out["history"]
    assert out["phi_sha256"] == orc["phi_sha256"]


# The bench's c4_refined configuration (GSRB, box 16, one refined level,
# callback Dirichlet) at 3 and 4 ranks with the bench's coarse replication
# bound (64 boxes of 16^3): refinement boundaries across ranks, history and
# every box's final phi against the reference's own multi-rank runs.
@pytest.mark.parametrize("ranks", [3, 4])
def test_c4_refined_gsrb_bench_replication(ranks):
    e = GOLDEN["c4_ref2_box16_gsrb"]
    out = run_problem_loopback(e["args"], ranks, rep_cells=64 * 16 ** 3)
    _check(out, e["runs"][str(ranks)])


# C2 with lexicographic GS at its own size on 2 and 8 ranks: the register-ring
# sweep and k_fill_tile_xl with faces on other ranks (packed into the halo
# send buffer from the partly staged box).  Dirichlet histories and phi do not
# depend on the rank count (each box reads only ghosts frozen since
# the last fill), so the reference's one-rank run is the expected result.
@pytest.mark.parametrize("ranks", [2, 8])
def test_c2_gs_ring_multirank_matches_reference(ranks):
    e = GOLDEN["c2_256_box16_gs_d0"]
    out = run_problem_loopback(e["args"], ranks)
    _check(out, e["runs"]["1"])


# Round 4: a multi-rank stand-alone V-cycle no longer waits for the GPU on the
# host (round 3 agreed on the fill skip with an all-gather + stream
# synchronisation every cycle).  Dirichlet (no periodic mean, which the
# loopback transport gathers on the host), without max_res: zero waits per
# cycle; with max_res: one (the residual read back, m_multigrid.f90:226-234).
@pytest.mark.parametrize("args,ranks", [("16 64 64 64 3 v gsrb lpl 0 d0 sol 1 lb 0", 2),
                                        ("16 128 128 128 3 v gsrb lpl 0 sol sol 2 lb 0", 4),
                                        ("16 64 64 64 3 v gs lpl 0 d0 sol 1 lb 0", 8)])
def test_multirank_vcycle_makes_no_host_wait(args, ranks, monkeypatch):
    monkeypatch.delenv("OMG_CHECK_COLLECTIVE")   # (its agreement waits on the host by design)

    def body(be, rank, reduce):
        ctx = be.mg.ctx
        omg.mg_fas_vcycle(be.mg)          # the first cycle fills (uploads dropped the ghosts)
        n0 = ctx.host_sync_count()
        for _ in range(3):
            omg.mg_fas_vcycle(be.mg)
        n1 = ctx.host_sync_count()
        omg.mg_fas_vcycle(be.mg, max_res=True)
        n2 = ctx.host_sync_count()
        return n1 - n0, n2 - n1, ctx.comm_stream_priority()

    for no_max, with_max, prio in run_loopback(args, ranks, body):
        assert no_max == 0
        assert with_max == 1
        assert prio < 0   # the highest priority HIP offers (lower is higher)


# Round 6: the multi-substep passes on levels split over ranks (the deep halo,
# omg_plan.cpp plan_deep): the remote boxes the columns read are proxies,
# filled once per pass (phi of the colour read; rhs when it changed, the
# periodic mean subtracted on them like on their owners), and the remote
# faces' ghosts exchanged after it.  The 128^3 tree's 512-box finest level
# takes it with the level bound lowered to one box; every rank must run the
# k_gsrb4 / k_gsrb3 passes there and the deep rounds, and the history and
# every box's final phi must be the reference's at the same rank count.  (C3
# itself at 2/4/8 ranks, test_c3_512_multirank_matches_reference_golden, takes
# it at the default bound: 16384 / 8192 / 4096 boxes per rank on level 1.)
DEEP_STATS = ("smoother_gsrb4@1", "smoother_gsrb3@1", "smoother_gsrb4p@1", "deep_phi@1", "deep_rhs@1",
              "deep_faces@1", "deep_res@0")


@pytest.mark.parametrize("name,ranks", [("per128_box16_gsrb_v", 2), ("per128_box16_gsrb_v", 8)])
def test_deep_halo_multirank_matches_reference(name, ranks, monkeypatch):
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", "1")
    e = GOLDEN[name]
    out = run_problem_loopback(e["args"], ranks, stats=DEEP_STATS)
    _check(out, e["runs"][str(ranks)])
    n_it = parse(e["args"])["n_its"]
    for st in out["stats"]:
        # per cycle: the down pass (k_gsrb4) and the up pass, one phi round
        # each; rhs once (the proxies follow the mean).  The up pass is the
        # correction form (k_gsrb4<PRO 2>) from level 0's res, which level 0
        # (64 boxes, split too) stores with its last pass and sends to its
        # proxies (deep_res)
        assert st["smoother_gsrb4@1"] == n_it and st["smoother_gsrb4p@1"] == n_it, st
        assert st["smoother_gsrb3@1"] == 0 and st["deep_res@0"] == n_it, st
        assert st["deep_phi@1"] == 2 * n_it and st["deep_rhs@1"] == 1 and st["deep_faces@1"] == 2 * n_it, st


# Against the oracle at the same rank count: other smoothing counts (the down
# pass as k_gsrb3 + one-substep launches + the split fused last substep, the
# up passes after k_prolong_smooth), Helmholtz, FMG (rhs rewritten below the
# finest level every cycle), and OMG_NO_DEEP in the same process.
@pytest.mark.parametrize("args,ranks,cycles", [
    ("16 128 128 128 3 v gsrb lpl 0 per sol 1 lb 0", 4, (3, 1)),
    ("16 128 128 128 3 v gsrb lpl 0 per sol 1 lb 0", 2, (1, 3)),
    ("16 128 128 128 3 v gsrb helm 2 per sol 1 lb 0", 4, (2, 2)),
    ("16 128 128 128 3 v gsrb helm 2 per sol 1 lb 0", 8, (4, 4)),
    ("16 128 128 128 2 f gsrb lpl 0 per sol 1 lb 0", 2, (2, 2)),
])
@pytest.mark.parametrize("switch", [None, "OMG_NO_DEEP"])
def test_deep_halo_multirank_matches_oracle(args, ranks, cycles, switch, monkeypatch):
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", "1")
    if switch:
        monkeypatch.setenv(switch, "1")
    out = run_problem_loopback(args, ranks, cycles=cycles, stats=DEEP_STATS)
    cfg = parse(args)
    orc = OracleBackend(cfg, ranks)
    import pyoracle  # on sys.path once OracleBackend exists (checker only)
    orc.o.configure(op=OPS[cfg["op"]], lam=cfg["lam"], smoother=pyoracle.GSRB, n_cycle_down=cycles[0],
                    n_cycle_up=cycles[1], subtract_mean=True)
    setup_problem(orc)
    assert out["history"] == _cycles(orc, cfg)
    assert out["phi_sha256"] == phi_digest(orc)
    deep = sum(st["deep_phi@1"] for st in out["stats"])
    assert (deep == 0) == (switch == "OMG_NO_DEEP"), out["stats"]
