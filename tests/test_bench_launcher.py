"""bench.py's own multi-rank launcher on the CPU: `python bench.py --gpus N`
without torchrun starts N ranks itself (one process each, gloo for the
host-side collectives); with --plan-only every rank builds the bench tree's
plan-only context (OMG_DEVICE_NONE) and the ranks check over gloo that every
transfer pairs up with its peer's, key for key in wire order — the plans the
RCCL halo exchange of the driver's multi-GPU run uses."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, env_extra=None, rc=0):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    assert p.returncode == rc, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]   # rank 0 only
    return json.loads(lines[0])


@pytest.mark.parametrize("n,mode,domain", [(2, "weak", [1024, 512, 512]),
                                           (4, "strong", [512, 512, 512]),
                                           (8, "weak256", [512, 512, 512])])
def test_launcher_spawns_ranks_whose_plans_pair_up(n, mode, domain):
    out = _run("--gpus", str(n), "--mode", mode, "--plan-only")
    assert out["n_ranks"] == n and out["domain"] == domain
    assert [r["rank"] for r in out["ranks"]] == list(range(n))
    assert out["ok"], [r["problems"] for r in out["ranks"]]
    # Morton chunks: every rank owns an equal share of the finest level and
    # exchanges faces with its octant neighbours only
    boxes = {r["boxes_lvl_hi"] for r in out["ranks"]}
    assert len(boxes) == 1
    for r in out["ranks"]:
        assert r["halo_faces_recv_lvl_hi"] > 0 and 1 <= len(r["peers_lvl_hi"]) <= min(3, n - 1)


def test_cpu_baseline_timeout_leaves_no_process(tmp_path):
    """bench.py's cpu_baseline runs each `mpiexec -n P` in a session of its
    own and kills that session's process group on timeout or exit: a
    reference run that hangs leaves no hydra proxy or rank behind (round 3's
    BENCH ended with one stray process: subprocess.run(timeout=...) killed
    mpiexec only)."""
    if not os.path.exists("/opt/conda/bin/mpiexec"):
        pytest.skip("no MPICH mpiexec")
    sys.path.insert(0, ROOT)
    import bench
    marker = "300.%06d" % (os.getpid() % 1000000)
    fake = tmp_path / "fake_ref"
    fake.write_text(f"#!/bin/bash\nsleep {marker} &\nsleep {marker}\n")
    fake.chmod(0o755)

    def alive():
        n = 0
        for pid in os.listdir("/proc"):
            if not pid.isdigit():
                continue
            try:
                with open(f"/proc/{pid}/cmdline", "rb") as f:
                    cmd = f.read().replace(b"\0", b" ").decode(errors="replace")
            except OSError:
                continue
            n += marker in cmd or str(fake) in cmd
        return n

    out = bench.cpu_baseline([16, 16, 16], ref=str(fake), timeout=3, plan=[(2, 1, 1)])
    assert "TimeoutExpired" in out["by_ranks"]["2"]["error"]
    assert out["value"] is None
    import time
    for _ in range(50):   # (SIGKILL is delivered asynchronously)
        if alive() == 0:
            break
        time.sleep(0.1)
    assert alive() == 0


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu():
    """The N > 1 bench path end to end on real hardware before the driver's
    multi-GPU run: `bench.py --gpus 2` on a one-GPU box starts two ranks that
    share the GPU, so the library takes the host transport over the gloo
    group (RCCL refuses two ranks on one device); the line must report two
    GPUs, the host transport and the weak-scaling workload."""
    out = _run("--gpus", "2", "--steps", "2", "--warmup", "1", "--mode", "weak256", "--full", "--no-cpu-baseline",
               "--no-extra")
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["value"] > 0
    assert out["comm"]["transport"] == "host", out["comm"]
    # the self-check before the timed run: C3 at 2 ranks against the
    # reference's own 2-rank history
    assert out["parity"]["ok"] is True and out["parity"]["ranks"] == 2, out["parity"]


@pytest.mark.gpu
def test_bench_parity_mismatch_exits_nonzero():
    """A history that differs from the reference's (one bit flipped by the
    test hook OMG_BENCH_PARITY_CORRUPT) stops the bench before anything is
    timed: exit 3, a line with parity false and no value."""
    out = _run("--gpus", "2", "--mode", "weak256", "--full", "--no-cpu-baseline", "--no-extra",
               env_extra={"OMG_BENCH_PARITY_CORRUPT": "1"}, rc=3)
    assert out["parity"]["ok"] is False and out["parity"]["first_mismatch"] == 3 and out["value"] is None


class _FakeMG:
    """get_level as bench.dump_outputs calls it: n boxes of 16^3 + ghosts."""
    highest_lvl = 3

    def __init__(self, n):
        import numpy as np
        self.phi = np.random.default_rng(5).standard_normal((n, 18, 18, 18))

    def get_level(self, lvl, iv):
        assert lvl == self.highest_lvl
        return self.phi


@pytest.mark.parametrize("n,world,rank", [(700, 1, 0), (700, 4, 3), (40, 1, 0)])
def test_dump_outputs_writes_a_fixed_sample(tmp_path, n, world, rank):
    """--dump-outputs: float64 .npy files, every box's sum and a sample of
    whole boxes that is the same from call to call (seeded), 512 boxes over
    all ranks at the most; ranks of a multi-rank run write files of their own."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    omg = bench.__graft_entry__.load_package()
    mg = _FakeMG(n)
    suffix = f"_rank{rank}" if world > 1 else ""
    got = []
    for d in ("a", "b"):
        bench.dump_outputs(omg, mg, str(tmp_path / d), rank, world)
        files = sorted(os.listdir(tmp_path / d))
        assert files == sorted(f"{k}{suffix}.npy" for k in ("phi_box_sums", "phi_sample", "phi_sample_boxes"))
        got.append({f: np.load(tmp_path / d / f) for f in files})
        assert all(a.dtype == np.float64 for a in got[-1].values())
    assert all(np.array_equal(got[0][f], got[1][f]) for f in got[0])
    sums, sample, boxes = (got[0][f"{k}{suffix}.npy"] for k in ("phi_box_sums", "phi_sample", "phi_sample_boxes"))
    pick = boxes.astype(int)
    assert len(pick) == min(n, 512 // world) and len(set(pick)) == len(pick) and (np.diff(pick) > 0).all()
    assert np.array_equal(sample, mg.phi[pick])
    assert np.array_equal(sums, mg.phi[:, 1:-1, 1:-1, 1:-1].sum(axis=(1, 2, 3)))
    assert bench.DUMP_SAMPLE_BOXES * 18 ** 3 * 8 + 8 * 8 * 512 ** 3 // 16 ** 3 < 64 * 2 ** 20   # C3 at 8 ranks


@pytest.mark.gpu
def test_bench_plain_run_and_dump(tmp_path):
    """A plain run times the steps and nothing else: value and ms_per_step
    agree, no parity / roofline / sub-benchmark / CPU baseline on the line;
    --dump-outputs leaves phi of the last step, its box sums those of the
    sampled boxes."""
    import numpy as np
    out = _run("--gpus", "1", "--steps", "3", "--warmup", "1", "--mode", "weak256", "--dump-outputs", str(tmp_path))
    assert out["steps"] == 3 and out["dtype"] == "f64" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(256 ** 3 / (out["ms_per_step"] * 1e-3), rel=1e-9)
    for key in ("parity", "roofline", "cpu_baseline", "kernels_one_cycle"):
        assert out[key] is None, key
    assert not {"c4_refined", "gs_lex", "c3_strong"} & set(out)
    sums, sample, boxes = (np.load(tmp_path / f"{k}.npy") for k in ("phi_box_sums", "phi_sample", "phi_sample_boxes"))
    assert sums.shape == (16 ** 3,) and sample.shape == (512, 18, 18, 18) and sample.dtype == np.float64
    assert np.isfinite(sample).all() and np.abs(sample).max() > 0.1   # u = prod(sin): phi has converged towards it
    # (two sums of n = 16^3 values, |phi| <= ~1, in possibly different orders: each within n 2^-53 sum|phi| < 2e-9)
    assert np.abs(sample[:, 1:-1, 1:-1, 1:-1].sum(axis=(1, 2, 3)) - sums[boxes.astype(int)]).max() < 4e-9


def test_parity_verdict():
    sys.path.insert(0, ROOT)
    import bench
    h = [{"it": i, "err": "%016X" % i, "res": "0", "max_res": "0"} for i in range(4)]
    assert bench.parity_verdict(h, [dict(x) for x in h]) == {"ok": True, "first_mismatch": None}
    g = [dict(x) for x in h]
    g[2]["res"] = "1"
    assert bench.parity_verdict(h, g) == {"ok": False, "first_mismatch": 2}
    assert bench.parity_verdict(h[:3], h) == {"ok": False, "first_mismatch": 3}
