"""The C oracle (oracle/liboracle.so) against the reference's own outputs.

tests/golden/golden.json was produced by running the REFERENCE octree-mg
(compiled from its Fortran sources, amdflang -O2, MPICH) through
oracle/omg_golden.f90 — see tests/golden/make_golden.py.  Every per-iteration
scalar and the sha256 of the final phi of every box must match bit-for-bit,
including the periodic runs at 2/4/8 ranks, which pin the order of the
per-rank get_sum + MPI_Allreduce(sum) (src/m_multigrid.f90:254-256).
"""
import json
import os

import pytest

from tests.mgdriver import run_problem

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))["configs"]
# "big" entries (the bench's 512^3 configuration) are checked against the
# device only: the C oracle would take minutes and ~7 GB here
# (custom_rb entries: a refinement_bnd callback the oracle does not restate;
# the device and the Fortran drop-in are held to them)
CASES = [(n, r) for n, e in GOLDEN.items() if not e.get("big") and not e.get("custom_rb") for r in e["runs"]]


def test_golden_histories_are_finite():
    """Every recorded scalar is a finite double (a reference run that diverged
    would pin nothing)."""
    import math
    import struct
    for name, e in GOLDEN.items():
        for r, run in e["runs"].items():
            for h in run["history"]:
                for k in ("err", "res", "max_res"):
                    v = struct.unpack("<d", struct.pack("<Q", int(h[k], 16)))[0]
                    assert math.isfinite(v), (name, r, h["it"], k, h[k])


# The coarse solve's limits (max_coarse_cycles, residual_coarse_rel / _abs)
# pin something only where they end the coarse loop earlier than the defaults
# do: the reference's runs of one problem under each limit must differ.
@pytest.mark.parametrize("names", [("cyc_coarse_cap1", "cyc_coarse_cap3", "cyc_coarse_default"),
                                   ("cyc_coarse_rel", "cyc_coarse_abs", "cyc_coarse_default"),
                                   ("cyc_coarse_gs_rel", "cyc_coarse_gs_default"),
                                   ("cyc_coarse_vlpl_gs_cap2", "cyc_coarse_vlpl_gs_default")])
def test_coarse_limits_bind_in_the_reference(names):
    from tests.mgdriver import parse
    problems = {tuple(GOLDEN[n]["args"].split()[:6] + GOLDEN[n]["args"].split()[7:]) for n in names}
    smoothers = {parse(GOLDEN[n]["args"])["smoother"] for n in names}
    assert len(problems) == 1 and len(smoothers) == 1   # the same problem, only the limits differ
    digests = [GOLDEN[n]["runs"]["1"]["phi_sha256"] for n in names]
    assert len(set(digests)) == len(names), dict(zip(names, digests))


@pytest.mark.parametrize("name,ranks", CASES, ids=[f"{n}-r{r}" for n, r in CASES])
def test_oracle_matches_reference(name, ranks):
    e = GOLDEN[name]
    run = e["runs"][ranks]
    out = run_problem(e["args"], backend="oracle", n_ranks=int(ranks))
    assert out["history"] == run["history"]
    assert out.get("error") == run.get("error")
    if "phi_sha256" in run:
        assert out["phi_sha256"] == run["phi_sha256"]
    if "rhs_sha256" in run:   # aniso operator pinned through rhs = L(u)
        assert out["rhs_sha256"] == run["rhs_sha256"]
    if "mid_sha256" in run:   # cycle a: what its calls between the cycles wrote
        assert out["mid_sha256"] == run["mid_sha256"]


# Cycle a's calls between the cycles (mg_restrict_lvl of rhs, mg_prolong into
# old without adding, mg_fill_ghost_cells_lvl of res) show in nothing a cycle
# prints or leaves in phi; mid_sha256 is what pins them.  Each of them left
# out must change it.
@pytest.mark.parametrize("skipped", ["restrict_lvl", "prolong", "fill_ghost_cells_lvl"])
@pytest.mark.parametrize("name", ["api_per32_box8", "api_ref3_gs_box8"])
def test_api_script_calls_show_in_the_golden(monkeypatch, name, skipped):
    from tests.mgdriver import OracleBackend
    call = OracleBackend.call
    monkeypatch.setattr(OracleBackend, "call", lambda self, fn, *a: None if fn == skipped else call(self, fn, *a))
    e = GOLDEN[name]
    out = run_problem(e["args"], backend="oracle")
    assert out["mid_sha256"] != e["runs"]["1"]["mid_sha256"]
