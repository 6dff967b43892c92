"""Free-space boundary conditions on the GPU (omg_poisson_free_3d: the
Green's function, the hipFFT solve, the boundary table and the multigrid
cycle in libomg.so) against the reference's own results
(tests/golden/free_golden.json, PSolver's output in tests/golden/*_phi.npy)
and against the CPU oracle, within the round-off tolerance of
tests/freedriver.py (the transforms sum in another order than PSolver)."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import freedriver as FD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "free_golden.json")))["configs"]

pytestmark = pytest.mark.gpu

_ORACLE_RUNS = {}


def _oracle(name):
    """run_oracle of a golden entry (CPU), computed once per module and never
    modified."""
    if name not in _ORACLE_RUNS:
        _ORACLE_RUNS[name] = FD.run_oracle(GOLDEN[name]["args"])
    return _ORACLE_RUNS[name]


def _worst(got, ref, mask=None):
    """max |got - ref| over the cells of mask (all cells if None)."""
    d = np.abs(got - ref)
    return float(np.max(d[..., mask] if mask is not None else d))


def _highest_xyz(mg, phi):
    """[box, k, j, i] of the highest level (my_ids order) -> [x, y, z]."""
    lvl = mg.highest_lvl
    nc = mg.box_size_lvl[lvl]
    dom = np.max(mg.ix[mg.lvls[lvl].ids], axis=0) * nc
    out = np.zeros(dom)
    for n, id_ in enumerate(mg.lvls[lvl].my_ids):
        p = (mg.ix[id_] - 1) * nc
        out[p[0]:p[0] + nc, p[1]:p[1] + nc, p[2]:p[2] + nc] = phi[n, 1:-1, 1:-1, 1:-1].transpose(2, 1, 0)
    return out


@pytest.mark.parametrize("name", ["free16_fftonly", "free24x16_fftonly", "free16a_fftonly",
                                  "free24x16a_fftonly"])
def test_fft_solve_matches_reference_psolver(name):
    """The FFT level is the highest: phi is the device's Green's-function
    solve itself, against PSolver's output on the interiors, and against the
    oracle's guess on every stored cell: the face ghosts k_free_guess writes
    (m_free_space.f90:176-183) as well.  On the off-centre layouts this pins
    the axis order of k_free_gather and k_free_guess and the mirror images of
    k_free_karray, which the centred charge cannot see."""
    e = GOLDEN[name]
    cfg = FD.parse(e["args"])
    tol = FD.tolerances(cfg)["phi_abs"]
    out = FD.run_device(e["args"])
    ref = np.load(os.path.join(ROOT, "tests", "golden", e["phi_npy"]))
    got = _highest_xyz(out["mg"], out["phi"])
    d = float(np.max(np.abs(got - ref)))
    print(name, "phi interior - PSolver:", d, "tol", tol)
    assert d <= tol, d
    orc = _oracle(name)
    assert np.max(np.abs(orc["phi"])) > 0.01     # the comparison below is of real data
    dg = _worst(out["phi"], orc["phi"], FD.stored_mask(cfg["box"]))
    print(name, "phi stored cells - oracle:", dg, "tol", tol)
    assert dg <= tol, dg
    FD.compare_history(out["history"], FD.golden_history(e), cfg, name)


@pytest.mark.parametrize("name", ["free32b_f", "free48x32b_f", "free32b_lowest_f"])
def test_boundary_planes_match_oracle(name):
    """omg_free_planes after the first call against the oracle's six planes
    (m_free_space.f90:163-171), each plane on its own: k_free_planes' low and
    high sides, its index order and the ABI's layout, on planes that differ
    from their opposite and from their transpose."""
    e = GOLDEN[name]
    cfg = FD.parse(e["args"])
    tol = FD.tolerances(cfg)["phi_abs"]
    orc = _oracle(name)
    d = FD._Device(cfg)
    d.step(cfg, 1)
    lvl, nx, planes = FD.device_planes(d.mg)
    assert lvl == orc["fft_lvl"] and nx == orc["nx"], (lvl, nx, orc["fft_lvl"], orc["nx"])
    for n in range(6):
        assert planes[n].shape == orc["planes"][n].shape, ("plane", n + 1)
        dn = _worst(planes[n], orc["planes"][n])
        print(name, "plane", n + 1, "device - oracle:", dn, "tol", tol)
        assert dn <= tol, ("plane", n + 1, dn)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_free_space_matches_reference_history(name):
    """Every iteration of the reference's test_free_space set-up (max error,
    rms error, max_res) within the stated tolerance, one GPU."""
    e = GOLDEN[name]
    out = FD.run_device(e["args"])
    FD.compare_history(out["history"], FD.golden_history(e), FD.parse(e["args"]), name)


@pytest.mark.parametrize("name", ["free64_box8_f", "free48x32_f", "free64_lowest_f"])
def test_free_space_final_phi_matches_oracle(name):
    """The final phi of the highest level, device against the CPU oracle."""
    e = GOLDEN[name]
    cfg = FD.parse(e["args"])
    dev = FD.run_device(e["args"])
    orc = FD.run_oracle(e["args"])
    d = float(np.max(np.abs(dev["phi"][:, 1:-1, 1:-1, 1:-1] - orc["phi"][:, 1:-1, 1:-1, 1:-1])))
    assert d <= FD.tolerances(cfg)["phi_abs"], d


@pytest.mark.parametrize("name,ranks", [("free64_box8_f", 2), ("free64_box8_f", 4), ("free64_box16_f", 2),
                                        ("free128_box16_f", 4), ("free32_fftonly", 2)])
def test_free_space_multirank_matches_reference(name, ranks):
    """Several ranks through the loopback transport: the FFT level's rhs is
    gathered on every rank, each solves the same grid, the boundary table
    covers its own boxes; the reference's run at that rank count."""
    e = GOLDEN[name]
    out = FD.run_device_loopback(e["args"], ranks)
    _assert_ranks_agree_on_reduced_history(out)
    FD.compare_history(out["history"], FD.golden_history(e, ranks), FD.parse(e["args"]), name)


def _assert_ranks_agree_on_reduced_history(out):
    """What must hold between the ranks whatever the data: every rank solved
    the same FFT grid with the same plan, so its six planes are rank 0's bit
    for bit; max_res is each rank's own all-reduce, so the histories (whose
    errors are reduced from the ranks' own, kept in out["ranks"]) are equal."""
    R = out["ranks"]
    for r, m in enumerate(R):
        assert (m["fft_lvl"], m["nx"]) == (R[0]["fft_lvl"], R[0]["nx"]), ("rank", r)
        for n in range(6):
            assert np.array_equal(m["planes"][n], R[0]["planes"][n]), \
                ("rank", r, "plane", n + 1, _worst(m["planes"][n], R[0]["planes"][n]))
    for r, h in enumerate(out["all"]):
        assert h == out["all"][0], ("rank", r)
    for n, h in enumerate(out["history"]):
        assert h["err"] == max(m["errs"][n][0] for m in R), ("it", n + 1)


@pytest.mark.parametrize("name,ranks", [("free32b_f", 2), ("free32b_f", 4), ("free64b_box16_f", 2),
                                        ("free64b_box16_f", 4), ("free16a_fftonly", 2)])
def test_free_space_multirank_per_rank_stages(name, ranks):
    """Several loopback ranks on the off-centre layouts, every rank checked
    on its own and stage by stage against one oracle run, so that a wrong
    result names the rank and the stage:
    1. its planes against the oracle's (the gather, the exchange, the scatter
       and the FFT solve of that rank);
    2. its planes bit for bit against rank 0's (the same grid, the same plan);
    3. phi of its FFT-level boxes after the first call against the oracle's,
       where no cycle runs (k_free_guess on its own boxes);
    4. its own max error per iteration against the oracle's over its boxes;
    5. the reduced history against the reference's at that rank count."""
    e = GOLDEN[name]
    cfg = FD.parse(e["args"])
    tol = FD.tolerances(cfg)
    orc = _oracle(name)
    tree = orc["tree"]
    out = FD.run_device_loopback(e["args"], ranks)
    R = out["ranks"]
    hl = tree.highest_lvl
    pos_hl = {int(i): n for n, i in enumerate(tree.lvls[hl].ids)}
    pos_fft = {int(i): n for n, i in enumerate(tree.lvls[orc["fft_lvl"]].ids)}
    assert sorted(i for m in R for i in m["hl_ids"]) == sorted(pos_hl)      # every box on one rank
    assert sorted(i for m in R for i in m["fft_ids"]) == sorted(pos_fft)
    failures = []
    for r, m in enumerate(R):
        if (m["fft_lvl"], m["nx"]) != (orc["fft_lvl"], orc["nx"]):
            failures.append(("rank", r, "grid", m["fft_lvl"], m["nx"]))
            continue
        for n in range(6):
            dn = _worst(m["planes"][n], orc["planes"][n])
            print(name, ranks, "rank", r, "plane", n + 1, "device - oracle:", dn, "tol", tol["phi_abs"])
            if not dn <= tol["phi_abs"]:
                failures.append(("rank", r, "stage 1: plane - oracle", n + 1, dn))
            if not np.array_equal(m["planes"][n], R[0]["planes"][n]):
                failures.append(("rank", r, "stage 2: plane != rank 0's", n + 1,
                                 _worst(m["planes"][n], R[0]["planes"][n])))
        if orc["fft_lvl"] == hl and m["fft_ids"]:
            sel = [pos_fft[i] for i in m["fft_ids"]]
            dg = _worst(m["phi_fft_1"], orc["phi_fft_1"][sel], FD.stored_mask(tree.box_size_lvl[hl]))
            print(name, ranks, "rank", r, "FFT-level phi - oracle:", dg, "tol", tol["phi_abs"])
            if not dg <= tol["phi_abs"]:
                failures.append(("rank", r, "stage 3: FFT-level phi - oracle", dg))
        sel = [pos_hl[i] for i in m["hl_ids"]]
        for it, (err, _) in enumerate(m["errs"]):
            want = float(np.max(orc["box_err"][it][0][sel])) if sel else 0.0
            print(name, ranks, "rank", r, "it", it + 1, "err - oracle:", abs(err - want), "tol", tol["err_abs"])
            if not abs(err - want) <= tol["err_abs"]:
                failures.append(("rank", r, "stage 4: max err, iteration", it + 1, err, want))
    assert not failures, failures
    _assert_ranks_agree_on_reduced_history(out)
    FD.compare_history(out["history"], FD.golden_history(e, ranks), cfg, name)


def test_free_space_replicated_fft_level():
    """The FFT level replicated on every rank (omg_set_coarse_replication):
    the rhs is gathered locally, no exchange."""
    e = GOLDEN["free64_box8_f"]
    out = FD.run_device_loopback(e["args"], 2, rep_cells=40000)
    FD.compare_history(out["history"], FD.golden_history(e, 2), FD.parse(e["args"]), "replicated")


def test_first_call_needs_new_rhs():
    cfg = FD.parse("8 32 32 32 1 0.15 f")
    d = FD._Device(cfg)
    with pytest.raises(RuntimeError, match="first call requires new_rhs"):
        FD.omg.mg_poisson_free_3d(d.mg, False, 0.15, True)


def test_laplacian_required():
    cfg = FD.parse("8 32 32 32 1 0.15 f")
    d = FD._Device(cfg)
    d.mg.operator_type = FD.T.MG_HELMHOLTZ
    with pytest.raises(RuntimeError, match="laplacian operator required"):
        FD.omg.mg_poisson_free_3d(d.mg, True, 0.15, True)
    # the C-ABI refuses it too (the device's operator, not the host's flag)
    FD.omg.helmholtz_set_lambda(d.mg, 1.0)
    FD.omg.mg_set_methods(d.mg)
    m = ctypes.c_double(0.0)
    with pytest.raises(FD.omg.device.OmgError, match="laplacian operator required"):
        d.mg.ctx.call("poisson_free_3d", 1, 0.15, 1, 1, ctypes.byref(m), np.zeros(3), None)


@pytest.mark.parametrize("name", ["free64_box8_f", "free32b_f", "free48x32b_f"])
def test_boundary_callback_reproduces_device_table(name):
    """After the solve, the host callback installed in mg.bc (the planes
    copied back) tabulates exactly the values the device stored: pushing it
    again and re-running the cycle changes nothing.  The callback is pinned
    to the oracle's interp_bc on the CPU, so on planes that differ from their
    opposite and their transpose, and with an origin whose components all
    differ, this is a bitwise test of k_free_bc_faces and FreePlaneGeom."""
    e = GOLDEN[name]
    cfg = FD.parse(e["args"])
    d = FD._Device(cfg)
    d.step(cfg, 1)
    a = d.step(cfg, 2)
    phi_a = d.mg.get_level(d.mg.highest_lvl, 1)
    d2 = FD._Device(cfg)
    d2.step(cfg, 1)
    d2.mg.push_bc([1])
    FD.omg.mg_phi_bc_store(d2.mg)
    b = d2.step(cfg, 2)
    phi_b = d2.mg.get_level(d2.mg.highest_lvl, 1)
    assert a == b
    assert np.array_equal(phi_a, phi_b)


@pytest.mark.parametrize("name", ["free32b_f", "free48x32b_f"])
def test_free_space_every_level_matches_oracle(name):
    """Every stored cell of phi (interiors and face ghosts) on every level
    after the last iteration against the oracle.  A physical ghost is
    2 bc - interior, so it carries the plane's round-off twice and the
    interior's once: 3 * phi_abs."""
    e = GOLDEN[name]
    cfg = FD.parse(e["args"])
    tol = 3 * FD.tolerances(cfg)["phi_abs"]
    orc = _oracle(name)
    dev = FD.run_device(e["args"])
    mg = dev["mg"]
    assert (mg.lowest_lvl, mg.highest_lvl) == (orc["tree"].lowest_lvl, orc["tree"].highest_lvl)
    for lvl in range(mg.lowest_lvl, mg.highest_lvl + 1):
        assert list(mg.lvls[lvl].my_ids) == list(orc["tree"].lvls[lvl].ids)
        d = _worst(mg.get_level(lvl, FD.T.MG_IPHI), orc["phi_lvls"][lvl], FD.stored_mask(mg.box_size_lvl[lvl]))
        print(name, "level", lvl, "phi stored cells - oracle:", d, "tol", tol)
        assert d <= tol, ("level", lvl, d)
