"""omg_get_dense_grad on the GPU: the central differences of a variable over the
boxes and their ghost cells, as dense device tensors.

The expected values never come from the code under test: they are numpy's
(a - b) * f, f = (0.5 * scale) / dr, on the (nc+2)^3 boxes that get_level
returns after mg_fill_ghost_cells_lvl, laid into the level's grid with
tests/denseutil.py.  Every comparison is on bits (int64 views), the sign of
zero included: one subtraction and one multiplication have no tolerance.

1. every level of six trees (boxes of 16, 8, 5, 6, 4, 3 and 2 cells; periodic,
   physical, refinement-boundary faces), phi and rhs, three scales, the tile
   kernel and the per-cell kernel;
2. windows: whole, cut, reaching outside, strided, 8 B off a 16-B boundary,
   component masks;
3. fill: stale ghosts used as they stand or filled first; rhs after
   mg_phi_bc_store;
4. the lazy state two stand-alone cycles leave;
5. stream ordering without a host wait;
6. two loopback ranks and a replicated coarse level;
7. errors before any launch."""
import numpy as np
import pytest
import torch

from tests import denseutil as U
from tests.apiwalk import PER128
from tests.mgdriver import DeviceBackend, T, omg, parse, phi_digest, run_loopback, setup_problem

pytestmark = pytest.mark.gpu

IPHI, IRHS = 1, 2
DIR16 = "16 32 32 32 1 v gsrb lpl 0 d0 sol 1 lb 0"    # 8 boxes, each with three physical faces
BOX5 = "5 10 10 10 1 v gsrb lpl 0 d0 sol 1 lb 0"      # odd box size (denseutil.odd_box_tree)
BOX6 = "6 12 12 12 1 v gs lpl 0 d0 sol 1 lb 0"        # its coarsest level has one 3^3 box
WIN16 = "16 32 32 32 1 v gsrb lpl 0 per sol 1 lb 0"
STREAM64 = "16 64 64 64 1 v gsrb lpl 0 per sol 1 lb 0"
TREES = {"uniform": U.UNIFORM, "dirichlet16": DIR16, "noncube": U.NONCUBE, "refined": U.REFINED, "box5": BOX5,
         "box6": BOX6}
SIZES = {"uniform": {8, 4, 2}, "dirichlet16": {16, 8, 4, 2}, "noncube": {8, 4, 2}, "refined": {8, 4, 2},
         "box5": {5}, "box6": {6, 3}}
SCALES = (1.0, -1.0, 0.37)


def _switch(monkeypatch, generic):
    if generic:
        monkeypatch.setenv("OMG_DENSE_GENERIC", "1")
    else:
        monkeypatch.delenv("OMG_DENSE_GENERIC", raising=False)


def _backend(args, profile=True):
    cfg = parse(args)
    be = U.OddBoxBackend(cfg) if cfg["box"] % 2 else DeviceBackend(cfg)
    if args == DIR16:   # Dirichlet faces of non-zero value, another one per face
        for nb in range(1, 7):
            be.mg.bc[nb][IPHI] = omg.BC(T.MG_BC_DIRICHLET, 0.25 * nb - 0.6)
        be.mg.push_bc([IPHI])
    if profile:
        be.mg.ctx.call("set_profiling", 1)
    return be


def _random_boxes(rng, n, nc):
    """Random boxes, ghosts included, with a slab of one value: differences
    that are exactly zero (-0.0 under a negative scale)."""
    a = rng.standard_normal((n, nc + 2, nc + 2, nc + 2))
    a[:, :, :, : (nc + 2) // 2] = 1.5
    return a


def _sentinel(shape):
    return torch.full(tuple(shape), int(U.SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)


def _launches(be, name):
    be.mg.ctx.call("synchronize")
    return be.mg.ctx.kernel_stats(name)[0]


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def numpy_grad(tree, lvl, ids, boxes, scale):
    """int64 bits [3, nz, ny, nx] of the level's grid: (cc(+1) - cc(-1)) * f on
    the boxes [box, k, j, i] (ghosts as they are), SENTINEL where no box is."""
    nc = tree.box_size_lvl[lvl]
    dr = np.asarray(tree.dr[lvl], dtype=np.float64)
    s = slice(1, nc + 1)
    out = []
    for d, (hi, lo) in enumerate([((s, s, slice(2, nc + 2)), (s, s, slice(0, nc))),
                                  ((s, slice(2, nc + 2), s), (s, slice(0, nc), s)),
                                  ((slice(2, nc + 2), s, s), (slice(0, nc), s, s))]):
        f = (0.5 * float(scale)) / float(dr[d])
        g = np.zeros_like(boxes)
        g[:, s, s, s] = (boxes[(slice(None),) + hi] - boxes[(slice(None),) + lo]) * f
        out.append(U.assemble(tree, lvl, ids, g, U.SENTINEL))
    return np.stack(out)


def _crop(full, lo, n, m=8):
    """The window (lo, n) of [3, nz, ny, nx] bits, SENTINEL outside the grid."""
    _, nz, ny, nx = full.shape
    big = np.full((3, nz + 2 * m, ny + 2 * m, nx + 2 * m), U.SENTINEL, dtype=np.int64)
    big[:, m:-m, m:-m, m:-m] = full
    return big[:, lo[2] + m:lo[2] + m + n[2], lo[1] + m:lo[1] + m + n[1], lo[0] + m:lo[0] + m + n[0]]


def _upload_all(be, iv, boxes):
    for lvl in be.levels():
        be.mg.set_level(lvl, iv, boxes[lvl])


def _filled(be, iv, rng):
    """Random boxes on every level, a fill of every level, the download: the
    reference's mg%boxes(id)%cc after mg_fill_ghost_cells.  Then the random
    boxes go up again, so the ghosts on the device are stale.
    Returns ({lvl: uploaded}, {lvl: filled})."""
    tree = be.tree
    up = {lvl: _random_boxes(rng, len(tree.lvls[lvl].my_ids), tree.box_size_lvl[lvl]) for lvl in be.levels()}
    _upload_all(be, iv, up)
    omg.mg_fill_ghost_cells(be.mg, iv)
    filled = {lvl: be.mg.get_level(lvl, iv) for lvl in be.levels()}
    _upload_all(be, iv, up)
    return up, filled


# -- 1. bitwise against numpy, both kernels, every level ------------------------------
@pytest.mark.parametrize("name", sorted(TREES))
def test_every_level_bitwise_against_numpy(monkeypatch, name):
    be = _backend(TREES[name])
    mg, tree = be.mg, be.tree
    rng = np.random.default_rng(20261020)
    assert {tree.box_size_lvl[lvl] for lvl in be.levels()} == SIZES[name]
    if name == "refined":
        # (ref_bnds lists the coarse side: levels 2 and 3 have refinement-boundary ghosts)
        assert len(tree.lvls[1].ref_bnds) and len(tree.lvls[2].ref_bnds)
    tiled = sum(tree.box_size_lvl[lvl] in (16, 8) for lvl in be.levels())
    calls = 0
    for iv in (IPHI, IRHS):
        up, filled = _filled(be, iv, rng)
        for lvl in be.levels():   # (ascending: a refinement-boundary fill reads the level below)
            ids = tree.lvls[lvl].my_ids
            g = U.grid(tree, lvl)
            cells = len(ids) * tree.box_size_lvl[lvl] ** 3
            m = U.stored_mask(tree.box_size_lvl[lvl])
            assert not np.array_equal(up[lvl][:, m], filled[lvl][:, m])   # (the fill changed the ghosts)
            for scale in SCALES:
                want = numpy_grad(tree, lvl, ids, filled[lvl], scale)
                if scale < 0 and tree.box_size_lvl[lvl] >= 4:
                    assert (want == np.array([-0.0]).view(np.int64)[0]).any()   # (the sign of zero is compared)
                got = []
                for generic in (False, True):
                    _switch(monkeypatch, generic)
                    out = _sentinel((3, g[2], g[1], g[0]))
                    res, n = mg.get_dense_grad(lvl, iv, out=out, scale=scale)
                    calls += 1
                    assert res is out and n == cells == U.count_cells(tree, lvl, (0, 0, 0), g, ids)
                    got.append(_bits(out))
                    assert np.array_equal(got[-1], want), (name, iv, lvl, scale, generic)
                assert np.array_equal(got[0], got[1])
    assert _launches(be, "dense_grad") == calls
    # the tile kernel served the 16^3 and 8^3 levels, and nothing under the switch
    assert _launches(be, "dense_grad_row") == tiled * 2 * len(SCALES)


# -- 2. windows -------------------------------------------------------------------------
def _strided(n):
    """The three windows as views of a larger tensor: (big, view [3, nz, ny, nx])."""
    big = _sentinel((3, n[2], n[1] + 2, n[0] + 6))
    return big, big[:, :, 1:1 + n[1], 2:2 + n[0]]


def _off8(n):
    """Every component 8 B off a 16-B boundary: (flat, view)."""
    per = n[0] * n[1] * n[2]
    flat = _sentinel((3 * per + 1,))
    assert flat.data_ptr() % 16 == 0 and per % 2 == 0
    return flat, flat[1:].view(3, n[2], n[1], n[0])


@pytest.fixture(scope="module")
def win16():
    """One 32^3 periodic tree of 16^3 boxes with filled random phi and rhs
    (shared by the window tests, which only read it)."""
    be = _backend(WIN16)
    tree, ids = be.tree, be.tree.lvls[1].my_ids
    rng = np.random.default_rng(7)
    full = {}
    for iv in (IPHI, IRHS):
        boxes = _random_boxes(rng, len(ids), 16)
        be.mg.set_level(1, iv, boxes)
        omg.mg_fill_ghost_cells_lvl(be.mg, 1, iv)
        full[iv] = numpy_grad(tree, 1, ids, be.mg.get_level(1, iv), -1.0)
    return be, full


# (lo, n, layout, whether the tile kernel serves part of the window)
WINDOWS = {
    "whole": ((0, 0, 0), (32, 32, 32), None, True),
    "whole-boxes": ((16, 0, 16), (16, 32, 16), None, True),
    "cut-odd": ((3, 5, 7), (20, 9, 13), None, False),
    "outside": ((-4, 0, 28), (40, 8, 8), None, True),
    "strided": ((0, 0, 16), (32, 32, 16), _strided, True),
    "off8": ((0, 16, 0), (32, 16, 32), _off8, False),
    "both": ((8, 0, 0), (24, 32, 32), None, True),
}


@pytest.mark.parametrize("generic", [False, True], ids=["tile", "generic"])
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_windows(monkeypatch, win16, name, generic):
    _switch(monkeypatch, generic)
    be, full = win16
    lo, n, layout, tile = WINDOWS[name]
    be.mg.ctx.call("reset_stats")
    for iv in (IPHI, IRHS):
        want = _crop(full[iv], lo, n)
        big, out = (None, _sentinel((3, n[2], n[1], n[0]))) if layout is None else layout(n)
        _, cells = be.mg.get_dense_grad(1, iv, out=out, lo=lo, scale=-1.0)
        assert cells == U.count_cells(be.tree, 1, lo, n) == int((want[0] != U.SENTINEL).sum())
        assert 0 < cells <= 32 ** 3
        assert np.array_equal(_bits(out), want), (name, iv)
        if big is not None:   # (the larger tensor around the views: only the views were written)
            outside = torch.ones_like(big, dtype=torch.bool)
            if layout is _strided:
                outside[:, :, 1:1 + n[1], 2:2 + n[0]] = False
                assert bool((big.view(torch.int64)[outside] == int(U.SENTINEL)).all())
            else:
                assert int((big.view(torch.int64) == int(U.SENTINEL)).sum()) == big.numel() - 3 * n[0] * n[1] * n[2]
    # a base misaligned by one double (and every odd window) never reaches the tile kernel
    assert (_launches(be, "dense_grad_row") > 0) == (tile and not generic)
    assert _launches(be, "dense_grad") == 2


def test_cut_windows_of_every_tree_level(monkeypatch):
    """denseutil.cut_windows on the refined tree's levels, both kernels."""
    be = _backend(U.REFINED)
    tree = be.tree
    _, filled = _filled(be, IPHI, np.random.default_rng(5))
    for lvl in be.levels():
        ids = tree.lvls[lvl].my_ids
        full = numpy_grad(tree, lvl, ids, filled[lvl], 0.37)
        for lo, n in U.cut_windows(tree, lvl):
            want = _crop(full, lo, n)
            for generic in (False, True):
                _switch(monkeypatch, generic)
                out = _sentinel((3, n[2], n[1], n[0]))
                _, cells = be.mg.get_dense_grad(lvl, IPHI, out=out, lo=lo, scale=0.37)
                assert cells == U.count_cells(tree, lvl, lo, n, ids), (lvl, lo, n)
                assert np.array_equal(_bits(out), want), (lvl, lo, n, generic)


def test_a_fifth_window_replaces_the_oldest(monkeypatch):
    """The gradient shares omg_get_dense's four cached windows of a level: more
    of them still give the right values, and only a call that replaces a
    window whose records are on the device waits on the host."""
    _switch(monkeypatch, False)
    be = _backend(WIN16, profile=False)
    mg, ctx, tree = be.mg, be.mg.ctx, be.tree
    ids = tree.lvls[1].my_ids
    mg.set_level(1, IPHI, _random_boxes(np.random.default_rng(43), len(ids), 16))
    omg.mg_fill_ghost_cells_lvl(mg, 1, IPHI)
    want = numpy_grad(tree, 1, ids, mg.get_level(1, IPHI), -1.0)
    ctx.call("synchronize")
    waits = []
    for z in (0, 2, 4, 6, 8, 0):   # (five distinct windows; the first was replaced by then)
        before = ctx.host_sync_count()
        out, cells = mg.get_dense_grad(1, IPHI, lo=(0, 0, z), shape=(16, 32, 32), scale=-1.0)
        waits.append(ctx.host_sync_count() - before)
        assert cells == 16 * 32 * 32
        assert np.array_equal(_bits(out), _crop(want, (0, 0, z), (32, 32, 16))), z
    assert waits == [0, 0, 0, 0, 1, 1]


MASKS = [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True),
         (False, True, True)]


@pytest.mark.parametrize("generic", [False, True], ids=["tile", "generic"])
def test_component_masks_leave_skipped_tensors_alone(monkeypatch, win16, generic):
    _switch(monkeypatch, generic)
    be, full = win16
    for mask in MASKS:
        # through `components` on one tensor, and through a sequence with Nones
        out = _sentinel((3, 32, 32, 32))
        res, cells = be.mg.get_dense_grad(1, IPHI, out=out, scale=-1.0, components=mask)
        parts = [(_sentinel((32, 32, 32)) if m else None) for m in mask]
        res2, cells2 = be.mg.get_dense_grad(1, IPHI, out=parts, scale=-1.0)
        assert res is out and res2 is parts and cells == cells2 == 32 ** 3
        got = _bits(out)
        for d in range(3):
            if mask[d]:
                assert np.array_equal(got[d], full[IPHI][d]), (mask, d)
                assert np.array_equal(_bits(parts[d]), full[IPHI][d]), (mask, d)
            else:
                assert (got[d] == U.SENTINEL).all(), (mask, d)


# -- 3. fill ----------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["tile", "generic"])
@pytest.mark.parametrize("args", [WIN16, DIR16], ids=["periodic", "dirichlet"])
def test_fill_false_uses_the_ghosts_as_they_stand(monkeypatch, args, generic):
    _switch(monkeypatch, generic)
    be = _backend(args)
    mg, tree = be.mg, be.tree
    ids = tree.lvls[1].my_ids
    rng = np.random.default_rng(31)
    mg.set_level(1, IPHI, _random_boxes(rng, len(ids), 16))
    omg.mg_fill_ghost_cells_lvl(mg, 1, IPHI)
    mg.set_dense(1, IPHI, torch.from_numpy(rng.standard_normal((32, 32, 32))).cuda())   # (the ghosts are stale now)
    stale = mg.get_level(1, IPHI)          # the new interior, the old phi's ghosts: no fill ran
    want_stale = numpy_grad(tree, 1, ids, stale, 1.0)
    out, _ = mg.get_dense_grad(1, IPHI, fill=False)
    assert np.array_equal(_bits(out), want_stale)
    assert np.array_equal(mg.get_level(1, IPHI).view(np.int64), stale.view(np.int64))   # (it filled nothing)
    out, _ = mg.get_dense_grad(1, IPHI, fill=True)
    got = _bits(out)
    omg.mg_fill_ghost_cells_lvl(mg, 1, IPHI)
    fresh = mg.get_level(1, IPHI)
    assert not np.array_equal(fresh.view(np.int64), stale.view(np.int64))
    want = numpy_grad(tree, 1, ids, fresh, 1.0)
    assert not np.array_equal(want, want_stale)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("generic", [False, True], ids=["tile", "generic"])
def test_rhs_after_phi_bc_store_differences_the_stored_boundary_values(monkeypatch, generic):
    _switch(monkeypatch, generic)
    be = _backend(DIR16)
    mg, tree = be.mg, be.tree
    ids = tree.lvls[1].my_ids
    mg.set_level(1, IRHS, _random_boxes(np.random.default_rng(37), len(ids), 16))
    omg.mg_fill_ghost_cells_lvl(mg, 1, IRHS)
    omg.mg_phi_bc_store(mg)
    rhs = mg.get_level(1, IRHS)
    ghosts = rhs[:, U.stored_mask(16) & ~np.pad(np.ones((16,) * 3, bool), 1)]
    assert np.isin(ghosts, [0.25 * nb - 0.6 for nb in range(1, 7)]).any()   # (the stored boundary values are there)
    out, cells = mg.get_dense_grad(1, IRHS, fill=False, scale=-1.0)
    assert cells == 32 ** 3
    assert np.array_equal(_bits(out), numpy_grad(tree, 1, ids, rhs, -1.0))
    assert np.array_equal(mg.get_level(1, IRHS).view(np.int64), rhs.view(np.int64))


# -- 4. the lazy state two stand-alone cycles leave ------------------------------------------
def test_pending_shift_and_deferred_ghosts_are_resolved_and_the_next_cycle_is_unchanged(monkeypatch):
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", "64")
    monkeypatch.delenv("OMG_BLOCK3_COLUMN", raising=False)
    _switch(monkeypatch, False)
    trio = []
    for _ in range(3):
        be = DeviceBackend(parse(PER128))
        setup_problem(be)
        be.mg.ctx.call("set_profiling", 1)
        be.vcycle(False)
        be.vcycle(False)
        trio.append(be)
    a, b, c = trio   # a: the gradient call; b: the reference download; c: cycles alone
    tree, top = a.tree, a.tree.highest_lvl
    ids = tree.lvls[top].my_ids
    # (the cycles ended in k_gsrb4's correction form, the one that defers the ghosts)
    assert _launches(a, f"smoother_gsrb4p@{top}") >= 2
    out, cells = a.mg.get_dense_grad(top, scale=-1.0)
    assert cells == 128 ** 3 and _launches(a, f"dense_grad_row@{top}") == 1
    omg.mg_fill_ghost_cells_lvl(b.mg, top, IPHI)
    want = numpy_grad(tree, top, ids, b.mg.get_level(top, IPHI), -1.0)
    assert np.array_equal(_bits(out), want)
    ha, hc = a.vcycle(True), c.vcycle(True)
    assert float(ha).hex() == float(hc).hex()
    assert phi_digest(a) == phi_digest(c)


# -- 5. stream ordering, no host wait ---------------------------------------------------------
def test_calls_are_ordered_on_the_callers_stream_without_a_host_wait(monkeypatch):
    _switch(monkeypatch, False)
    be = _backend(STREAM64, profile=False)
    mg, ctx, tree = be.mg, be.mg.ctx, be.tree
    ids = tree.lvls[1].my_ids
    mg.set_level(1, IPHI, _random_boxes(np.random.default_rng(9), len(ids), 16))
    omg.mg_fill_ghost_cells_lvl(mg, 1, IPHI)
    want = numpy_grad(tree, 1, ids, mg.get_level(1, IPHI), 1.0)
    scratch = torch.zeros(32 * 1024 * 1024, dtype=torch.float64, device="cuda")   # 256 MB
    out = _sentinel((3, 64, 64, 64))
    mg.get_dense_grad(1, out=out)   # (the window's records go up here)
    side = torch.cuda.Stream()
    ctx.call("synchronize")
    torch.cuda.synchronize()
    out.copy_(_sentinel((3, 64, 64, 64)))
    torch.cuda.synchronize()
    syncs = ctx.host_sync_count()
    with torch.cuda.stream(side):
        for _ in range(200):   # (tens of milliseconds of queued passes)
            scratch.add_(1.0)
        kept = []
        for _ in range(3):
            _, n = mg.get_dense_grad(1, out=out)
            assert n == 64 ** 3
            kept.append(out.clone())          # the consumer queued behind the call
            out.fill_(0.0)                    # and a writer behind the consumer
        still_running = not side.query()
    assert ctx.host_sync_count() == syncs
    assert still_running, "the queued passes had finished: the calls were not made under load"
    torch.cuda.synchronize()
    for k in kept:
        assert np.array_equal(_bits(k), want)
    assert float(scratch[0]) == 200.0


# -- 6. ranks ------------------------------------------------------------------------------------
def test_two_ranks_hold_their_own_boxes_and_fill_remote_faces(monkeypatch):
    _switch(monkeypatch, False)

    def body(be, rank, reduce):
        tree, ids = be.tree, be.my_ids(1)
        boxes = _random_boxes(np.random.default_rng(41 + rank), len(ids), 16)
        be.set_level(1, IPHI, boxes)
        omg.mg_fill_ghost_cells_lvl(be.mg, 1, IPHI)
        filled = be.mg.get_level(1, IPHI)
        be.set_level(1, IPHI, boxes)          # (the ghosts, remote faces included, are stale again)
        assert not np.array_equal(filled[:, U.stored_mask(16)], boxes[:, U.stored_mask(16)])
        out = _sentinel((3, 64, 64, 64))
        _, cells = be.mg.get_dense_grad(1, out=out, scale=-1.0)
        assert cells == len(ids) * 16 ** 3
        got = _bits(out)
        assert np.array_equal(got, numpy_grad(tree, 1, ids, filled, -1.0))
        remote = int(sum(tree.rank[tree.neighbors[i, nb]] != rank for i in ids for nb in range(6)
                         if tree.neighbors[i, nb] > 0))
        return cells, got[0] != U.SENTINEL, remote

    res = run_loopback(STREAM64, 2, body, timeout=120)
    assert res[0][0] + res[1][0] == 64 ** 3 and res[0][0] > 0 and res[1][0] > 0
    assert not (res[0][1] & res[1][1]).any() and (res[0][1] | res[1][1]).all()
    assert res[0][2] > 0 and res[1][2] > 0   # (both ranks have faces whose neighbour is remote)


def test_replicated_level_reads_the_hosts_own_boxes(monkeypatch):
    _switch(monkeypatch, False)

    def body(be, rank, reduce):
        lvl = 0
        assert be.rep_lvl >= lvl
        tree, ids = be.tree, be.my_ids(lvl)
        nc = tree.box_size_lvl[lvl]
        assert 0 < len(ids) < len(tree.lvls[lvl].ids)
        be.set_level(lvl, IPHI, _random_boxes(np.random.default_rng(17 + rank), len(ids), nc))   # (collective)
        omg.mg_fill_ghost_cells_lvl(be.mg, lvl, IPHI)
        filled = be.mg.get_level(lvl, IPHI)
        g = U.grid(tree, lvl)
        out = _sentinel((3, g[2], g[1], g[0]))
        _, cells = be.mg.get_dense_grad(lvl, out=out)
        assert cells == len(ids) * nc ** 3
        assert np.array_equal(_bits(out), numpy_grad(tree, lvl, ids, filled, 1.0))
        return cells

    res = run_loopback(STREAM64, 2, body, timeout=120, rep_cells=8 * 16 ** 3)
    assert sum(res) == 8 * 16 ** 3


# -- 7. errors before any launch -------------------------------------------------------------
def test_bad_pointers_are_errors_before_any_launch_and_the_context_stays_usable(win16):
    be, full = win16
    ctx = be.mg.ctx
    ctx.call("reset_stats")
    n, stride = (32, 32, 32), (1, 32, 1024)
    good = _sentinel((3, 32, 32, 32))
    host = np.zeros(32 ** 3)
    small = _sentinel((32 ** 3,))
    far = (1, 32, 1 << 34)   # planes 128 GiB apart: past the end of any allocation
    p = good.data_ptr()
    for what, ptrs, st in (("the pointer is not device memory", (host.ctypes.data, 0, 0), stride),
                           ("the pointer is not device memory", (p, 0, host.ctypes.data), stride),
                           ("the window reaches past the end of the pointer's allocation",
                            (0, small.data_ptr(), 0), far),
                           ("the windows of components 0 and 1 overlap", (p, p + 8 * (32 ** 3 - 1), 0), stride),
                           ("the windows of components 1 and 2 overlap", (0, p + 8, p), stride)):
        with pytest.raises(omg.device.OmgError) as ex:
            ctx.get_dense_grad(1, IPHI, ptrs, (0, 0, 0), n, st, -1.0)
        assert str(ex.value) == "omg_get_dense_grad: " + what
        assert _launches(be, "dense_grad") == 0
        assert (_bits(good) == U.SENTINEL).all() and (_bits(small) == U.SENTINEL).all()
        # the context stays usable
        ok = _sentinel((3, 32, 32, 32))
        assert ctx.get_dense_grad(1, IPHI, [ok[d].data_ptr() for d in range(3)], (0, 0, 0), n, stride, -1.0) == 32 ** 3
        assert np.array_equal(_bits(ok), full[IPHI])
        ctx.call("reset_stats")
