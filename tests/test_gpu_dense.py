"""omg_put_dense / omg_get_dense on the GPU: dense device tensors <-> the boxes,
against the host path (omg_upload_level / omg_download_level) and numpy.

1. round trips on every level of four trees (boxes of 16, 8, 5 and 6 cells),
   row kernel and per-cell kernel;
2. windows that are whole boxes, cut boxes, reach outside, are strided views
   or start 8 B off a 16-B boundary;
3. the refined levels of a three-level tree (part of the grid has no box);
4. the state a cycle leaves (pending phi shift, deferred ghosts, stored
   boundary data in the rhs ghosts, the ring-order copy of rhs);
5. stream ordering without a host synchronise;
6. two ranks on the loopback transport, and a replicated coarse level.

Every comparison is on bits: a copy has no tolerance."""
import numpy as np
import pytest
import torch

from tests import denseutil as U
from tests.apiwalk import PER128, RING, TREES
from tests.mgdriver import DeviceBackend, omg, parse, phi_digest, run_loopback, setup_problem

pytestmark = pytest.mark.gpu

IPHI, IRHS = 1, 2
BOX16 = "16 32 16 48 1 v gsrb lpl 0 d0 sol 1 lb 0"   # 2 x 1 x 3 boxes: a swap of axes shows
BOX5 = "5 10 10 10 1 v gsrb lpl 0 d0 sol 1 lb 0"      # odd box size (denseutil.odd_box_tree)
BOX6 = "6 12 12 12 1 v gs lpl 0 d0 sol 1 lb 0"        # its coarsest level has one 3^3 box
WIN16 = "16 32 32 32 1 v gsrb lpl 0 per sol 1 lb 0"
STREAM64 = "16 64 64 64 1 v gsrb lpl 0 per sol 1 lb 0"


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(a, b, msg=None):
    assert np.array_equal(_bits(a), _bits(b)), msg


def _switch(monkeypatch, generic):
    if generic:
        monkeypatch.setenv("OMG_DENSE_GENERIC", "1")
    else:
        monkeypatch.delenv("OMG_DENSE_GENERIC", raising=False)


def _backend(args, profile=True):
    cfg = parse(args)
    be = U.OddBoxBackend(cfg) if cfg["box"] % 2 else DeviceBackend(cfg)
    if profile:
        be.mg.ctx.call("set_profiling", 1)
    return be


def _random_boxes(rng, n, nc):
    return rng.standard_normal((n, nc + 2, nc + 2, nc + 2))


def _downloaded(boxes, nc):
    """What a download of uploaded `boxes` gives: edges and corners read 0."""
    out = boxes.copy()
    out[:, ~U.stored_mask(nc)] = 0.0
    return out


def _sentinel(shape):
    return torch.full(tuple(shape), int(U.SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)


def _launches(be, name):
    be.mg.ctx.call("synchronize")
    return be.mg.ctx.kernel_stats(name)[0]


def _put_and_check(be, lvl, iv, rng, lo=None, n=None, window=None):
    """Upload a pattern with non-zero ghosts, put a random window, download:
    the interior inside the window is the window's, everything else the
    pattern's.  window(host array) -> the device tensor to pass."""
    mg, tree = be.mg, be.tree
    ids, nc = tree.lvls[lvl].my_ids, tree.box_size_lvl[lvl]
    g = U.grid(tree, lvl)
    lo = (0, 0, 0) if lo is None else lo
    n = g if n is None else n
    pat = _random_boxes(rng, len(ids), nc)
    mg.set_level(lvl, iv, pat)
    dense = rng.standard_normal((n[2], n[1], n[0]))
    t = torch.from_numpy(dense).cuda() if window is None else window(dense)
    cells = mg.set_dense(lvl, iv, t, lo)
    assert cells == U.count_cells(tree, lvl, lo, n, ids), (lvl, lo, n)
    _same(mg.get_level(lvl, iv), _downloaded(U.scatter(tree, lvl, ids, pat, dense, lo), nc), ("put", lvl, lo, n))
    _same(t.cpu().numpy(), dense, "put changed its source")
    return cells


def _get_and_check(be, lvl, iv, rng, lo=None, n=None, window=None):
    """Upload random boxes, get a window pre-filled with a sentinel: covered
    elements are the boxes' cells, the others still the sentinel."""
    mg, tree = be.mg, be.tree
    ids, nc = tree.lvls[lvl].my_ids, tree.box_size_lvl[lvl]
    g = U.grid(tree, lvl)
    lo = (0, 0, 0) if lo is None else lo
    n = g if n is None else n
    boxes = _random_boxes(rng, len(ids), nc)
    mg.set_level(lvl, iv, boxes)
    # the level's grid with a margin, so that a window may reach outside
    m = 8
    full = np.full((g[2] + 2 * m, g[1] + 2 * m, g[0] + 2 * m), U.SENTINEL, dtype=np.int64)
    full[m:-m, m:-m, m:-m] = U.assemble(tree, lvl, ids, boxes, U.SENTINEL)
    want = full[lo[2] + m:lo[2] + m + n[2], lo[1] + m:lo[1] + m + n[1], lo[0] + m:lo[0] + m + n[0]]
    assert want.shape == (n[2], n[1], n[0])
    out = _sentinel((n[2], n[1], n[0])) if window is None else window(None)
    got, cells = mg.get_dense(lvl, iv, out=out, lo=lo)
    assert got is out
    assert cells == U.count_cells(tree, lvl, lo, n, ids) == int((want != U.SENTINEL).sum()), (lvl, lo, n)
    _same(out.cpu().numpy(), want, ("get", lvl, lo, n))
    return cells


# -- 1. round trips against the host path --------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["row", "generic"])
@pytest.mark.parametrize("args", [BOX16, U.NONCUBE, BOX5, BOX6], ids=["box16", "box8", "box5", "box6"])
def test_round_trip_on_every_level(monkeypatch, args, generic):
    _switch(monkeypatch, generic)
    be = _backend(args)
    rng = np.random.default_rng(20261020)
    sizes = set()
    for lvl in be.levels():
        sizes.add(be.tree.box_size_lvl[lvl])
        _put_and_check(be, lvl, IRHS, rng)
        _get_and_check(be, lvl, IPHI, rng)
    assert sizes == {BOX16: {16, 8, 4, 2}, U.NONCUBE: {8, 4, 2}, BOX5: {5}, BOX6: {6, 3}}[args]
    n_lvls = len(be.levels())
    assert _launches(be, "dense_put") == n_lvls and _launches(be, "dense_get") == n_lvls
    # the row kernel served the 16^3 and 8^3 levels, and nothing under the switch
    rows = 0 if generic else sum(be.tree.box_size_lvl[lvl] in (16, 8) for lvl in be.levels())
    assert _launches(be, "dense_put_row") == rows and _launches(be, "dense_get_row") == rows
    top = be.tree.highest_lvl
    assert _launches(be, f"dense_put_row@{top}") == (0 if generic or be.tree.box_size not in (16, 8) else 1)


# -- 2. windows -------------------------------------------------------------------
def _strided(n):
    """The window as a view of a larger tensor: (big, view)."""
    big = _sentinel((n[2], n[1] + 2, n[0] + 6))
    return big, big[:, 1:1 + n[1], 2:2 + n[0]]


def _off8(n):
    """The window 8 B off a 16-B boundary: (flat, view)."""
    flat = _sentinel((n[0] * n[1] * n[2] + 1,))
    assert flat.data_ptr() % 16 == 0
    return flat, flat[1:].view(n[2], n[1], n[0])


# (lo, n, layout, whether the row kernel serves the window)
WINDOWS = {
    "whole-boxes": ((16, 0, 16), (16, 32, 16), None, True),
    "cut-odd": ((3, 5, 7), (20, 9, 13), None, False),
    "outside": ((-4, 0, 28), (40, 8, 8), None, True),    # (even offsets, whole rows: part of the planes)
    "strided": ((0, 0, 16), (32, 32, 16), _strided, True),
    "off8": ((0, 16, 0), (32, 16, 32), _off8, False),
    "both": ((8, 0, 0), (24, 32, 32), None, True),       # the boxes at x = 0 cut in x, the others whole
}


@pytest.mark.parametrize("generic", [False, True], ids=["row", "generic"])
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_windows(monkeypatch, name, generic):
    _switch(monkeypatch, generic)
    lo, n, layout, row = WINDOWS[name]
    be = _backend(WIN16)
    rng = np.random.default_rng(7)
    held = []

    def put_window(dense):
        if layout is None:
            return torch.from_numpy(dense).cuda()
        big, view = layout(n)
        view.copy_(torch.from_numpy(dense))
        held.append((big, big.clone()))
        return view

    def get_window(_):
        if layout is None:
            return _sentinel((n[2], n[1], n[0]))
        big, view = layout(n)
        held.append((big, view))
        return view

    cells = _put_and_check(be, 1, IRHS, rng, lo, n, put_window)
    assert 0 < cells < 32 ** 3
    if held:   # (the larger tensor around the view: a put writes nothing of it)
        _same(held[0][0].cpu().numpy(), held[0][1].cpu().numpy())
    held.clear()
    assert _get_and_check(be, 1, IPHI, rng, lo, n, get_window) == cells
    if held:   # (a get writes the view alone)
        big, view = held[0]
        outside = torch.ones_like(big, dtype=torch.bool)
        if layout is _strided:
            outside[:, 1:1 + n[1], 2:2 + n[0]] = False
        else:
            outside[1:] = False
        assert bool((big.view(torch.int64)[outside] == int(U.SENTINEL)).all())
    used = row and not generic
    assert (_launches(be, "dense_put_row") > 0) == used and (_launches(be, "dense_get_row") > 0) == used
    if name == "both" and not generic:   # (one call, both kernels: four boxes each)
        assert be.mg.ctx.kernel_stats("dense_put_row")[2] == 4 * 16 ** 3


def test_a_fifth_window_replaces_the_oldest(monkeypatch):
    """The level keeps the clipping of four windows; more of them still copy
    the right cells, and only the call that replaces one waits on the host."""
    _switch(monkeypatch, False)
    be = _backend(WIN16, profile=False)
    mg, ctx, tree = be.mg, be.mg.ctx, be.tree
    ids = tree.lvls[1].my_ids
    boxes = _random_boxes(np.random.default_rng(23), len(ids), 16)
    mg.set_level(1, IRHS, boxes)
    want = U.assemble(tree, 1, ids, boxes, U.SENTINEL)
    ctx.call("synchronize")
    waits = []
    for z in (0, 2, 4, 6, 8, 10, 0, 2):   # (the last two were replaced by then)
        before = ctx.host_sync_count()
        out, cells = mg.get_dense(1, IRHS, lo=(0, 0, z), shape=(16, 32, 32))
        waits.append(ctx.host_sync_count() - before)
        assert cells == 16 * 32 * 32
        _same(out.cpu().numpy(), want[z:z + 16])
    assert waits == [0, 0, 0, 0, 1, 1, 1, 1]


# -- 3. refined levels --------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["row", "generic"])
def test_refined_levels_leave_the_uncovered_grid_alone(monkeypatch, generic):
    _switch(monkeypatch, generic)
    be = _backend(U.REFINED)
    rng = np.random.default_rng(11)
    for lvl in (2, 3):
        n_boxes = len(be.tree.lvls[lvl].ids)
        g = U.grid(be.tree, lvl)
        assert n_boxes * 512 < g[0] * g[1] * g[2]   # (part of the grid has no box)
        assert _put_and_check(be, lvl, IRHS, rng) == n_boxes * 512
        assert _get_and_check(be, lvl, IPHI, rng) == n_boxes * 512


# -- 4. the state a cycle leaves ---------------------------------------------------
def _twin(args, store_bc=False):
    pair = []
    for _ in range(2):
        be = DeviceBackend(parse(args))
        setup_problem(be)
        if store_bc:
            omg.mg_phi_bc_store(be.mg)
        be.mg.ctx.call("set_profiling", 1)
        pair.append(be)
    return pair


def _replace_interior(be, lvl, iv, dense):
    """The host path's equivalent of set_dense: download, new interior, upload
    (the ghosts go back as they came)."""
    ids = be.tree.lvls[lvl].my_ids
    be.mg.set_level(lvl, iv, U.scatter(be.tree, lvl, ids, be.mg.get_level(lvl, iv), dense))


def _state_twin(args, store_bc=False):
    a, b = _twin(args, store_bc)
    tree, top = a.tree, a.tree.highest_lvl
    ids, nc = tree.lvls[top].my_ids, tree.box_size_lvl[top]
    for be in (a, b):
        be.vcycle(False)
        be.vcycle(False)
    phi_a, cells = a.mg.get_dense(top, IPHI)
    assert cells == len(ids) * nc ** 3
    phi_b = b.mg.get_level(top, IPHI)
    _same(phi_a.cpu().numpy().view(np.int64), U.assemble(tree, top, ids, phi_b, U.SENTINEL), "phi after two cycles")
    rng = np.random.default_rng(3)
    g = U.grid(tree, top)
    new_phi = 0.5 * phi_a.cpu().numpy() + 1e-3 * rng.standard_normal((g[2], g[1], g[0]))
    new_rhs = rng.standard_normal((g[2], g[1], g[0]))
    a.mg.set_dense(top, IPHI, torch.from_numpy(new_phi).cuda())
    a.mg.set_dense(top, IRHS, torch.from_numpy(new_rhs).cuda())
    _replace_interior(b, top, IPHI, new_phi)
    _replace_interior(b, top, IRHS, new_rhs)
    hist_a = [a.vcycle(True), a.vcycle(True)]
    hist_b = [b.vcycle(True), b.vcycle(True)]
    assert [float(x).hex() for x in hist_a] == [float(x).hex() for x in hist_b]
    assert phi_digest(a) == phi_digest(b)
    assert phi_digest(a, IRHS) == phi_digest(b, IRHS)
    return a, b


def test_put_and_get_meet_a_pending_shift_and_deferred_ghosts(monkeypatch):
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", "64")
    monkeypatch.delenv("OMG_BLOCK3_COLUMN", raising=False)
    _switch(monkeypatch, False)
    a, _ = _state_twin(PER128)
    # (the cycles ended in k_gsrb4's correction form, the one that defers the ghosts)
    assert _launches(a, "smoother_gsrb4p@1") >= 2
    assert _launches(a, "dense_put_row@1") == 2 and _launches(a, "dense_get_row@1") == 1


def test_put_leaves_the_stored_boundary_data_alone(monkeypatch):
    """Physical faces with mg_phi_bc_store: the boundary values live in the rhs
    ghosts.  The uploading twin sends back the ghosts it downloaded; the same
    history shows that set_dense left them as they were."""
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", "64")
    monkeypatch.delenv("OMG_BLOCK3_COLUMN", raising=False)
    _switch(monkeypatch, False)
    a, b = _state_twin(TREES["mx2_helm64_box16"], store_bc=True)
    top = a.tree.highest_lvl
    rhs = a.mg.get_level(top, IRHS)
    _same(rhs, b.mg.get_level(top, IRHS))
    nc = a.tree.box_size_lvl[top]
    ghosts = rhs[:, U.stored_mask(nc) & ~np.pad(np.ones((nc,) * 3, bool), 1)]
    assert np.count_nonzero(ghosts)   # (the stored boundary values are there)


def test_put_of_rhs_drops_the_ring_order_copy(monkeypatch):
    monkeypatch.delenv("OMG_BLOCK3_MIN_BOXES", raising=False)
    _switch(monkeypatch, False)
    a, b = _twin(RING)
    top = a.tree.highest_lvl
    g = U.grid(a.tree, top)
    new_rhs = np.random.default_rng(5).standard_normal((g[2], g[1], g[0]))
    a.vcycle(False)
    b.vcycle(False)
    before = _launches(a, f"rhs_lex@{top}")
    assert before >= 1   # (the register ring served the level)
    a.mg.set_dense(top, IRHS, torch.from_numpy(new_rhs).cuda())
    _replace_interior(b, top, IRHS, new_rhs)
    assert float(a.vcycle(True)).hex() == float(b.vcycle(True)).hex()
    assert _launches(a, f"rhs_lex@{top}") > before
    assert phi_digest(a) == phi_digest(b)


# -- 5. stream ordering, no host synchronise -------------------------------------------
def test_calls_are_ordered_on_the_callers_stream_without_a_host_wait(monkeypatch):
    _switch(monkeypatch, False)
    be = _backend(STREAM64, profile=False)
    mg, ctx = be.mg, be.mg.ctx
    first = torch.from_numpy(np.random.default_rng(9).standard_normal((64, 64, 64))).cuda()
    scratch = torch.zeros(32 * 1024 * 1024, dtype=torch.float64, device="cuda")   # 256 MB
    side = torch.cuda.Stream()
    ctx.call("synchronize")
    torch.cuda.synchronize()
    syncs = ctx.host_sync_count()
    with torch.cuda.stream(side):
        for _ in range(200):   # (tens of milliseconds of queued passes)
            scratch.add_(1.0)
        src = torch.empty_like(first)
        src.copy_(first)
        n_put = mg.set_dense(1, IRHS, src)
        src.fill_(-1.0)
        out = _sentinel((64, 64, 64))
        _, n_get = mg.get_dense(1, IRHS, out=out)
        kept = out.clone()
        still_running = not side.query()
    assert ctx.host_sync_count() == syncs
    assert still_running, "the queued passes had finished: the calls were not made under load"
    assert n_put == n_get == 64 ** 3
    torch.cuda.synchronize()
    _same(kept.cpu().numpy(), first.cpu().numpy())
    assert float(scratch[0]) == 200.0


# -- 6. two ranks ------------------------------------------------------------------------
def test_two_ranks_cover_disjoint_parts(monkeypatch):
    _switch(monkeypatch, False)
    dense = np.random.default_rng(13).standard_normal((64, 64, 64))

    def body(be, rank, reduce):
        t = torch.from_numpy(dense).cuda()
        n_put = be.mg.set_dense(1, IRHS, t)
        out = _sentinel((64, 64, 64))
        _, n_get = be.mg.get_dense(1, IRHS, out=out)
        assert n_put == n_get == len(be.my_ids(1)) * 16 ** 3
        return n_put, out.cpu().numpy().view(np.int64)

    res = run_loopback(STREAM64, 2, body, timeout=120)
    assert res[0][0] + res[1][0] == 64 ** 3 and res[0][0] > 0 and res[1][0] > 0
    cov = [r[1] != U.SENTINEL for r in res]
    assert not (cov[0] & cov[1]).any() and (cov[0] | cov[1]).all()
    _same(np.where(cov[0], res[0][1], res[1][1]), dense)


def test_replicated_level_get_own_boxes_put_refused(monkeypatch):
    _switch(monkeypatch, False)

    def body(be, rank, reduce):
        lvl = 0
        assert be.rep_lvl >= lvl
        tree, ids = be.tree, be.my_ids(lvl)
        nc = tree.box_size_lvl[lvl]
        assert 0 < len(ids) < len(tree.lvls[lvl].ids)
        boxes = np.random.default_rng(17 + rank).standard_normal((len(ids), nc + 2, nc + 2, nc + 2))
        be.set_level(lvl, IRHS, boxes)   # (collective on a replicated level)
        g = U.grid(tree, lvl)
        out = _sentinel((g[2], g[1], g[0]))
        _, cells = be.mg.get_dense(lvl, IRHS, out=out)
        assert cells == len(ids) * nc ** 3
        _same(out.cpu().numpy().view(np.int64), U.assemble(tree, lvl, ids, boxes, U.SENTINEL))
        with pytest.raises(omg.device.OmgError, match="omg_upload_level"):
            be.mg.set_dense(lvl, IRHS, out)
        return cells

    res = run_loopback(STREAM64, 2, body, timeout=120, rep_cells=8 * 16 ** 3)
    assert sum(res) == 8 * 16 ** 3
