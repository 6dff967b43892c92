"""omg_get_boxes_grad on the GPU: the gradient of a variable over a list of
boxes, cell- or face-centred, as blocks of up to three component pools.

The expected values never come from the code under test: they are numpy's
(a - b) * f on the (nc+2)^3 boxes that get_level returns after the ghost fill
(block_grad below), f = (0.5 * scale) / dr at the cells and scale / dr at the
faces.  Every comparison is on int64 bit views, the sign of zero included:
one subtraction and one multiplication have no tolerance.  Every pool starts
as denseutil.SENTINEL, and every element outside the defined values, edges
and corners included, must still hold it.

1. every level of six trees (boxes of 16, 8, 6, 5, 4, 3 and 2 cells; physical,
   periodic and refinement-boundary faces), phi and rhs, three scales, both
   centrings, the tile kernel and the per-cell kernel;
2. block geometry: ghost widths 0..3, a base 8 B off a 16-B boundary, an odd
   row stride, a pool slice, permuted and partial lists, component masks,
   three separate pools against one tensor;
3. the leaves of a three-level tree in one call, against numpy differences of
   get_blocks(ghosts=True, fill=True);
4. the lazy state two stand-alone cycles leave;
5. the record cache and its host waits, launches per level;
6. stream ordering without a host wait;
7. two loopback ranks, and a replicated coarse level;
8. errors on a real context before any launch."""
import numpy as np
import pytest
import torch

from tests import denseutil as U
from tests.mgdriver import DeviceBackend, omg, parse, phi_digest, run_loopback, setup_problem

pytestmark = pytest.mark.gpu

IPHI, IRHS, IRES = 1, 2, 4
BOX16 = "16 32 32 32 1 v gsrb lpl 0 d0 sol 1 lb 0"     # levels of 16, 8, 4, 2
BOX5 = "5 10 10 10 1 v gsrb lpl 0 d0 sol 1 lb 0"       # odd box size (denseutil.odd_box_tree)
BOX6 = "6 12 12 12 1 v gs lpl 0 d0 sol 1 lb 0"         # its coarsest level has one 3^3 box
STREAM64 = "16 64 64 64 1 v gsrb lpl 0 per sol 1 lb 0"
REFINED_RB = "8 32 32 32 1 v gsrb lpl 0 sol sol 3 lb 0"
TREES = {"box16": BOX16, "noncube": U.NONCUBE, "refined": U.REFINED, "refined-gsrb": REFINED_RB, "box5": BOX5,
         "box6": BOX6}
SIZES = {"box16": {16, 8, 4, 2}, "noncube": {8, 4, 2}, "refined": {8, 4, 2}, "refined-gsrb": {8, 4, 2},
         "box5": {5}, "box6": {6, 3}}
SCALES = (1.0, -1.0, 0.37)
CENTRINGS = ("cell", "face")
SENT = int(U.SENTINEL)
NEG_ZERO = np.array([-0.0]).view(np.int64)[0]


def _switch(monkeypatch, variant):
    """variant: None the library's routing (short lists: the per-cell kernel),
    "tile" the tile kernel wherever it can serve, "generic" the per-cell kernel."""
    for k in ("OMG_BOXES_GENERIC", "OMG_BOXES_TILE"):
        monkeypatch.delenv(k, raising=False)
    if variant == "generic":
        monkeypatch.setenv("OMG_BOXES_GENERIC", "1")
    elif variant == "tile":
        monkeypatch.setenv("OMG_BOXES_TILE", "1")


def _backend(args, profile=True):
    cfg = parse(args)
    be = U.OddBoxBackend(cfg) if cfg["box"] % 2 else DeviceBackend(cfg)
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
    return torch.full(tuple(shape), SENT, dtype=torch.int64, device="cuda").view(torch.float64)


def _launches(be, name):
    be.mg.ctx.call("synchronize")
    return be.mg.ctx.kernel_stats(name)[0]


def _ids(be, lvl):
    return [int(i) for i in be.tree.lvls[lvl].my_ids]


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.int64)


def block_grad(boxes, dr, scale, centering):
    """(bits, mask): int64 bits [3, n, nc+2, nc+2, nc+2] of the differences of
    `boxes` [n, k, j, i] (ghosts as they are) in the frame of the cells
    0 .. nc+1, and mask [3, nc+2, nc+2, nc+2], the values that are defined.
    cell: (cc(+1) - cc(-1)) * ((0.5 * scale) / dr) at the interior cells.
    face: (cc(+1) - cc) * (scale / dr) at 0 .. nc along the component's
    direction and 1 .. nc along the two others, at the lower cell's place."""
    n, nc = boxes.shape[0], boxes.shape[1] - 2
    s, lo, hi, fa = slice(1, nc + 1), slice(0, nc), slice(2, nc + 2), slice(0, nc + 1)
    bits = np.full((3, n) + (nc + 2,) * 3, U.SENTINEL, dtype=np.int64)
    mask = np.zeros((3,) + (nc + 2,) * 3, dtype=bool)
    for d in range(3):
        ax = 2 - d   # (x is the last axis of [k, j, i])
        if centering == "cell":
            at, up, dn = [s, s, s], [s, s, s], [s, s, s]
            up[ax], dn[ax] = hi, lo
            f = (0.5 * float(scale)) / float(dr[d])
        else:
            at, up, dn = [s, s, s], [s, s, s], [s, s, s]
            at[ax], up[ax], dn[ax] = fa, slice(1, nc + 2), fa
            f = float(scale) / float(dr[d])
        g = (boxes[(slice(None),) + tuple(up)] - boxes[(slice(None),) + tuple(dn)]) * f
        bits[(d, slice(None)) + tuple(at)] = g.view(np.int64)
        mask[(d,) + tuple(at)] = True
    return bits, mask


def in_pool(bits, mask, width):
    """The frame values placed in blocks [3, n, m, m, m] with `width` ghost
    layers (m = nc + 2*width), SENTINEL everywhere else."""
    _, n, p = bits.shape[:3]
    nc = p - 2
    m = nc + 2 * width
    out = np.full((3, n, m, m, m), U.SENTINEL, dtype=np.int64)
    for d in range(3):
        frame = np.where(mask[d], bits[d], U.SENTINEL)
        if width >= 1:
            c = slice(width - 1, width + nc + 1)
            out[d][:, c, c, c] = frame
        else:
            assert not mask[d][0].any() and not mask[d][:, 0].any() and not mask[d][:, :, 0].any()
            out[d] = frame[:, 1:-1, 1:-1, 1:-1]
    return out


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
@pytest.mark.parametrize("variant", ["tile", "generic"])
@pytest.mark.parametrize("name", sorted(TREES))
def test_every_level_bitwise_against_numpy(monkeypatch, name, variant):
    _switch(monkeypatch, variant)
    be = _backend(TREES[name])
    mg, tree = be.mg, be.tree
    rng = np.random.default_rng(20261021)
    assert {tree.box_size_lvl[lvl] for lvl in be.levels()} == SIZES[name]
    if name.startswith("refined"):
        # (ref_bnds lists the coarse side: levels 2 and 3 have refinement-boundary ghosts)
        assert len(tree.lvls[1].ref_bnds) and len(tree.lvls[2].ref_bnds)
    tiled = sum(tree.box_size_lvl[lvl] in (16, 8) for lvl in be.levels())
    calls, zeros = 0, 0
    for iv in (IPHI, IRHS):
        up, filled = _filled(be, iv, rng)
        first = True
        for lvl in be.levels():
            ids, nc = _ids(be, lvl), tree.box_size_lvl[lvl]
            stored = U.stored_mask(nc)
            assert not np.array_equal(up[lvl][:, stored], filled[lvl][:, stored])   # (the fill changed the ghosts)
            for scale in SCALES:
                for centering in CENTRINGS:
                    bits, mask = block_grad(filled[lvl], tree.dr[lvl], scale, centering)
                    want = in_pool(bits, mask, 1)
                    zeros += int((want == NEG_ZERO).sum())
                    out = _sentinel((3, len(ids)) + (nc + 2,) * 3)
                    # (the first call of a variable fills the stale ghosts of every level)
                    res, n = mg.get_blocks_grad(ids, iv, out=out, ghost_width=1, scale=scale, fill=first,
                                                centering=centering)
                    first = False
                    calls += 1
                    assert res is out and n == len(ids) * int(mask[0].sum())
                    assert n == len(ids) * (nc + (centering == "face")) * nc * nc
                    assert np.array_equal(_bits(out), want), (name, iv, lvl, scale, centering, variant)
    assert zeros > 0   # (the sign of zero was compared)
    assert _launches(be, "boxes_grad") == calls
    # the tile kernel served the 16^3 and 8^3 levels, and nothing under the switch
    want_tiles = 0 if variant == "generic" else tiled * 2 * len(SCALES) * len(CENTRINGS)
    assert _launches(be, "boxes_grad_tile") == want_tiles


# -- 2. block geometry ---------------------------------------------------------------
def _plain(n, m):
    big = torch.full((3, n, m, m, m), SENT, dtype=torch.int64, device="cuda")
    return big, lambda t: [t[d] for d in range(3)]


def _off8(n, m):
    """8 B off a 16-B boundary: views starting at an odd element."""
    big = torch.full((3 * n * m ** 3 + 1,), SENT, dtype=torch.int64, device="cuda")
    assert big.data_ptr() % 16 == 0
    return big, lambda t: [t[1:].view(3, n, m, m, m)[d] for d in range(3)]


def _odd_rows(n, m):
    """An odd row stride, from a padded view."""
    p = m + 1 + m % 2
    assert p % 2 == 1
    big = torch.full((3, n, m, m + 1, p), SENT, dtype=torch.int64, device="cuda")
    return big, lambda t: [t[d][:, :, :m, :m] for d in range(3)]


def _pool(n, m):
    """Variables 1..3 of an AMR pool [box, variable, k, j, i]: pools that interleave."""
    big = torch.full((n, 5, m, m, m), SENT, dtype=torch.int64, device="cuda")
    return big, lambda t: [t[:, 1 + d] for d in range(3)]


def _separate(n, m):
    """Three allocations of their own."""
    big = [torch.full((n, m, m, m), SENT, dtype=torch.int64, device="cuda") for _ in range(3)]
    return big, lambda t: list(t)


LAYOUTS = {"plain": _plain, "off8": _off8, "odd-rows": _odd_rows, "pool": _pool, "separate": _separate}
MASKS = [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (True, True, False),
         (True, False, True), (False, True, True)]


@pytest.fixture(scope="module", params=[BOX16, U.NONCUBE], ids=["box16", "box8"])
def geo(request):
    """A tree whose level 1 holds filled random phi (shared by the geometry
    tests, which only read it): (backend, ids, filled boxes)."""
    be = _backend(request.param)
    ids = _ids(be, 1)
    nc = be.tree.box_size_lvl[1]
    be.mg.set_level(1, IPHI, _random_boxes(np.random.default_rng(100 + nc), len(ids), nc))
    omg.mg_fill_ghost_cells_lvl(be.mg, 1, IPHI)
    return be, ids, be.mg.get_level(1, IPHI)


@pytest.mark.parametrize("variant", [None, "tile", "generic"], ids=["routed", "tile", "generic"])
@pytest.mark.parametrize("centering", CENTRINGS)
@pytest.mark.parametrize("width", [0, 1, 2, 3])
def test_block_geometry(monkeypatch, geo, width, centering, variant):
    if centering == "face" and width == 0:
        with pytest.raises(ValueError, match="ghost_width >= 1"):
            geo[0].mg.get_blocks_grad(geo[1], out=_sentinel((3, len(geo[1]), 8, 8, 8)), centering="face")
        return
    _switch(monkeypatch, variant)
    be, all_ids, filled = geo
    mg = be.mg
    mg.ctx.call("reset_stats")
    nc = be.tree.box_size_lvl[1]
    m = nc + 2 * width
    rng = np.random.default_rng(10 * nc + width)
    bits, mask = block_grad(filled, be.tree.dr[1], -1.0, centering)
    for q, (name, layout) in enumerate(LAYOUTS.items()):
        for sub in (list(rng.permutation(all_ids)), list(rng.permutation(all_ids))[:len(all_ids) // 2 + 1]):
            sub = [int(i) for i in sub]
            where = [all_ids.index(i) for i in sub]
            n = len(sub)
            comps = MASKS[(q + n + width) % len(MASKS)] if name != "plain" else MASKS[0]
            big, view = layout(n, m)
            parts = view(big) if isinstance(big, list) else view(big.view(torch.float64))
            if isinstance(big, list):
                parts = [t.view(torch.float64) for t in parts]
            if name == "off8":
                assert parts[0].data_ptr() % 16 == 8
            if name == "odd-rows":
                assert parts[0].stride(2) % 2 == 1
            if name == "pool":
                assert parts[0].stride(0) == 5 * m ** 3
            want = in_pool(bits[:, where], mask, width)
            res, cells = mg.get_blocks_grad(sub, IPHI, out=parts, ghost_width=width, scale=-1.0, fill=False,
                                            centering=centering, components=comps)
            assert res is parts and cells == n * int(mask[0].sum())
            for d in range(3):
                if comps[d]:
                    assert np.array_equal(_bits(parts[d]), want[d]), (name, n, d)
                    parts[d].view(torch.int64).fill_(SENT)
            # the skipped components and everything around the blocks still hold the sentinel
            for t in (big if isinstance(big, list) else [big]):
                assert bool((t == SENT).all()), ("wrote outside the blocks or into a skipped component", name, n)
    tile = variant == "tile"   # (routed: lists this short go to the per-cell kernel)
    assert (_launches(be, "boxes_grad_tile") > 0) == tile
    assert _launches(be, "boxes_grad") == 2 * len(LAYOUTS)


@pytest.mark.parametrize("centering", CENTRINGS)
def test_three_separate_pools_equal_one_tensor(monkeypatch, geo, centering):
    _switch(monkeypatch, "tile")
    be, ids, filled = geo
    nc = be.tree.box_size_lvl[1]
    one = _sentinel((3, len(ids)) + (nc + 2,) * 3)
    three = [_sentinel((len(ids),) + (nc + 2,) * 3) for _ in range(3)]
    _, a = be.mg.get_blocks_grad(ids, out=one, ghost_width=1, scale=0.37, fill=False, centering=centering)
    _, b = be.mg.get_blocks_grad(ids, out=three, ghost_width=1, scale=0.37, fill=False, centering=centering)
    assert a == b
    want = in_pool(*block_grad(filled, be.tree.dr[1], 0.37, centering), 1)
    assert np.array_equal(_bits(one), want)
    for d in range(3):
        assert np.array_equal(_bits(three[d]), want[d])
    # the default `out` is a tensor [3, n, m, m, m] of its own
    res, c = be.mg.get_blocks_grad(ids, ghost_width=1, scale=0.37, fill=False, centering=centering)
    assert c == a and tuple(res.shape) == (3, len(ids)) + (nc + 2,) * 3
    m = np.broadcast_to(block_grad(filled, be.tree.dr[1], 0.37, centering)[1][:, None], want.shape)
    assert np.array_equal(_bits(res)[m], want[m])


# -- 3. a refined tree in one call --------------------------------------------------------
@pytest.mark.parametrize("variant", ["tile", "generic"])
@pytest.mark.parametrize("args", [U.REFINED, REFINED_RB], ids=["gs", "gsrb"])
def test_leaves_of_a_refined_tree_in_one_call(monkeypatch, args, variant):
    _switch(monkeypatch, variant)
    be = _backend(args)
    mg, tree = be.mg, be.tree
    rng = np.random.default_rng(31)
    lvls = [l for l in be.levels() if l >= 1]
    assert lvls == [1, 2, 3]
    leaves = [int(i) for l in lvls for i in tree.lvls[l].my_leaves]
    lvl_of = [l for l in lvls for _ in tree.lvls[l].my_leaves]
    assert all(len(tree.lvls[l].my_leaves) for l in lvls) and all(len(tree.lvls[l].my_parents) for l in (1, 2))
    _upload_all(be, IPHI, {l: _random_boxes(rng, len(_ids(be, l)), tree.box_size_lvl[l]) for l in be.levels()})
    got = {}
    for centering in CENTRINGS:   # (the first call fills the stale ghosts, refinement boundaries included)
        out = _sentinel((3, len(leaves), 10, 10, 10))
        _, cells = mg.get_blocks_grad(leaves, IPHI, out=out, ghost_width=1, scale=-1.0, fill=True,
                                      centering=centering)
        assert cells == len(leaves) * (512 if centering == "cell" else 576)
        got[centering] = _bits(out)
    # the coupling's own definition: differences of the blocks with their filled ghosts
    blocks, _ = mg.get_blocks(IPHI, leaves, ghost_width=1, ghosts=True, fill=True)
    blocks = blocks.cpu().numpy()
    stored = U.stored_mask(8)
    for l in lvls:   # (and those blocks are the filled boxes of the host path)
        ids, phi = _ids(be, l), mg.get_level(l, IPHI)
        for q, id_ in enumerate(ids):
            if id_ in leaves:
                assert np.array_equal(blocks[leaves.index(id_)][stored].view(np.int64), phi[q][stored].view(np.int64))
    for centering in CENTRINGS:
        want = np.full((3, len(leaves), 10, 10, 10), U.SENTINEL, dtype=np.int64)
        for l in lvls:   # (dr differs by level: f_d is per level)
            sel = [q for q, ll in enumerate(lvl_of) if ll == l]
            want[:, sel] = in_pool(*block_grad(blocks[sel], tree.dr[l], -1.0, centering), 1)
        assert np.array_equal(got[centering], want), centering
    assert _launches(be, "boxes_grad") == 2 and _launches(be, "boxes_get") == 1
    assert _launches(be, "boxes_grad_tile") == (0 if variant == "generic" else 2 * 3)
    if variant == "tile":
        assert [_launches(be, f"boxes_grad_tile@{l}") for l in lvls] == [2, 2, 2]


# -- 4. the lazy state two stand-alone cycles leave ------------------------------------------
def test_pending_shift_deferred_ghosts_and_pending_res_are_resolved_and_the_next_cycle_is_unchanged(monkeypatch):
    # (the 64 boxes of the 64^3 tree's level 1 and the 8 of level 0 take the multi-substep passes)
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", "8")
    monkeypatch.delenv("OMG_BLOCK3_COLUMN", raising=False)
    _switch(monkeypatch, "tile")
    trio = []
    for _ in range(3):
        be = DeviceBackend(parse(STREAM64))
        setup_problem(be)
        be.mg.ctx.call("set_profiling", 1)
        be.vcycle(False)
        be.vcycle(False)
        trio.append(be)
    a, b, c = trio   # a: the gradient calls; b: the reference download; c: cycles alone
    tree, top = a.tree, a.tree.highest_lvl
    ids = _ids(a, top)
    # (the cycles ended in k_gsrb4's correction form, the one that defers the ghosts)
    assert _launches(a, f"smoother_gsrb4p@{top}") >= 2
    got = {}
    for iv, fill in ((IPHI, True), (IRES, False)):
        for centering in CENTRINGS:
            out = _sentinel((3, len(ids), 18, 18, 18))
            _, cells = a.mg.get_blocks_grad(ids, iv, out=out, ghost_width=1, scale=-1.0, fill=fill,
                                            centering=centering)
            assert cells == len(ids) * (16 + (centering == "face")) * 256
            got[iv, centering] = _bits(out)
    assert _launches(a, f"boxes_grad_tile@{top}") == 4
    omg.mg_fill_ghost_cells_lvl(b.mg, top, IPHI)
    for iv in (IPHI, IRES):
        boxes = b.mg.get_level(top, iv)
        assert np.abs(boxes[:, 1:-1, 1:-1, 1:-1]).max() > 0
        for centering in CENTRINGS:
            want = in_pool(*block_grad(boxes, tree.dr[top], -1.0, centering), 1)
            assert np.array_equal(got[iv, centering], want), (iv, centering)
    ha, hc = a.vcycle(True), c.vcycle(True)
    assert float(ha).hex() == float(hc).hex()
    assert phi_digest(a) == phi_digest(c)


# -- 5. the record cache, host waits, launches per level ------------------------------------
def test_cached_lists_make_no_host_wait_and_a_fifth_replaces_the_oldest(monkeypatch):
    _switch(monkeypatch, "tile")
    be = _backend(BOX16, profile=False)
    mg, ctx = be.mg, be.mg.ctx
    ids = _ids(be, 1)
    assert len(ids) == 8
    mg.set_level(1, IRHS, _random_boxes(np.random.default_rng(23), 8, 16))
    omg.mg_fill_ghost_cells_lvl(mg, 1, IRHS)
    bits, mask = block_grad(mg.get_level(1, IRHS), be.tree.dr[1], 1.0, "face")
    lists = [ids, ids[::-1], ids[:5], ids[2:], ids[1:7]]
    outs = [_sentinel((3, len(l), 18, 18, 18)) for l in lists]
    ctx.call("synchronize")

    def get(q):
        before = ctx.host_sync_count()
        _, cells = mg.get_blocks_grad(lists[q], IRHS, out=outs[q], ghost_width=1, fill=False, centering="face")
        waits = ctx.host_sync_count() - before
        assert cells == len(lists[q]) * 17 * 256
        return waits

    def check(q):
        where = [ids.index(i) for i in lists[q]]
        assert np.array_equal(_bits(outs[q]), in_pool(bits[:, where], mask, 1)), ("list", q)

    assert [get(0), get(0)] == [0, 0]                          # a repeated list
    assert [get(1), get(2), get(3), get(0)] == [0, 0, 0, 0]    # four lists, then the first again
    for q in range(4):
        check(q)
    assert get(4) == 1                                         # a fifth waits once (it replaced list 1)
    check(4)
    assert [get(0), get(2), get(3), get(4)] == [0, 0, 0, 0]
    # the centring is part of the key (a fifth list again), and the cache is the copies' cache too
    out = _sentinel((3, 8, 18, 18, 18))
    before = ctx.host_sync_count()
    mg.get_blocks_grad(ids, IRHS, out=out, ghost_width=1, fill=False, centering="cell")
    assert ctx.host_sync_count() - before == 1
    cb, cm = block_grad(mg.get_level(1, IRHS), be.tree.dr[1], 1.0, "cell")
    assert np.array_equal(_bits(out), in_pool(cb, cm, 1))
    before = ctx.host_sync_count()
    mg.get_blocks(IRHS, ids, ghost_width=1, ghosts=True, fill=False)
    assert ctx.host_sync_count() - before == 1
    # one launch of the tile kernel per level listed: 16^3 boxes of level 1 and the 8^3 box of level -1
    ctx.call("set_profiling", 1)
    ctx.call("reset_stats")
    low = _ids(be, -1)
    assert len(low) == 1 and be.tree.box_size_lvl[-1] == 8
    mg.set_level(-1, IRHS, _random_boxes(np.random.default_rng(29), 1, 8))
    omg.mg_fill_ghost_cells_lvl(mg, -1, IRHS)
    mixed = ids[:3] + low
    pool = _sentinel((3, 4, 18, 18, 18))
    s = pool.stride()
    off = np.arange(4, dtype=np.int64) * s[1] + (1 + 18 + 324)
    cells = ctx.get_boxes_grad(IRHS, mixed, [pool[d].data_ptr() for d in range(3)], off, (1, 18, 324), 1.0, 1, False,
                               torch.cuda.current_stream().cuda_stream)
    assert cells == 3 * 17 * 256 + 9 * 64
    assert [_launches(be, k) for k in ("boxes_grad", "boxes_grad_tile", "boxes_grad_tile@1", "boxes_grad_tile@-1")] \
        == [1, 2, 1, 1]
    h = _bits(pool)
    assert np.array_equal(h[:, :3], in_pool(bits[:, :3], mask, 1))
    lb, lm = block_grad(mg.get_level(-1, IRHS), be.tree.dr[-1], 1.0, "face")
    small = np.full((3, 1, 18, 18, 18), U.SENTINEL, dtype=np.int64)
    small[:, :, :10, :10, :10] = in_pool(lb, lm, 1)   # (the 8^3 block in the corner of its 18^3 slot)
    assert np.array_equal(h[:, 3:], small)


# -- 6. stream ordering, no host wait ---------------------------------------------------------
def test_calls_are_ordered_on_the_callers_stream_without_a_host_wait(monkeypatch):
    _switch(monkeypatch, "tile")
    be = _backend(STREAM64, profile=False)
    mg, ctx, tree = be.mg, be.mg.ctx, be.tree
    ids = _ids(be, 1)
    mg.set_level(1, IPHI, _random_boxes(np.random.default_rng(9), len(ids), 16))
    omg.mg_fill_ghost_cells_lvl(mg, 1, IPHI)
    want = in_pool(*block_grad(mg.get_level(1, IPHI), tree.dr[1], 1.0, "face"), 1)
    scratch = torch.zeros(32 * 1024 * 1024, dtype=torch.float64, device="cuda")   # 256 MB
    out = _sentinel((3, len(ids), 18, 18, 18))
    mg.get_blocks_grad(ids, out=out, ghost_width=1, centering="face")   # (the list's records go up here)
    side = torch.cuda.Stream()
    ctx.call("synchronize")
    torch.cuda.synchronize()
    out.copy_(_sentinel(out.shape))
    torch.cuda.synchronize()
    syncs = ctx.host_sync_count()
    with torch.cuda.stream(side):
        for _ in range(200):   # (tens of milliseconds of queued passes)
            scratch.add_(1.0)
        kept = []
        for _ in range(3):
            _, n = mg.get_blocks_grad(ids, out=out, ghost_width=1, centering="face")
            assert n == len(ids) * 17 * 256
            kept.append(out.clone())                  # the consumer queued behind the call
            out.copy_(_sentinel(out.shape))           # and a writer behind the consumer
        still_running = not side.query()
    assert ctx.host_sync_count() == syncs
    assert still_running, "the queued passes had finished: the calls were not made under load"
    torch.cuda.synchronize()
    for k in kept:
        assert np.array_equal(_bits(k), want)
    assert float(scratch[0]) == 200.0


# -- 7. several ranks -----------------------------------------------------------------------
def _by_id(id_, nc=8):
    """The data of a box, the same on whichever rank owns it."""
    return _random_boxes(np.random.default_rng(1000 + int(id_)), 1, nc)[0]


def _leaf_run(be, rank, reduce):
    mg, tree = be.mg, be.tree
    lvls = [l for l in be.levels() if l >= 1]
    for l in be.levels():   # every box by its id (collective for phi, and on every rank for empty levels too)
        ids, nc = _ids(be, l), tree.box_size_lvl[l]
        data = np.stack([_by_id(i, nc) for i in ids]) if ids else np.zeros((0,) + (nc + 2,) * 3)
        mg.set_level(l, IPHI, data)
    leaves = [int(i) for l in lvls for i in tree.lvls[l].my_leaves]
    if tree.n_cpu > 1:   # a box of another rank is an error, and the context goes on
        other = next(int(i) for l in lvls for i in tree.lvls[l].leaves if int(tree.rank[int(i)]) != rank)
        with pytest.raises(omg.device.OmgError, match="omg_get_boxes_grad.*not owned"):
            mg.get_blocks_grad([other], ghost_width=1, fill=False)
    res = {}
    for centering in CENTRINGS:   # (fill=True: collective, across rank and refinement boundaries)
        out = _sentinel((3, len(leaves), 10, 10, 10))
        _, cells = mg.get_blocks_grad(leaves, IPHI, out=out, ghost_width=1, scale=-1.0, fill=True,
                                      centering=centering)
        assert cells == len(leaves) * (512 if centering == "cell" else 576)
        h = _bits(out) if leaves else np.zeros((3, 0, 10, 10, 10), np.int64)
        res[centering] = {id_: h[:, q] for q, id_ in enumerate(leaves)}
    remote = int(sum(tree.rank[tree.neighbors[i, nb]] != rank for i in leaves for nb in range(6)
                     if tree.neighbors[i, nb] > 0))
    return res, remote


@pytest.fixture(scope="module")
def one_rank_leaves():
    """The leaves' gradients of the refined tree on one rank, checked against numpy."""
    be = _backend(U.REFINED, False)
    res, _ = _leaf_run(be, 0, None)
    tree = be.tree
    for l in (1, 2, 3):
        ids, phi = _ids(be, l), be.mg.get_level(l, IPHI)
        leaves = [int(i) for i in tree.lvls[l].my_leaves]
        sel = [ids.index(i) for i in leaves]
        for centering in CENTRINGS:
            want = in_pool(*block_grad(phi[sel], tree.dr[l], -1.0, centering), 1)
            for q, id_ in enumerate(leaves):
                assert np.array_equal(res[centering][id_], want[:, q]), (l, id_, centering)
    return res


def test_two_ranks_give_the_one_rank_bits(monkeypatch, one_rank_leaves):
    _switch(monkeypatch, "tile")
    out = run_loopback(U.REFINED, 2, _leaf_run, timeout=120)
    assert all(r[1] > 0 for r in out)   # (both ranks have leaf faces whose neighbour is remote)
    for centering in CENTRINGS:
        merged = {}
        for r, _ in out:
            assert r[centering] and not set(r[centering]) & set(merged)
            merged.update(r[centering])
        assert sorted(merged) == sorted(one_rank_leaves[centering])
        for id_, want in one_rank_leaves[centering].items():
            assert np.array_equal(merged[id_], want), (centering, id_)


def test_replicated_level_own_boxes_only(monkeypatch):
    _switch(monkeypatch, None)

    def body(be, rank, reduce):
        lvl = 0
        assert be.rep_lvl >= lvl
        tree, ids = be.tree, _ids(be, lvl)
        nc = tree.box_size_lvl[lvl]
        assert 0 < len(ids) < len(tree.lvls[lvl].ids)
        be.set_level(lvl, IRHS, _random_boxes(np.random.default_rng(17 + rank), len(ids), nc))   # (collective)
        omg.mg_fill_ghost_cells_lvl(be.mg, lvl, IRHS)
        filled = be.mg.get_level(lvl, IRHS)
        total = 0
        for centering in CENTRINGS:
            out = _sentinel((3, len(ids)) + (nc + 2,) * 3)
            _, cells = be.mg.get_blocks_grad(ids, IRHS, out=out, ghost_width=1, fill=False, centering=centering)
            bits, mask = block_grad(filled, tree.dr[lvl], 1.0, centering)
            assert cells == len(ids) * int(mask[0].sum())
            assert np.array_equal(_bits(out), in_pool(bits, mask, 1))
            total += cells
        other = next(int(i) for i in tree.lvls[lvl].ids if int(i) not in ids)
        with pytest.raises(omg.device.OmgError, match="omg_get_boxes_grad.*own boxes"):
            be.mg.get_blocks_grad(ids[:1] + [other], IRHS, ghost_width=1, fill=False)
        return total

    res = run_loopback(STREAM64, 2, body, timeout=120, rep_cells=8 * 16 ** 3)
    assert sum(res) == 8 * (16 ** 3 + 17 * 256)


# -- 8. errors before any launch -------------------------------------------------------------
def test_bad_pointers_are_errors_before_any_launch_and_the_context_stays_usable(monkeypatch, geo):
    _switch(monkeypatch, "tile")
    be, ids, filled = geo
    ctx = be.mg.ctx
    ctx.call("reset_stats")
    nc = be.tree.box_size_lvl[1]
    m, n = nc + 2, len(ids)
    stride = (1, m, m * m)
    off = np.arange(n, dtype=np.int64) * m ** 3 + (1 + m + m * m)
    good = _sentinel((3, n, m, m, m))
    host = np.zeros(n * m ** 3)
    p = [good[d].data_ptr() for d in range(3)]
    far = off.copy()
    far[-1] += 1 << 34    # (a block 128 GiB up: past the end of any allocation)
    low = off.copy()
    low[0] -= 1 << 34
    past = "a block reaches past the end of the pointer's allocation"
    before = "a block starts before the pointer's allocation"
    cases = [("the pointer is not device memory", (host.ctypes.data, 0, 0), off, 0),
             ("the pointer is not device memory", (p[0], p[1], host.ctypes.data), off, 1),
             (past, (0, p[1], 0), far, 0),
             (past, (p[0], p[1], p[2]), far, 1),
             (before, (p[0], 0, 0), low, 0),
             (before, (0, 0, p[2]), low, 1),
             ("components 0 and 1 share one pointer", (p[0], p[0], 0), off, 0),
             ("components 1 and 2 share one pointer", (p[2], p[1], p[1]), off, 1)]
    for what, ptrs, o, centering in cases:
        with pytest.raises(omg.device.OmgError) as ex:
            ctx.get_boxes_grad(IPHI, ids, ptrs, o, stride, -1.0, centering, False)
        assert str(ex.value) == "omg_get_boxes_grad: " + what
        assert _launches(be, "boxes_grad") == 0
        assert (_bits(good) == U.SENTINEL).all()
    # the context stays usable
    for centering in (0, 1):
        ok = _sentinel((3, n, m, m, m))
        cells = ctx.get_boxes_grad(IPHI, ids, [ok[d].data_ptr() for d in range(3)], off, stride, -1.0, centering,
                                   False)
        assert cells == n * (nc + centering) * nc * nc
        assert np.array_equal(_bits(ok), in_pool(*block_grad(filled, be.tree.dr[1], -1.0, CENTRINGS[centering]), 1))
