"""omg_put_boxes / omg_get_boxes on the GPU: blocks of an AMR pool in device
memory <-> the boxes, against the host path (omg_upload_level /
omg_download_level).

1. round trips on every level of four trees (boxes of 16, 8, 5 and 6 cells),
   tile kernel and per-cell kernel, with and without the face ghosts;
2. block geometry: pool ghost widths 0..3, a base 8 B off a 16-B boundary, an
   odd row stride, a pool variable slice, permuted and partial lists;
3. the leaves of a refined tree, three levels in one call;
4. the AMR coupling end to end against the host path;
5. the state a cycle leaves, and stored boundary data in the rhs ghosts;
6. the record cache and its host waits; stream ordering;
7. several ranks on the loopback transport, and a replicated coarse level.

Every comparison is on bits: a copy has no tolerance."""
import numpy as np
import pytest
import torch

from tests import denseutil as U
from tests.apiwalk import PER128, TREES
from tests.mgdriver import DeviceBackend, omg, parse, phi_digest, run_loopback, setup_problem

pytestmark = pytest.mark.gpu

IPHI, IRHS, IRES = 1, 2, 4
BOX16 = "16 32 32 32 1 v gsrb lpl 0 d0 sol 1 lb 0"
BOX5 = "5 10 10 10 1 v gsrb lpl 0 d0 sol 1 lb 0"      # odd box size (denseutil.odd_box_tree)
BOX6 = "6 12 12 12 1 v gs lpl 0 d0 sol 1 lb 0"        # its coarsest level has one 3^3 box
STREAM64 = "16 64 64 64 1 v gsrb lpl 0 per sol 1 lb 0"
REFINED_RB = "8 32 32 32 1 v gsrb lpl 0 sol sol 3 lb 0"
SENT = int(U.SENTINEL)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(a, b, msg=None):
    assert np.array_equal(_bits(a), _bits(b)), msg


def _switch(monkeypatch, variant):
    """variant: None the library's routing (short lists: the per-cell kernel),
    "tile" the tile kernel wherever it can serve, "8" / "16" the same with
    that variant for blocks off a 16-B boundary, "generic" the per-cell kernel."""
    for k in ("OMG_BOXES_GENERIC", "OMG_BOXES_TILE", "OMG_BOXES_ODD"):
        monkeypatch.delenv(k, raising=False)
    if variant == "generic":
        monkeypatch.setenv("OMG_BOXES_GENERIC", "1")
    elif variant:
        monkeypatch.setenv("OMG_BOXES_TILE", "1")
        if variant != "tile":
            monkeypatch.setenv("OMG_BOXES_ODD", variant)


def _backend(args, profile=True):
    cfg = parse(args)
    be = U.OddBoxBackend(cfg) if cfg["box"] % 2 else DeviceBackend(cfg)
    if profile:
        be.mg.ctx.call("set_profiling", 1)
    return be


def _random_boxes(rng, n, nc):
    return rng.standard_normal((n, nc + 2, nc + 2, nc + 2))


def _sentinel(shape):
    return torch.full(tuple(shape), SENT, dtype=torch.int64, device="cuda").view(torch.float64)


def _launches(be, name):
    be.mg.ctx.call("synchronize")
    return be.mg.ctx.kernel_stats(name)[0]


def _ids(be, lvl):
    return [int(i) for i in be.tree.lvls[lvl].my_ids]


def _interior(nc):
    return np.pad(np.ones((nc,) * 3, bool), 1)


# -- 1. round trips against the host path --------------------------------------
@pytest.mark.parametrize("variant", ["tile", "generic"])
@pytest.mark.parametrize("args", [BOX16, U.NONCUBE, BOX5, BOX6], ids=["box16", "box8", "box5", "box6"])
def test_round_trip_on_every_level(monkeypatch, args, variant):
    _switch(monkeypatch, variant)
    be = _backend(args)
    mg = be.mg
    rng = np.random.default_rng(20261020)
    sizes = set()
    for lvl in be.levels():
        ids, nc = _ids(be, lvl), be.tree.box_size_lvl[lvl]
        sizes.add(nc)
        stored, inner = U.stored_mask(nc), _interior(nc)
        # get, with the face ghosts as they stand
        boxes = _random_boxes(rng, len(ids), nc)
        mg.set_level(lvl, IPHI, boxes)
        out = _sentinel((len(ids),) + (nc + 2,) * 3)
        got, cells = mg.get_blocks(IPHI, ids, out=out, ghost_width=1, ghosts=True, fill=False)
        assert got is out and cells == len(ids) * (nc ** 3 + 6 * nc ** 2)
        h = out.cpu().numpy()
        _same(h[:, stored], mg.get_level(lvl, IPHI)[:, stored], ("get", lvl))
        _same(h[:, stored], boxes[:, stored])
        assert (_bits(h)[:, ~stored] == U.SENTINEL).all(), ("edges and corners", lvl)
        # put, with the face ghosts
        blocks = _random_boxes(rng, len(ids), nc)
        assert mg.set_blocks(IRHS, torch.from_numpy(blocks).cuda(), ids, ghost_width=1, ghosts=True) == cells
        _same(mg.get_level(lvl, IRHS)[:, stored], blocks[:, stored], ("put", lvl))
        # put, interior only: the ghost slots keep what set_level put there
        pat = _random_boxes(rng, len(ids), nc)
        mg.set_level(lvl, IRHS, pat)
        blocks = _random_boxes(rng, len(ids), nc)
        assert mg.set_blocks(IRHS, torch.from_numpy(blocks).cuda(), ids, ghost_width=1) == len(ids) * nc ** 3
        back = mg.get_level(lvl, IRHS)
        _same(back[:, inner], blocks[:, inner], ("put interior", lvl))
        _same(back[:, stored & ~inner], pat[:, stored & ~inner], ("put kept the ghosts", lvl))
        # get, interior only
        out = _sentinel((len(ids),) + (nc + 2,) * 3)
        mg.get_blocks(IRHS, ids, out=out, ghost_width=1, fill=False)
        h = out.cpu().numpy()
        _same(h[:, inner], blocks[:, inner])
        assert (_bits(h)[:, ~inner] == U.SENTINEL).all()
    assert sizes == {BOX16: {16, 8, 4, 2}, U.NONCUBE: {8, 4, 2}, BOX5: {5}, BOX6: {6, 3}}[args]
    n_lvls = len(be.levels())
    assert _launches(be, "boxes_put") == 2 * n_lvls and _launches(be, "boxes_get") == 2 * n_lvls
    tiles = 0 if variant == "generic" else 2 * sum(be.tree.box_size_lvl[lvl] in (16, 8) for lvl in be.levels())
    assert _launches(be, "boxes_put_tile") == tiles and _launches(be, "boxes_get_tile") == tiles


# -- 2. block geometry ---------------------------------------------------------------
def _plain(n, m):
    big = torch.full((n, m, m, m), SENT, dtype=torch.int64, device="cuda")
    return big, lambda t: t


def _off8(n, m):
    """8 B off a 16-B boundary: a view starting at an odd element."""
    big = torch.full((n * m ** 3 + 1,), SENT, dtype=torch.int64, device="cuda")
    assert big.data_ptr() % 16 == 0
    return big, lambda t: t[1:].view(n, m, m, m)


def _odd_rows(n, m):
    """An odd row stride, from a padded view."""
    p = m + 1 + m % 2
    assert p % 2 == 1
    big = torch.full((n, m, m + 1, p), SENT, dtype=torch.int64, device="cuda")
    return big, lambda t: t[:, :, :m, :m]


def _pool(n, m):
    """Variable 1 of an AMR pool [box, variable, k, j, i]."""
    big = torch.full((n, 3, m, m, m), SENT, dtype=torch.int64, device="cuda")
    return big, lambda t: t[:, 1]


LAYOUTS = {"plain": _plain, "off8": _off8, "odd-rows": _odd_rows, "pool": _pool}


@pytest.mark.parametrize("variant", [None, "tile", "8", "16", "generic"],
                         ids=["routed", "tile", "odd8", "odd16", "generic"])
@pytest.mark.parametrize("width", [0, 1, 2, 3])
@pytest.mark.parametrize("args", [BOX16, U.NONCUBE], ids=["box16", "box8"])
def test_block_geometry(monkeypatch, args, width, variant):
    _switch(monkeypatch, variant)
    be = _backend(args)
    mg, lvl = be.mg, 1
    all_ids, nc = _ids(be, lvl), be.tree.box_size_lvl[lvl]
    m, w = nc + 2 * width, width
    ghosts = width >= 1
    rng = np.random.default_rng(100 * nc + width)
    stored, inner = U.stored_mask(nc), _interior(nc)
    moved = stored if ghosts else inner
    core = (slice(None),) + (slice(w - 1, w + nc + 1),) * 3 if ghosts else None
    for name, layout in LAYOUTS.items():
        for sub in (list(rng.permutation(all_ids)), list(rng.permutation(all_ids))[:len(all_ids) // 2 + 1]):
            sub = [int(i) for i in sub]
            where = [all_ids.index(i) for i in sub]
            n = len(sub)
            big, view = layout(n, m)
            bits, blocks = view(big), view(big.view(torch.float64))
            if name == "off8":
                assert blocks.data_ptr() % 16 == 8
            if name == "odd-rows":
                assert blocks.stride(2) % 2 == 1
            if name == "pool":
                assert blocks.stride(0) == 3 * m ** 3

            def cut(a):   # the (nc+2)^3 part of blocks [n, m, m, m] around the interior
                if ghosts:
                    return a[core]
                return np.pad(a[:, w:w + nc, w:w + nc, w:w + nc], ((0, 0),) + ((1, 1),) * 3)

            # get: the copied cells arrive, everything else of the pool still holds the sentinel
            boxes = _random_boxes(rng, len(all_ids), nc)
            mg.set_level(lvl, IPHI, boxes)
            got, cells = mg.get_blocks(IPHI, sub, out=blocks, ghost_width=width, ghosts=ghosts, fill=False)
            assert got is blocks and cells == n * int(moved.sum())
            h = cut(blocks.cpu().numpy())
            _same(h[:, moved], boxes[where][:, moved], ("get", name, n))
            sel = np.zeros((n, m, m, m), dtype=bool)
            if ghosts:
                sel[core] = moved
            else:
                sel[:, w:w + nc, w:w + nc, w:w + nc] = True
            bits[torch.from_numpy(sel).cuda()] = SENT
            assert bool((big == SENT).all()), ("get wrote outside the copied cells", name, n)
            # put: the listed boxes take the cells, the others keep theirs, the source stands
            pat = _random_boxes(rng, len(all_ids), nc)
            mg.set_level(lvl, IRHS, pat)
            src = rng.standard_normal((n, m, m, m))
            blocks.copy_(torch.from_numpy(src))
            before = big.clone()
            assert mg.set_blocks(IRHS, blocks, sub, ghost_width=width, ghosts=ghosts) == cells
            want = pat.copy()
            tmp = want[where]
            tmp[:, moved] = cut(src)[:, moved]
            want[where] = tmp
            _same(mg.get_level(lvl, IRHS)[:, stored], want[:, stored], ("put", name, n))
            assert torch.equal(big, before), "put changed its source"
    tile = variant in ("tile", "8", "16")   # (routed: lists this short go to the per-cell kernel)
    assert (_launches(be, "boxes_put_tile") > 0) == tile and (_launches(be, "boxes_get_tile") > 0) == tile


# -- 3. a refined tree in one call --------------------------------------------------------
@pytest.mark.parametrize("variant", ["tile", "generic"])
def test_leaves_of_a_refined_tree_in_one_call(monkeypatch, variant):
    _switch(monkeypatch, variant)
    be = _backend(U.REFINED)
    mg, tree = be.mg, be.tree
    rng = np.random.default_rng(31)
    lvls = [l for l in be.levels() if l >= 1]
    assert lvls == [1, 2, 3]
    leaves = [int(i) for l in lvls for i in tree.lvls[l].my_leaves]
    assert all(len(tree.lvls[l].my_leaves) for l in lvls) and all(len(tree.lvls[l].my_parents) for l in (1, 2))
    pat = {l: _random_boxes(rng, len(_ids(be, l)), 8) for l in lvls}
    for l in lvls:
        mg.set_level(l, IRHS, pat[l])
    src = rng.standard_normal((len(leaves), 10, 10, 10))
    assert mg.set_blocks(IRHS, torch.from_numpy(src).cuda(), leaves, ghost_width=1) == len(leaves) * 512
    inner, stored = _interior(8), U.stored_mask(8)
    want = {}
    for l in lvls:
        ids = _ids(be, l)
        want[l] = pat[l].copy()
        for q, id_ in enumerate(ids):
            if id_ in leaves:   # (every leaf's interior arrives, parents keep their values)
                want[l][q][inner] = src[leaves.index(id_)][inner]
        _same(mg.get_level(l, IRHS)[:, stored], want[l][:, stored], ("level", l))
    out = _sentinel((len(leaves), 10, 10, 10))
    _, cells = mg.get_blocks(IRHS, leaves, out=out, ghost_width=1, ghosts=True, fill=False)
    assert cells == len(leaves) * (512 + 384)
    h = out.cpu().numpy()
    for l in lvls:
        ids = _ids(be, l)
        for q, id_ in enumerate(ids):
            if id_ in leaves:
                _same(h[leaves.index(id_)][stored], want[l][q][stored])
    assert _launches(be, "boxes_put") == 1 and _launches(be, "boxes_get") == 1
    assert _launches(be, "boxes_put_tile") == (0 if variant == "generic" else 3)


# -- 4. the AMR coupling end to end -----------------------------------------------------
@pytest.mark.parametrize("args", [U.REFINED, REFINED_RB], ids=["gs", "gsrb"])
def test_amr_coupling_matches_the_host_path(monkeypatch, args):
    _switch(monkeypatch, "tile")
    a, b = _backend(args, False), _backend(args, False)
    for be in (a, b):
        setup_problem(be)
    tree = a.tree
    lvls = [l for l in a.levels() if l >= 1]
    leaves = [int(i) for l in lvls for i in tree.lvls[l].my_leaves]
    rng = np.random.default_rng(41)
    inner, stored = _interior(8), U.stored_mask(8)
    # the new right-hand side of every leaf: the problem's own, scaled and perturbed
    src = np.zeros((len(leaves), 10, 10, 10))
    for l in lvls:
        ids, rhs = _ids(a, l), a.mg.get_level(l, IRHS)
        for q, id_ in enumerate(ids):
            if id_ in leaves:
                src[leaves.index(id_)][inner] = 0.5 * rhs[q][inner] + 1e-2 * rng.standard_normal(512)
                rhs[q][inner] = src[leaves.index(id_)][inner]
        a.mg.set_level(l, IRHS, rhs)                                   # (a) the host path
    b.mg.set_blocks(IRHS, torch.from_numpy(src).cuda(), leaves, ghost_width=1)   # (b) blocks
    hist = []
    for be in (a, b):
        hist.append([be.fmg(False, True), be.vcycle(True), be.vcycle(True)])
    assert [float(x).hex() for x in hist[0]] == [float(x).hex() for x in hist[1]]
    omg.mg_fill_ghost_cells(a.mg, IPHI)
    out = _sentinel((len(leaves), 10, 10, 10))
    _, cells = b.mg.get_blocks(IPHI, leaves, out=out, ghost_width=1, ghosts=True, fill=True)
    assert cells == len(leaves) * (512 + 384)
    h = out.cpu().numpy()
    for l in lvls:
        ids, phi = _ids(a, l), a.mg.get_level(l, IPHI)
        for q, id_ in enumerate(ids):
            if id_ in leaves:
                _same(h[leaves.index(id_)][stored], phi[q][stored], ("phi", l, id_))
    assert np.abs(h[:, inner]).max() > 0


# -- 5. the state a cycle leaves ----------------------------------------------------------
def _problem(args, store_bc=False):
    be = DeviceBackend(parse(args))
    setup_problem(be)
    if store_bc:
        omg.mg_phi_bc_store(be.mg)
    be.mg.ctx.call("set_profiling", 1)
    return be


def test_blocks_meet_a_pending_shift_deferred_ghosts_and_a_pending_res(monkeypatch):
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", "64")
    monkeypatch.delenv("OMG_BLOCK3_COLUMN", raising=False)
    _switch(monkeypatch, "tile")
    a, b, ref = _problem(PER128), _problem(PER128), _problem(PER128)
    top = a.tree.highest_lvl
    ids = _ids(a, top)
    stored = U.stored_mask(16)
    for be in (a, b, ref):
        be.vcycle(False)
        be.vcycle(False)
    # (the cycles ended in k_gsrb4's correction form, the one that defers the ghosts)
    assert _launches(a, f"smoother_gsrb4p@{top}") >= 2
    got = {}
    for iv, fill in ((IPHI, True), (IRHS, False), (IRES, False)):
        out = _sentinel((len(ids), 18, 18, 18))
        _, cells = a.mg.get_blocks(iv, ids, out=out, ghost_width=1, ghosts=True, fill=fill)
        assert cells == len(ids) * (16 ** 3 + 6 * 256)
        got[iv] = out.cpu().numpy()
    # a twin that ran the same cycles, read through the host path
    omg.mg_fill_ghost_cells(ref.mg, IPHI)
    for iv in (IPHI, IRHS, IRES):
        _same(got[iv][:, stored], ref.mg.get_level(top, iv)[:, stored], ("after two cycles", iv))
        assert (_bits(got[iv])[:, ~stored] == U.SENTINEL).all()
    # a third cycle gives the bits of a twin that made no gets
    assert float(a.vcycle(True)).hex() == float(b.vcycle(True)).hex()
    # a put of phi between cycles is set_level's
    rng = np.random.default_rng(3)
    new_phi = 0.5 * a.mg.get_level(top, IPHI) + 1e-3 * rng.standard_normal((len(ids), 18, 18, 18))
    a.mg.set_blocks(IPHI, torch.from_numpy(new_phi).cuda(), ids, ghost_width=1, ghosts=True)
    b.mg.set_level(top, IPHI, new_phi)
    assert float(a.vcycle(True)).hex() == float(b.vcycle(True)).hex()
    assert phi_digest(a) == phi_digest(b)
    assert _launches(a, f"boxes_get_tile@{top}") == 3 and _launches(a, f"boxes_put_tile@{top}") == 1


def test_put_keeps_or_overwrites_the_stored_boundary_data(monkeypatch):
    _switch(monkeypatch, "tile")
    be = _problem(TREES["mx2_helm64_box16"], store_bc=True)
    mg, top = be.mg, be.tree.highest_lvl
    ids = _ids(be, top)
    stored, inner = U.stored_mask(16), _interior(16)
    face = stored & ~inner
    rhs0 = mg.get_level(top, IRHS)
    assert np.count_nonzero(rhs0[:, face])   # (the stored boundary values are there)
    rng = np.random.default_rng(5)
    blocks = rng.standard_normal((len(ids), 18, 18, 18))
    mg.set_blocks(IRHS, torch.from_numpy(blocks).cuda(), ids, ghost_width=1, ghosts=False)
    back = mg.get_level(top, IRHS)
    _same(back[:, inner], blocks[:, inner])
    _same(back[:, face], rhs0[:, face], "ghosts=False keeps the rhs ghost slots")
    mg.set_blocks(IRHS, torch.from_numpy(blocks).cuda(), ids, ghost_width=1, ghosts=True)
    _same(mg.get_level(top, IRHS)[:, stored], blocks[:, stored], "ghosts=True overwrites them, as set_level")


# -- 6. the record cache, host waits, stream ordering ----------------------------------------
def test_cached_lists_make_no_host_wait_and_a_fifth_replaces_the_oldest(monkeypatch):
    _switch(monkeypatch, "tile")
    be = _backend(BOX16, profile=False)
    mg, ctx = be.mg, be.mg.ctx
    ids = _ids(be, 1)
    assert len(ids) == 8
    boxes = _random_boxes(np.random.default_rng(23), 8, 16)
    mg.set_level(1, IRHS, boxes)
    lists = [ids, ids[::-1], ids[:5], ids[2:], ids[1:7]]
    outs = [_sentinel((len(l), 16, 16, 16)) for l in lists]
    ctx.call("synchronize")

    def get(q):
        before = ctx.host_sync_count()
        _, cells = mg.get_blocks(IRHS, lists[q], out=outs[q], fill=False)
        waits = ctx.host_sync_count() - before
        assert cells == len(lists[q]) * 4096
        return waits

    def check(q):
        where = [ids.index(i) for i in lists[q]]
        _same(outs[q].cpu().numpy(), boxes[where][:, 1:17, 1:17, 1:17], ("list", q))

    assert [get(0), get(0)] == [0, 0]                          # a repeated list
    assert [get(1), get(2), get(3), get(0)] == [0, 0, 0, 0]    # four lists, then the first again
    for q in range(4):
        check(q)
    assert get(4) == 1                                         # a fifth waits once (it replaced list 1)
    check(4)
    assert [get(0), get(2), get(3), get(4)] == [0, 0, 0, 0]
    # one other box_off entry is another list: block 2 stays empty, block 3 is filled
    pool = _sentinel((4, 16, 16, 16))
    three = ids[:3]
    for off in ([0, 4096, 2 * 4096], [0, 4096, 3 * 4096]):
        assert ctx.get_boxes(IRHS, three, pool.data_ptr(), off, (1, 16, 256), 0, False,
                             torch.cuda.current_stream().cuda_stream) == 3 * 4096
        h = pool.cpu().numpy()
        last = off[2] // 4096
        _same(h[[0, 1, last]], boxes[:3][:, 1:17, 1:17, 1:17])
        assert (_bits(h[5 - last]) == U.SENTINEL).all()
        pool.copy_(_sentinel((4, 16, 16, 16)))


def test_calls_are_ordered_on_the_callers_stream_without_a_host_wait(monkeypatch):
    _switch(monkeypatch, "tile")
    be = _backend(STREAM64, profile=False)
    mg, ctx = be.mg, be.mg.ctx
    ids = _ids(be, 1)
    first = torch.from_numpy(np.random.default_rng(9).standard_normal((len(ids), 18, 18, 18))).cuda()
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
        n_put = mg.set_blocks(IRHS, src, ids, ghost_width=1, ghosts=True)
        src.fill_(-1.0)
        out = _sentinel((len(ids), 18, 18, 18))
        _, n_get = mg.get_blocks(IRHS, ids, out=out, ghost_width=1, ghosts=True, fill=False)
        kept = out.clone()
        still_running = not side.query()
    assert ctx.host_sync_count() == syncs
    assert still_running, "the queued passes had finished: the calls were not made under load"
    assert n_put == n_get == len(ids) * (4096 + 6 * 256)
    torch.cuda.synchronize()
    stored = U.stored_mask(16)
    _same(kept.cpu().numpy()[:, stored], first.cpu().numpy()[:, stored])
    assert float(scratch[0]) == 200.0


# -- 7. several ranks -----------------------------------------------------------------------
def _by_id(id_, nc=8):
    """The data of a box, the same on whichever rank owns it."""
    return np.random.default_rng(1000 + int(id_)).standard_normal((nc + 2,) * 3)


def _leaf_run(be, rank, reduce):
    mg, tree = be.mg, be.tree
    lvls = [l for l in be.levels() if l >= 1]
    for l in be.levels():   # every box by its id (collective for phi, and on every rank for empty levels too)
        ids, nc = _ids(be, l), tree.box_size_lvl[l]
        data = np.stack([_by_id(i, nc) for i in ids]) if ids else np.zeros((0,) + (nc + 2,) * 3)
        mg.set_level(l, IPHI, data)
    leaves = [int(i) for l in lvls for i in tree.lvls[l].my_leaves]
    src = np.stack([2.0 * _by_id(i) for i in leaves]) if leaves else np.zeros((0, 10, 10, 10))
    blocks = torch.from_numpy(src).cuda()
    none = torch.zeros((0, 10, 10, 10), dtype=torch.float64, device="cuda")
    # two collective puts: rank 0's leaves while the others list nothing, then the reverse
    n_put = mg.set_blocks(IPHI, blocks if rank == 0 else none, leaves if rank == 0 else [], ghost_width=1)
    n_put += mg.set_blocks(IPHI, none if rank == 0 else blocks, [] if rank == 0 else leaves, ghost_width=1)
    assert n_put == len(leaves) * 512
    # a box of another rank is an error, and the context goes on
    if tree.n_cpu > 1:
        other = next(int(i) for l in lvls for i in tree.lvls[l].leaves if int(tree.rank[int(i)]) != rank)
        with pytest.raises(omg.device.OmgError, match="omg_get_boxes.*not owned"):
            mg.get_blocks(IRHS, [other], ghost_width=1, fill=False)
    out = _sentinel((len(leaves), 10, 10, 10))
    _, cells = mg.get_blocks(IPHI, leaves, out=out, ghost_width=1, ghosts=True, fill=True)
    assert cells == len(leaves) * (512 + 384)
    h = _bits(out.cpu().numpy()) if leaves else np.zeros((0, 10, 10, 10), np.int64)
    return {id_: h[q] for q, id_ in enumerate(leaves)}


@pytest.fixture(scope="module")
def one_rank_leaves():
    be = _backend(U.REFINED, False)
    return _leaf_run(be, 0, None)


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_put_and_get_their_own_leaves(monkeypatch, one_rank_leaves, world):
    _switch(monkeypatch, "tile")
    res = run_loopback(U.REFINED, world, _leaf_run, timeout=120)
    assert all(len(r) for r in res)
    merged = {}
    for r in res:
        assert not set(r) & set(merged)
        merged.update(r)
    assert sorted(merged) == sorted(one_rank_leaves)
    stored = U.stored_mask(8)
    for id_, want in one_rank_leaves.items():
        assert np.array_equal(merged[id_][stored], want[stored]), id_
        assert (merged[id_][~stored] == U.SENTINEL).all()
        _same(merged[id_][_interior(8)], (2.0 * _by_id(id_))[_interior(8)])


def test_replicated_level_get_own_boxes_put_refused(monkeypatch):
    _switch(monkeypatch, None)

    def body(be, rank, reduce):
        lvl = 0
        assert be.rep_lvl >= lvl
        tree, ids = be.tree, _ids(be, lvl)
        nc = tree.box_size_lvl[lvl]
        assert 0 < len(ids) < len(tree.lvls[lvl].ids)
        boxes = np.random.default_rng(17 + rank).standard_normal((len(ids), nc + 2, nc + 2, nc + 2))
        be.set_level(lvl, IRHS, boxes)   # (collective on a replicated level)
        out = _sentinel((len(ids),) + (nc + 2,) * 3)
        _, cells = be.mg.get_blocks(IRHS, ids, out=out, ghost_width=1, ghosts=True, fill=False)
        stored = U.stored_mask(nc)
        assert cells == len(ids) * int(stored.sum())
        _same(out.cpu().numpy()[:, stored], boxes[:, stored])
        other = next(int(i) for i in tree.lvls[lvl].ids if int(i) not in ids)
        with pytest.raises(omg.device.OmgError, match="omg_get_boxes"):
            be.mg.get_blocks(IRHS, ids[:1] + [other], ghost_width=1, fill=False)
        with pytest.raises(omg.device.OmgError, match="omg_put_boxes.*omg_upload_level"):
            be.mg.set_blocks(IRHS, out, ids, ghost_width=1)
        return cells

    res = run_loopback(STREAM64, 2, body, timeout=120, rep_cells=8 * 16 ** 3)
    assert sum(res) == 8 * (16 ** 3 + 6 * 256)
