"""omg_put_boxes_div on the GPU: the divergence of a vector field, cell- or
face-centred, from blocks of up to three component pools into a variable.

The expected values never come from the code under test: they are numpy's
(a - b) * f on the pools the test generated, summed in the order x, y, z
(block_div below), f = (0.5 * scale) / dr at the cells and scale / dr at the
faces.  Every comparison is on int64 bit views, the sign of zero included:
a subtraction, a multiplication and the additions as written have no
tolerance.  A level is compared whole, stored ghosts included: they and the
boxes not listed must keep the bits they had.

 1. every level of five trees (boxes of 16, 8, 6, 5, 4, 3 and 2 cells), rhs and
    phi, three scales, both centrings, the tile and the per-cell kernel;
 2. never read: NaN in every pool element outside the named read set;
 3. never written: iv's ghosts, the other variables, the boxes not listed;
 4. block geometry under the routed, the tile and the per-cell kernel;
 5. the leaves of a three-level tree in one call, each level with its own dr;
 6. the path it replaces (numpy divergence, set_blocks) on the lazy state two
    stand-alone cycles leave: the next cycle gives the same bits;
 7. face-centred divergence of the face-centred gradient against mg_apply_op;
 8. the record cache, its host waits, launches per level;
 9. stream ordering without a host wait;
10. two loopback ranks against one;
11. errors on a real context before any launch."""
import numpy as np
import pytest
import torch

from tests import denseutil as U
from tests.mgdriver import DeviceBackend, omg, parse, phi_digest, run_loopback, setup_problem

pytestmark = pytest.mark.gpu

IPHI, IRHS, IOLD, IRES = 1, 2, 3, 4
BOX16 = "16 32 32 32 1 v gsrb lpl 0 d0 sol 1 lb 0"     # levels of 16, 8, 4, 2
BOX5 = "5 10 10 10 1 v gsrb lpl 0 d0 sol 1 lb 0"       # odd box size (denseutil.odd_box_tree)
BOX6 = "6 12 12 12 1 v gs lpl 0 d0 sol 1 lb 0"         # its coarsest level has one 3^3 box
STREAM64 = "16 64 64 64 1 v gsrb lpl 0 per sol 1 lb 0"
REFINED_RB = "8 32 32 32 1 v gsrb lpl 0 sol sol 3 lb 0"
REFINED16 = "16 64 64 64 1 v gsrb lpl 0 sol sol 2 lb 0"   # level 2: the refined inner eighth
TREES = {"box16": BOX16, "refined": U.REFINED, "refined-gsrb": REFINED_RB, "box5": BOX5, "box6": BOX6}
SIZES = {"box16": {16, 8, 4, 2}, "refined": {8, 4, 2}, "refined-gsrb": {8, 4, 2}, "box5": {5}, "box6": {6, 3}}
SCALES = (1.0, -1.0, 0.37)
CENTRINGS = ("cell", "face")
NEG_ZERO = np.array([-0.0]).view(np.int64)[0]
MASKS = [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (True, True, False),
         (True, False, True), (False, True, True)]


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


def _launches(be, name):
    be.mg.ctx.call("synchronize")
    return be.mg.ctx.kernel_stats(name)[0]


def _ids(be, lvl):
    return [int(i) for i in be.tree.lvls[lvl].my_ids]


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.int64)


def _field(rng, n, m):
    """A random vector field [3, n, m, m, m] with a slab in which every
    component is constant: divergences that are exactly zero there (-0.0
    under a negative scale)."""
    v = rng.standard_normal((3, n, m, m, m))
    v[..., : m // 2] = 1.5
    return v


def read_mask(nc, width, centering):
    """[3, m, m, m]: the elements of a block the call may read, per component:
    the interior and, along the component's direction, the index 0 (both
    centrings) and nc+1 (cells); faces read 0 .. nc along it."""
    m, w = nc + 2 * width, width
    s = slice(w, w + nc)
    mask = np.zeros((3, m, m, m), dtype=bool)
    for d in range(3):
        at = [s, s, s]
        at[2 - d] = slice(w - 1, w + nc + 1) if centering == "cell" else slice(w - 1, w + nc)
        mask[(d,) + tuple(at)] = True
    return mask


def block_div(v, nc, width, dr, scale, centering, comps=(True, True, True)):
    """numpy's divergence [n, nc, nc, nc] of the field v [3, n, m, m, m] (or a
    list of three [n, m, m, m]) with `width` ghost layers: the terms
    (hi - lo) * f of the components in `comps`, added in the order x, y, z."""
    w = width
    s = slice(w, w + nc)
    total = None
    for d in range(3):
        if not comps[d]:
            continue
        ax = 3 - d   # (x is the last axis of [n, k, j, i])
        at, lo, hi = [slice(None), s, s, s], [slice(None), s, s, s], [slice(None), s, s, s]
        lo[ax] = slice(w - 1, w + nc - 1)
        if centering == "cell":
            hi[ax] = slice(w + 1, w + nc + 1)
            f = (0.5 * float(scale)) / float(dr[d])
        else:
            f = float(scale) / float(dr[d])
        t = (v[d][tuple(hi)] - v[d][tuple(lo)]) * f
        total = t if total is None else total + t
    return total


def _poison(v, nc, width, centering, comps):
    """NaN in every element outside the read set, and in a masked component's
    whole pool (a copy)."""
    v = np.array(v)
    mask = read_mask(nc, width, centering)
    for d in range(3):
        v[d][:, ~mask[d]] = np.nan
        if not comps[d]:
            v[d][:] = np.nan
    return v


def _seed(be, rng, ivs=(IPHI, IRHS, IOLD, IRES)):
    """Random bits in every stored cell of the variables `ivs` on every level;
    returns {(lvl, iv): the level as get_level returns it}."""
    out = {}
    for lvl in be.levels():
        n, nc = len(_ids(be, lvl)), be.tree.box_size_lvl[lvl]
        for iv in ivs:
            be.mg.set_level(lvl, iv, rng.standard_normal((n, nc + 2, nc + 2, nc + 2)))
    for lvl in be.levels():
        for iv in ivs:
            out[lvl, iv] = be.mg.get_level(lvl, iv)
    return out


def _expect(before, rows, want):
    """`before` [n, nc+2, ...] with the interiors of the boxes `rows` replaced by `want`."""
    exp = before.copy()
    inner = exp[:, 1:-1, 1:-1, 1:-1]
    inner[rows] = want
    return exp


def _same_level(be, lvl, iv, exp, msg=None):
    stored = U.stored_mask(be.tree.box_size_lvl[lvl])
    got = be.mg.get_level(lvl, iv)
    assert np.array_equal(_bits(got[:, stored]), _bits(exp[:, stored])), msg
    return got


def _cuda(v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


# -- 1. bitwise against numpy, both kernels, every level ------------------------------
@pytest.mark.parametrize("variant", ["tile", "generic"])
@pytest.mark.parametrize("name", sorted(TREES))
def test_every_level_bitwise_against_numpy(monkeypatch, name, variant):
    _switch(monkeypatch, variant)
    be = _backend(TREES[name])
    mg, tree = be.mg, be.tree
    rng = np.random.default_rng(20261021)
    assert {tree.box_size_lvl[lvl] for lvl in be.levels()} == SIZES[name]
    tiled = sum(tree.box_size_lvl[lvl] in (16, 8) for lvl in be.levels())
    state = _seed(be, rng, (IPHI, IRHS))
    calls, zeros, negs = 0, 0, 0
    for iv in (IRHS, IPHI):
        for lvl in be.levels():
            ids, nc = _ids(be, lvl), tree.box_size_lvl[lvl]
            v = _field(rng, len(ids), nc + 2)
            for scale in SCALES:
                for centering in CENTRINGS:
                    src = _cuda(_poison(v, nc, 1, centering, MASKS[0]))
                    n = mg.set_blocks_div(iv, src, ids, 1, scale=scale, centering=centering)
                    calls += 1
                    assert n == len(ids) * nc ** 3
                    want = block_div(v, nc, 1, tree.dr[lvl], scale, centering)
                    zeros += int((_bits(want) == 0).sum())
                    negs += int((_bits(want) == NEG_ZERO).sum())
                    state[lvl, iv] = _expect(state[lvl, iv], slice(None), want)
                    _same_level(be, lvl, iv, state[lvl, iv], (name, iv, lvl, scale, centering, variant))
    assert zeros > 0 and negs > 0   # (the sign of zero was compared)
    assert _launches(be, "boxes_div") == calls
    # the tile kernel served the 16^3 and 8^3 levels, and nothing under the switch
    want_tiles = 0 if variant == "generic" else tiled * 2 * len(SCALES) * len(CENTRINGS)
    assert _launches(be, "boxes_div_tile") == want_tiles


# -- the level shared by the tests 2, 3, 4 and 11 ---------------------------------------
@pytest.fixture(scope="module", params=[BOX16, U.NONCUBE], ids=["box16", "box8"])
def geo(request):
    """A tree whose every stored cell holds random bits: (backend, ids of
    level 1, {(lvl, iv): level}); the tests keep the dictionary current."""
    be = _backend(request.param)
    assert be.tree.box_size_lvl[1] in (16, 8)
    state = _seed(be, np.random.default_rng(100 + be.tree.box_size_lvl[1]))
    return be, _ids(be, 1), state


# -- 2. never read ------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["tile", "generic"])
@pytest.mark.parametrize("centering", CENTRINGS)
@pytest.mark.parametrize("width", [1, 2, 3])
def test_nothing_outside_the_named_elements_is_read(monkeypatch, geo, width, centering, variant):
    _switch(monkeypatch, variant)
    be, ids, state = geo
    nc = be.tree.box_size_lvl[1]
    rng = np.random.default_rng(7 * nc + width)
    v = _field(rng, len(ids), nc + 2 * width)
    for comps in MASKS:
        src = _poison(v, nc, width, centering, comps)
        assert np.isnan(src).any()
        if width > 1:   # (edges, corners and the outer layers are among them)
            assert np.isnan(src[:, :, 0]).all() and np.isnan(src[:, :, width - 1, width - 1, :]).all()
        n = be.mg.set_blocks_div(IRES, _cuda(src), ids, width, scale=-0.37, centering=centering, components=comps)
        assert n == len(ids) * nc ** 3
        want = block_div(v, nc, width, be.tree.dr[1], -0.37, centering, comps)
        assert not np.isnan(want).any()
        state[1, IRES] = _expect(state[1, IRES], slice(None), want)
        got = _same_level(be, 1, IRES, state[1, IRES], (width, centering, variant, comps))
        assert not np.isnan(got[:, 1:-1, 1:-1, 1:-1]).any()


# -- 3. never written ----------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["tile", "generic"])
@pytest.mark.parametrize("centering", CENTRINGS)
@pytest.mark.parametrize("iv", [IPHI, IRHS])
def test_ghosts_other_variables_and_unlisted_boxes_keep_their_bits(monkeypatch, geo, iv, centering, variant):
    _switch(monkeypatch, variant)
    be, ids, state = geo
    nc = be.tree.box_size_lvl[1]
    rng = np.random.default_rng([11, nc, iv, CENTRINGS.index(centering), len(variant)])
    rows = [int(q) for q in rng.permutation(len(ids))[: len(ids) // 2 + 1]]
    assert 0 < len(rows) < len(ids)
    v = _field(rng, len(rows), nc + 2)
    n = be.mg.set_blocks_div(iv, _cuda(v), [ids[q] for q in rows], 1, scale=1.0, centering=centering)
    assert n == len(rows) * nc ** 3
    want = block_div(v, nc, 1, be.tree.dr[1], 1.0, centering)
    inner = (slice(None),) + (slice(1, -1),) * 3
    assert not np.array_equal(_bits(state[1, iv][inner][rows]), _bits(want))   # (it does change the listed interiors)
    state[1, iv] = _expect(state[1, iv], rows, want)
    for (lvl, var), exp in state.items():   # every level, every variable, ghosts included
        _same_level(be, lvl, var, exp, ("changed", lvl, var))


# -- 4. block geometry ---------------------------------------------------------------------
def _plain(n, m):
    big = torch.zeros((3, n, m, m, m), dtype=torch.float64, device="cuda")
    return [big[d] for d in range(3)]


def _off8(n, m):
    """8 B off a 16-B boundary: views starting at an odd element."""
    big = torch.zeros((3 * n * m ** 3 + 1,), dtype=torch.float64, device="cuda")
    assert big.data_ptr() % 16 == 0
    parts = [big[1:].view(3, n, m, m, m)[d] for d in range(3)]
    assert parts[0].data_ptr() % 16 == 8
    return parts


def _odd_rows(n, m):
    """An odd row stride, from a padded view."""
    p = m + 1 + m % 2
    big = torch.zeros((3, n, m, m + 1, p), dtype=torch.float64, device="cuda")
    parts = [big[d][:, :, :m, :m] for d in range(3)]
    assert parts[0].stride(2) % 2 == 1
    return parts


def _pool(n, m):
    """Variables 1..3 of an AMR pool [box, variable, k, j, i]: pools that interleave."""
    big = torch.zeros((n, 5, m, m, m), dtype=torch.float64, device="cuda")
    parts = [big[:, 1 + d] for d in range(3)]
    assert parts[0].stride(0) == 5 * m ** 3
    return parts


def _separate(n, m):
    """Three allocations of their own."""
    return [torch.zeros((n, m, m, m), dtype=torch.float64, device="cuda") for _ in range(3)]


def _shared(n, m):
    """One pointer for the components x and y."""
    t = torch.zeros((2, n, m, m, m), dtype=torch.float64, device="cuda")
    return [t[0], t[0], t[1]]


LAYOUTS = {"plain": _plain, "off8": _off8, "odd-rows": _odd_rows, "pool": _pool, "separate": _separate,
           "shared": _shared}


@pytest.mark.parametrize("variant", [None, "tile", "generic"], ids=["routed", "tile", "generic"])
@pytest.mark.parametrize("width", [1, 2, 3])
def test_block_geometry(monkeypatch, geo, width, variant):
    _switch(monkeypatch, variant)
    be, all_ids, state = geo
    mg = be.mg
    mg.ctx.call("reset_stats")
    nc = be.tree.box_size_lvl[1]
    m = nc + 2 * width
    rng = np.random.default_rng(10 * nc + width)
    calls = 0
    for q, (name, layout) in enumerate(LAYOUTS.items()):
        for sub in (list(rng.permutation(all_ids)), list(rng.permutation(all_ids))[:len(all_ids) // 2 + 1]):
            sub = [int(i) for i in sub]
            rows = [all_ids.index(i) for i in sub]
            n = len(sub)
            for c, centering in enumerate(CENTRINGS):
                comps = MASKS[(q + n + width + c) % len(MASKS)] if name != "plain" else MASKS[0]
                v = _field(rng, n, m)
                if name == "shared":
                    v[1] = v[0]
                parts = layout(n, m)
                src = _poison(v, nc, width, centering, comps if name != "shared" else MASKS[0])
                if name == "shared":   # (one tensor: what either of the two components may read)
                    src[0] = np.where(np.isnan(src[0]), src[1], src[0])
                    src[1] = src[0]
                for d in (2, 1, 0):
                    parts[d].copy_(_cuda(src[d]))
                cells = mg.set_blocks_div(IRHS, parts, sub, width, scale=-1.0, centering=centering,
                                          components=comps)
                calls += 1
                assert cells == n * nc ** 3
                want = block_div(v, nc, width, be.tree.dr[1], -1.0, centering, comps)
                state[1, IRHS] = _expect(state[1, IRHS], rows, want)
                _same_level(be, 1, IRHS, state[1, IRHS], (name, n, centering, comps))
                for d in range(3):   # the pools are read-only
                    assert np.array_equal(_bits(parts[d]), _bits(src[d])), ("a pool was written", name, d)
    tile = variant == "tile"   # (routed: lists this short go to the per-cell kernel)
    assert (_launches(be, "boxes_div_tile") > 0) == tile
    assert _launches(be, "boxes_div") == calls


def test_a_width_of_zero_is_refused(geo):
    be, ids, _ = geo
    nc = be.tree.box_size_lvl[1]
    for centering in CENTRINGS:
        with pytest.raises(ValueError, match="ghost_width >= 1"):
            be.mg.set_blocks_div(IRHS, _plain(len(ids), nc), ids, 0, centering=centering)


# -- 5. a refined tree in one call --------------------------------------------------------
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
    assert len({float(tree.dr[l][0]) for l in lvls}) == 3
    state = _seed(be, rng, (IRHS,))
    for centering in CENTRINGS:
        v = _field(rng, len(leaves), 10)
        cells = mg.set_blocks_div(IRHS, _cuda(_poison(v, 8, 1, centering, MASKS[0])), leaves, 1, scale=-1.0,
                                  centering=centering)
        assert cells == len(leaves) * 512
        for l in lvls:   # (dr differs by level: f_d is per level)
            sel = [q for q, ll in enumerate(lvl_of) if ll == l]
            ids = _ids(be, l)
            rows = [ids.index(leaves[q]) for q in sel]
            want = block_div(v[:, sel], 8, 1, tree.dr[l], -1.0, centering)
            state[l, IRHS] = _expect(state[l, IRHS], rows, want)
        for l in be.levels():   # (the parents and the coarse levels keep their bits)
            _same_level(be, l, IRHS, state[l, IRHS], (centering, l))
    assert _launches(be, "boxes_div") == 2
    assert _launches(be, "boxes_div_tile") == (0 if variant == "generic" else 2 * 3)
    if variant == "tile":
        assert [_launches(be, f"boxes_div_tile@{l}") for l in lvls] == [2, 2, 2]


# -- 6. the path it replaces, on the state two stand-alone cycles leave ----------------------
def test_the_next_cycle_equals_the_one_after_set_blocks_of_the_numpy_divergence(monkeypatch):
    # (the 64 boxes of the 64^3 tree's level 1 and the 8 of level 0 take the multi-substep passes)
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", "8")
    monkeypatch.delenv("OMG_BLOCK3_COLUMN", raising=False)
    _switch(monkeypatch, "tile")
    pair = []
    for _ in range(2):
        be = DeviceBackend(parse(STREAM64))
        setup_problem(be)
        be.mg.ctx.call("set_profiling", 1)
        be.vcycle(False)
        be.vcycle(False)
        pair.append(be)
    a, b = pair   # a: the divergence entry; b: numpy and set_blocks
    tree, top = a.tree, a.tree.highest_lvl
    ids = _ids(a, top)
    assert len(ids) == 64
    # (the cycles ended in k_gsrb4's correction form: pending shifts, deferred ghosts, a pending res)
    assert _launches(a, f"smoother_gsrb4p@{top}") >= 2
    rng = np.random.default_rng(6)
    for centering in CENTRINGS:
        v = 1e-2 * _field(rng, len(ids), 18)
        assert a.mg.set_blocks_div(IRHS, _cuda(v), ids, 1, scale=1.0, centering=centering) == 64 * 4096
        want = block_div(v, 16, 1, tree.dr[top], 1.0, centering)
        assert b.mg.set_blocks(IRHS, _cuda(want), ids) == 64 * 4096
        ra, rb = a.vcycle(True), b.vcycle(True)
        assert float(ra).hex() == float(rb).hex(), centering
        assert phi_digest(a) == phi_digest(b), centering
    assert _launches(a, f"boxes_div_tile@{top}") == 2 and _launches(b, f"boxes_put_tile@{top}") == 2


# -- 7. div(grad) against the operator -----------------------------------------------------
@pytest.mark.parametrize("lvl", [1, 2], ids=["physical-faces", "refinement-faces"])
@pytest.mark.parametrize("args", [REFINED16, REFINED_RB], ids=["box16", "box8"])
def test_face_divergence_of_the_face_gradient_is_the_laplacian(monkeypatch, args, lvl):
    """|div(grad phi) - mg_apply_op| <= 64 eps M sum_d 1/dr_d^2 per box, M the
    largest |cc| of the box with its ghosts: a face difference (cc(+1) - cc)/dr
    carries one rounding of the subtraction and one of the product, relative to
    at most 2M/dr; the difference of two of them times 1/dr two more; the three
    sums two more: under 20 eps M sum 1/dr^2 on this side, and the operator's
    idr2 * (xm + xp - 2c) summed the same way stays under that too: 40 in all."""
    _switch(monkeypatch, "tile")
    be = _backend(args)
    mg, tree = be.mg, be.tree
    nc = tree.box_size_lvl[lvl]
    assert nc == parse(args)["box"]
    ids = _ids(be, lvl)
    phys = sum(int(tree.neighbors[i, nb] < 0) for i in ids for nb in range(6))
    # level 1 touches the domain boundary, level 2 lies inside with refinement-boundary ghosts all round
    assert len(tree.lvls[1].ref_bnds) and (phys > 0) == (lvl == 1)
    rng = np.random.default_rng(77)
    for l in be.levels():
        mg.set_level(l, IPHI, rng.standard_normal((len(_ids(be, l)), ) + (tree.box_size_lvl[l] + 2,) * 3))
    grad, n = mg.get_blocks_grad(ids, IPHI, ghost_width=1, scale=1.0, fill=True, centering="face")
    assert n == len(ids) * (nc + 1) * nc * nc
    assert mg.set_blocks_div(IRES, grad, ids, 1, scale=1.0, centering="face") == len(ids) * nc ** 3
    inner = (slice(None),) + (slice(1, -1),) * 3
    got = mg.get_level(lvl, IRES)[inner]
    cc = mg.get_level(lvl, IPHI)
    omg.mg_apply_op(mg, IRES)
    want = mg.get_level(lvl, IRES)[inner]
    stored = U.stored_mask(nc)
    M = np.abs(cc[:, stored]).max(axis=1)
    bound = 64 * np.finfo(np.float64).eps * M * float((1.0 / np.asarray(tree.dr[lvl], dtype=np.float64) ** 2).sum())
    err = np.abs(got - want).reshape(len(ids), -1).max(axis=1)
    print(f"div(grad) - op: max err / bound = {float((err / bound).max()):.3f}, physical faces {phys}")
    assert np.abs(want).max() > 0 and (err <= bound).all(), float((err / bound).max())


# -- 8. the record cache, host waits, launches per level ------------------------------------
def test_cached_lists_make_no_host_wait_and_a_fifth_replaces_the_oldest(monkeypatch):
    _switch(monkeypatch, "tile")
    be = _backend(BOX16, profile=False)
    mg, ctx, tree = be.mg, be.mg.ctx, be.tree
    ids = _ids(be, 1)
    assert len(ids) == 8
    rng = np.random.default_rng(23)
    state = _seed(be, rng, (IRHS,))
    v = _field(rng, 8, 18)
    pool = _cuda(v)
    lists = [ids, ids[::-1], ids[:5], ids[2:], ids[1:7]]
    ctx.call("synchronize")

    def put(q, centering="face"):
        rows = [ids.index(i) for i in lists[q]]
        src = pool[:, rows].contiguous()
        torch.cuda.synchronize()
        before = ctx.host_sync_count()
        cells = mg.set_blocks_div(IRHS, src, lists[q], 1, centering=centering)
        waits = ctx.host_sync_count() - before
        assert cells == len(rows) * 4096
        state[1, IRHS] = _expect(state[1, IRHS], rows, block_div(v[:, rows], 16, 1, tree.dr[1], 1.0, centering))
        return waits

    # (torch's allocator hands a freed block of one size out again: the bases stay 16-B aligned,
    # and the key holds the alignment, not the address)
    assert [put(0), put(0)] == [0, 0]                          # a repeated list
    assert [put(1), put(2), put(3), put(0)] == [0, 0, 0, 0]    # four lists, then the first again
    _same_level(be, 1, IRHS, state[1, IRHS])
    assert put(4) == 1                                         # a fifth waits once (it replaced list 1)
    _same_level(be, 1, IRHS, state[1, IRHS])
    assert [put(0), put(2), put(3), put(4)] == [0, 0, 0, 0]
    # the centring is part of the key (a fifth list again), and the key differs from the
    # gradient's and the copies' of the same list, strides and centring
    assert put(0, "cell") == 1
    _same_level(be, 1, IRHS, state[1, IRHS])
    out = torch.zeros((3, 8, 18, 18, 18), dtype=torch.float64, device="cuda")
    calls = (lambda: mg.get_blocks_grad(ids, IRHS, out=out, ghost_width=1, fill=False, centering="cell"),
             lambda: mg.set_blocks(IRHS, pool[0], ids, ghost_width=1),
             lambda: mg.set_blocks_div(IRHS, pool, ids, 1, centering="cell"))
    for call, waits in zip(calls, (1, 1, 0)):   # (two other keys, and this entry's own is still cached)
        torch.cuda.synchronize()
        before = ctx.host_sync_count()
        call()
        assert ctx.host_sync_count() - before == waits
    state[1, IRHS] = _expect(state[1, IRHS], slice(None), block_div(v, 16, 1, tree.dr[1], 1.0, "cell"))
    _same_level(be, 1, IRHS, state[1, IRHS])
    # one launch of the tile kernel per level listed: 16^3 boxes of level 1 and the 8^3 box of level -1
    ctx.call("set_profiling", 1)
    ctx.call("reset_stats")
    low = _ids(be, -1)
    assert len(low) == 1 and tree.box_size_lvl[-1] == 8
    mixed = ids[:3] + low
    w = _field(rng, 4, 18)
    src = _cuda(w)
    off = np.arange(4, dtype=np.int64) * 18 ** 3 + (1 + 18 + 324)
    cells = ctx.put_boxes_div(IRHS, mixed, [src[d].data_ptr() for d in range(3)], off, (1, 18, 324), 1.0, 1,
                              torch.cuda.current_stream().cuda_stream)
    assert cells == 3 * 4096 + 512
    assert [_launches(be, k) for k in ("boxes_div", "boxes_div_tile", "boxes_div_tile@1", "boxes_div_tile@-1")] \
        == [1, 2, 1, 1]
    _same_level(be, 1, IRHS, _expect(state[1, IRHS], [0, 1, 2], block_div(w[:, :3], 16, 1, tree.dr[1], 1.0, "face")))
    # (the 8^3 block in the corner of its 18^3 slot)
    _same_level(be, -1, IRHS, _expect(state[-1, IRHS], [0],
                                      block_div(w[:, 3:, :10, :10, :10], 8, 1, tree.dr[-1], 1.0, "face")))


# -- 9. stream ordering, no host wait ---------------------------------------------------------
def test_calls_are_ordered_on_the_callers_stream_without_a_host_wait(monkeypatch):
    _switch(monkeypatch, "tile")
    be = _backend(STREAM64, profile=False)
    mg, ctx, tree = be.mg, be.mg.ctx, be.tree
    ids = _ids(be, 1)
    v = _field(np.random.default_rng(9), len(ids), 18)
    first = _cuda(v)
    want = block_div(v, 16, 1, tree.dr[1], 1.0, "face")
    scratch = torch.zeros(32 * 1024 * 1024, dtype=torch.float64, device="cuda")   # 256 MB
    src = torch.zeros_like(first)
    out = torch.zeros((len(ids), 16, 16, 16), dtype=torch.float64, device="cuda")
    mg.set_blocks_div(IRES, src, ids, 1, centering="face")   # (the lists' records go up here)
    mg.get_blocks(IRES, ids, out=out, fill=False)
    side = torch.cuda.Stream()
    ctx.call("synchronize")
    torch.cuda.synchronize()
    syncs = ctx.host_sync_count()
    with torch.cuda.stream(side):
        for _ in range(200):   # (tens of milliseconds of queued passes)
            scratch.add_(1.0)
        src.copy_(first)                                           # the producer queued ahead of the call
        n = mg.set_blocks_div(IRES, src, ids, 1, centering="face")
        src.fill_(float("nan"))                                    # and a writer behind it
        mg.get_blocks(IRES, ids, out=out, fill=False)
        kept = out.clone()
        still_running = not side.query()
    assert ctx.host_sync_count() == syncs
    assert still_running, "the queued passes had finished: the calls were not made under load"
    assert n == len(ids) * 4096
    torch.cuda.synchronize()
    assert np.array_equal(_bits(kept), _bits(want))
    assert float(scratch[0]) == 200.0


# -- 10. several ranks ----------------------------------------------------------------------
def _by_id(id_, m=10):
    """The field of a box, the same on whichever rank owns it."""
    return _field(np.random.default_rng(1000 + int(id_)), 1, m)[:, 0]


def _leaf_run(be, rank, reduce):
    mg, tree = be.mg, be.tree
    lvls = [l for l in be.levels() if l >= 1]
    for l in be.levels():   # every box by its id (collective for phi, and on every rank for empty levels too)
        ids, nc = _ids(be, l), tree.box_size_lvl[l]
        data = np.stack([_by_id(i, nc + 2)[0] for i in ids]) if ids else np.zeros((0,) + (nc + 2,) * 3)
        mg.set_level(l, IPHI, data)
    omg.mg_fill_ghost_cells(mg, IPHI)   # (the ghosts stand: the put below must make them stale)
    leaves = [int(i) for l in lvls for i in tree.lvls[l].my_leaves]
    v = np.stack([_by_id(i) for i in leaves], axis=1) if leaves else np.zeros((3, 0, 10, 10, 10))
    src = _cuda(v)
    none = torch.zeros((3, 0, 10, 10, 10), dtype=torch.float64, device="cuda")
    # two collective calls: rank 0's leaves while the others list nothing, then the reverse
    n_put = mg.set_blocks_div(IPHI, src if rank == 0 else none, leaves if rank == 0 else [], 1, scale=0.37,
                              centering="face")
    n_put += mg.set_blocks_div(IPHI, none if rank == 0 else src, [] if rank == 0 else leaves, 1, scale=0.37,
                               centering="face")
    assert n_put == len(leaves) * 512
    if tree.n_cpu > 1:   # a box of another rank is an error, and the context goes on
        other = next(int(i) for l in lvls for i in tree.lvls[l].leaves if int(tree.rank[int(i)]) != rank)
        with pytest.raises(omg.device.OmgError, match="omg_put_boxes_div.*not owned"):
            mg.set_blocks_div(IRHS, src[:, :1], [other], 1)
    # (fill=True: collective; the ghosts come from the neighbours' new interiors, remote ones included)
    out, cells = mg.get_blocks(IPHI, leaves, ghost_width=1, ghosts=True, fill=True)
    assert cells == len(leaves) * (512 + 384)
    h = _bits(out) if leaves else np.zeros((0, 10, 10, 10), np.int64)
    lvl_of = {int(i): l for l in lvls for i in tree.lvls[l].my_leaves}
    inner = (slice(1, -1),) * 3
    for q, id_ in enumerate(leaves):   # the interiors against numpy, each level with its dr
        want = block_div(v[:, q:q + 1], 8, 1, tree.dr[lvl_of[id_]], 0.37, "face")[0]
        assert np.array_equal(h[q][inner], _bits(want)), id_
    return {id_: h[q] for q, id_ in enumerate(leaves)}


@pytest.fixture(scope="module")
def one_rank_leaves():
    return _leaf_run(_backend(U.REFINED, False), 0, None)


def test_two_ranks_give_the_one_rank_bits(monkeypatch, one_rank_leaves):
    _switch(monkeypatch, "tile")
    res = run_loopback(U.REFINED, 2, _leaf_run, timeout=120)
    assert all(len(r) for r in res)
    merged = {}
    for r in res:
        assert not set(r) & set(merged)
        merged.update(r)
    assert sorted(merged) == sorted(one_rank_leaves)
    stored = U.stored_mask(8)
    for id_, want in one_rank_leaves.items():
        assert np.array_equal(merged[id_][stored], want[stored]), id_


# -- 11. errors before any launch -------------------------------------------------------------
def test_bad_pointers_are_errors_before_any_launch_and_the_context_stays_usable(monkeypatch, geo):
    _switch(monkeypatch, "tile")
    be, ids, state = geo
    ctx = be.mg.ctx
    ctx.call("reset_stats")
    nc = be.tree.box_size_lvl[1]
    m, n = nc + 2, len(ids)
    stride = (1, m, m * m)
    off = np.arange(n, dtype=np.int64) * m ** 3 + (1 + m + m * m)
    v = _field(np.random.default_rng(41), n, m)
    good = _cuda(v)
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
             ("NULL pointers for all three components with n_boxes > 0", (0, 0, 0), off, 0),
             ("centering must be 0 (cells) or 1 (faces)", p, off, 2)]
    for what, ptrs, o, centering in cases:
        with pytest.raises(omg.device.OmgError) as ex:
            ctx.put_boxes_div(IRES, ids, ptrs, o, stride, -1.0, centering)
        assert str(ex.value) == "omg_put_boxes_div: " + what
        assert _launches(be, "boxes_div") == 0
    _same_level(be, 1, IRES, state[1, IRES], "an error changed the variable")
    # the context stays usable
    for centering in (0, 1):
        assert ctx.put_boxes_div(IRES, ids, p, off, stride, -1.0, centering) == n * nc ** 3
        state[1, IRES] = _expect(state[1, IRES], slice(None),
                                 block_div(v, nc, 1, be.tree.dr[1], -1.0, CENTRINGS[centering]))
        _same_level(be, 1, IRES, state[1, IRES])
