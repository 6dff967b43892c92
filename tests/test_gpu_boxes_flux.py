"""omg_get_boxes_flux on the GPU: omg_get_boxes_grad's values, each component
optionally weighted by a coefficient variable and optionally added to the
caller's pool.

The expected values never come from the code under test: they are numpy's, on
the (nc+2)^3 boxes that get_level returns after the ghost fill (phi) and on
the coefficient boxes as the test uploaded them (block_flux below):
    g = (hi - lo) * f,  f = (0.5 * scale) / dr at the cells, scale / dr at the faces,
    faces: v = (((2 * a_lo) * a_hi) / (a_lo + a_hi)) * g,  cells: v = a * g,
    no coefficient: v = g;  accumulate: pool + v.
Every comparison is on int64 bit views, the sign of zero included: no
operation here has a tolerance.  Pools start as denseutil.SENTINEL, or, for
accumulate, as random finite doubles (random sign and mantissa bits, exponents
within 2^-10 .. 2^10: a NaN's payload after an addition is not IEEE's to
define); every element outside the defined values must keep its bits.

 1. every level of six trees bitwise against numpy, both kernels (one of them
    not cubic: dr, and so the factor f, differs by direction);
 2. without coefficients the bits are get_blocks_grad's;
 3. mixed coefficients and component masks;
 4. block geometry, accumulating, under the routed, tile and per-cell kernel;
 5. the face divergence of the flux against mg_apply_op (variable coefficients);
 6. the leaves of a refined tree in one call, accumulating with scale -1;
 7. the lazy state two stand-alone cycles leave;
 8. the record cache (shared with get_blocks_grad) and its host waits;
 9. stream ordering under a loaded side stream, three accumulating calls;
10. two loopback ranks against one;
11. errors on a real context before any launch."""
import numpy as np
import pytest
import torch

from tests import denseutil as U
from tests.mgdriver import DeviceBackend, omg, parse, phi_digest, run_loopback, setup_problem

pytestmark = pytest.mark.gpu

IPHI, IRHS, IRES, IEPS = 1, 2, 4, 5
VL16 = "16 32 32 32 1 v gsrb vlpl 0 d0 sol 1 lb 0"     # boxes of 16, 8, 4, 2
VL8R = "8 32 32 32 4 v gs vlpl 0 sol sol 2 lb 0"       # refinement boundaries
AH8R = "8 32 32 32 2 v gs ahelm 5 sol sol 2 lb 0"      # three coefficients
BOX5 = "5 10 10 10 1 v gsrb lpl 0 d0 sol 1 lb 0"       # odd box size (denseutil.odd_box_tree)
BOX6 = "6 12 12 12 1 v gs lpl 0 d0 sol 1 lb 0"         # its coarsest level has one 3^3 box
STREAM64 = "16 64 64 64 1 v gsrb lpl 0 per sol 1 lb 0"
NONCUBE_VL = "8 16 24 8 1 v gs vlpl 0 d0 sol 1 lb 0"   # denseutil.NONCUBE with vlpl: dr differs by direction
# (tree, the coef argument, the coefficient variables it means, the box sizes of its levels)
TREES = {"vlpl16": (VL16, None, (5, 5, 5), {16, 8, 4, 2}), "vlpl8-refined": (VL8R, None, (5, 5, 5), {8, 4, 2}),
         "ahelm8-refined": (AH8R, None, (5, 6, 7), {8, 4, 2}), "box5": (BOX5, 5, (5, 5, 5), {5}),
         "box6": (BOX6, 5, (5, 5, 5), {6, 3}), "noncube-vlpl": (NONCUBE_VL, None, (5, 5, 5), {8, 4, 2})}
SCALES = (1.0, -1.0, 0.37)
CENTRINGS = ("cell", "face")
SENT = int(U.SENTINEL)
NEG_ZERO = np.array([-0.0]).view(np.int64)[0]
MASKS = [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (True, True, False),
         (True, False, True), (False, True, True)]


def _switch(monkeypatch, variant):
    """variant: None the library's routing, "tile" the tile kernel wherever it
    can serve, "generic" the per-cell kernel."""
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


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.int64)


def _cuda(bits):
    return torch.from_numpy(np.ascontiguousarray(bits)).cuda().view(torch.float64)


def _random_phi(rng, n, nc):
    """Random boxes, ghosts included, with a slab of one value: differences
    that are exactly zero (-0.0 under a negative scale)."""
    a = rng.standard_normal((n, nc + 2, nc + 2, nc + 2))
    a[:, :, :, : (nc + 2) // 2] = 1.5
    return a


def _random_coef(rng, n, nc):
    """Coefficients in [0.5, 2], ghosts included, with a slab of one value."""
    a = rng.uniform(0.5, 2.0, (n, nc + 2, nc + 2, nc + 2))
    a[:, : (nc + 2) // 2] = 1.25
    return a


def _random_bits(rng, shape):
    """int64 bits of finite doubles: random sign and mantissa, exponent 2^-10 .. 2^10."""
    b = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64)
    exp = np.uint64(1013) + ((b >> np.uint64(52)) & np.uint64(0x7FF)) % np.uint64(21)
    out = (b & np.uint64(1 << 63)) | (exp << np.uint64(52)) | (b & np.uint64((1 << 52) - 1))
    assert np.isfinite(out.view(np.float64)).all()
    return out.view(np.int64)


def _base(rng, shape, acc):
    return _random_bits(rng, shape) if acc else np.full(shape, U.SENTINEL, dtype=np.int64)


def block_flux(phi, coefs, dr, scale, centering):
    """(values, mask): float64 [3, n, nc+2, nc+2, nc+2], the flux of `phi`
    [n, k, j, i] (ghosts as they are) in the frame of the cells 0 .. nc+1, and
    mask [3, nc+2, nc+2, nc+2], the values that are defined (get_blocks_grad's
    elements).  coefs: per component a coefficient array shaped as phi, or None."""
    n, nc = phi.shape[0], phi.shape[1] - 2
    s, lo, hi, fa = slice(1, nc + 1), slice(0, nc), slice(2, nc + 2), slice(0, nc + 1)
    vals = np.zeros((3, n) + (nc + 2,) * 3)
    mask = np.zeros((3,) + (nc + 2,) * 3, dtype=bool)
    pick = lambda a, sl: a[(slice(None),) + tuple(sl)]   # noqa: E731
    for d in range(3):
        ax = 2 - d   # (x is the last axis of [k, j, i])
        at, up, dn = [s, s, s], [s, s, s], [s, s, s]
        if centering == "cell":
            up[ax], dn[ax] = hi, lo
            f = (0.5 * float(scale)) / float(dr[d])
        else:
            at[ax], up[ax], dn[ax] = fa, slice(1, nc + 2), fa
            f = float(scale) / float(dr[d])
        g = (pick(phi, up) - pick(phi, dn)) * f
        a = coefs[d]
        if a is None:
            v = g
        elif centering == "face":
            a_lo, a_hi = pick(a, dn), pick(a, up)
            v = (((2.0 * a_lo) * a_hi) / (a_lo + a_hi)) * g
        else:
            v = pick(a, at) * g
        vals[(d, slice(None)) + tuple(at)] = v
        mask[(d,) + tuple(at)] = True
    return vals, mask


def in_blocks(vals, mask, width, base, acc):
    """int64 bits [3, n, m, m, m] (m = nc + 2*width, width >= 1): `base` with
    the defined values placed (acc: added to what base holds, one addition)."""
    out = np.array(base)
    nc = vals.shape[2] - 2
    c = slice(width - 1, width + nc + 1)
    for d in range(3):
        win = out[d][:, c, c, c]
        new = (win.view(np.float64) + vals[d]) if acc else np.ascontiguousarray(vals[d])
        win[:, mask[d]] = new.view(np.int64)[:, mask[d]]
    return out


def _coefs_of(arrs, iv_coef):
    """The three coefficient arrays of iv_coef from {variable: array}."""
    return [arrs[v] if v else None for v in iv_coef]


def _upload_all(be, iv, boxes):
    for lvl in be.levels():
        be.mg.set_level(lvl, iv, boxes[lvl])


def _filled_phi(be, rng, iv=IPHI):
    """Random phi on every level, a fill, the download; then the random boxes
    go up again, so the ghosts on the device are stale.  Returns {lvl: filled}."""
    tree = be.tree
    up = {lvl: _random_phi(rng, len(tree.lvls[lvl].my_ids), tree.box_size_lvl[lvl]) for lvl in be.levels()}
    _upload_all(be, iv, up)
    omg.mg_fill_ghost_cells(be.mg, iv)
    filled = {lvl: be.mg.get_level(lvl, iv) for lvl in be.levels()}
    _upload_all(be, iv, up)
    stale = any(not np.array_equal(up[lvl][:, U.stored_mask(tree.box_size_lvl[lvl])],
                                   filled[lvl][:, U.stored_mask(tree.box_size_lvl[lvl])]) for lvl in be.levels())
    assert stale   # (the fill changed ghosts: `fill` matters)
    return filled


def _upload_coefs(be, rng, variables):
    """Random coefficients with ghosts on every level: {lvl: {variable: array}}."""
    tree = be.tree
    out = {}
    for lvl in be.levels():
        out[lvl] = {}
        for v in sorted(set(variables)):
            out[lvl][v] = _random_coef(rng, len(tree.lvls[lvl].my_ids), tree.box_size_lvl[lvl])
            be.mg.set_level(lvl, v, out[lvl][v])
    return out


# -- 1. bitwise against numpy, both kernels, every level ------------------------------
@pytest.mark.parametrize("variant", ["tile", "generic"])
@pytest.mark.parametrize("name", sorted(TREES))
def test_every_level_bitwise_against_numpy(monkeypatch, name, variant):
    _switch(monkeypatch, variant)
    args, coef, iv_coef, sizes = TREES[name]
    be = _backend(args)
    mg, tree = be.mg, be.tree
    rng = np.random.default_rng(20261021)
    assert {tree.box_size_lvl[lvl] for lvl in be.levels()} == sizes
    assert mg.flux_coefficients(coef) == iv_coef
    if "refined" in name:
        assert len(tree.lvls[1].ref_bnds)
    if name.startswith("noncube"):   # (the three factors f_d differ: a kernel that took one for all would fail)
        assert parse(args)["domain"] == parse(U.NONCUBE)["domain"]
        for lvl in be.levels():
            assert len({float(v) for v in tree.dr[lvl]}) == 3, (lvl, tree.dr[lvl])
    tiled = sum(tree.box_size_lvl[lvl] in (16, 8) for lvl in be.levels())
    filled = _filled_phi(be, rng)
    eps = _upload_coefs(be, rng, iv_coef)
    calls, zeros, neg_zeros, first = 0, 0, 0, True
    for lvl in be.levels():
        ids, nc = _ids(be, lvl), tree.box_size_lvl[lvl]
        shape = (3, len(ids)) + (nc + 2,) * 3
        for scale in SCALES:
            for centering in CENTRINGS:
                vals, mask = block_flux(filled[lvl], _coefs_of(eps[lvl], iv_coef), tree.dr[lvl], scale, centering)
                for d in range(3):
                    defined = np.ascontiguousarray(vals[d]).view(np.int64)[:, mask[d]]
                    zeros += int((defined == 0).sum())
                    neg_zeros += int((defined == NEG_ZERO).sum())
                for acc in (False, True):
                    base = _base(rng, shape, acc)
                    out = _cuda(base)
                    # (the first call fills the stale ghosts of every level)
                    res, n = mg.get_blocks_flux(ids, IPHI, coef=coef, out=out, ghost_width=1, scale=scale,
                                                fill=first, centering=centering, accumulate=acc)
                    first = False
                    calls += 1
                    assert res is out and n == len(ids) * int(mask[0].sum())
                    assert n == len(ids) * (nc + (centering == "face")) * nc * nc
                    want = in_blocks(vals, mask, 1, base, acc)
                    assert np.array_equal(_bits(out), want), (name, lvl, scale, centering, acc, variant)
    assert zeros > 0 and neg_zeros > 0   # (exact and negative zeros were compared)
    assert _launches(be, "boxes_flux") == calls
    # the tile kernel served the 16^3 and 8^3 levels, and nothing under the switch
    want_tiles = 0 if variant == "generic" else tiled * len(SCALES) * len(CENTRINGS) * 2
    assert _launches(be, "boxes_flux_tile") == want_tiles


# -- shared by 2, 3, 4, 11: level 1 of the 16-box and of an 8-box tree, only read --------
@pytest.fixture(scope="module", params=[VL16, AH8R], ids=["box16", "box8"])
def geo(request):
    """(backend, ids of level 1, filled phi, {variable: coefficient array})."""
    be = _backend(request.param)
    ids = _ids(be, 1)
    nc = be.tree.box_size_lvl[1]
    rng = np.random.default_rng(100 + nc)
    for lvl in be.levels():
        be.mg.set_level(lvl, IPHI, _random_phi(rng, len(_ids(be, lvl)), be.tree.box_size_lvl[lvl]))
    omg.mg_fill_ghost_cells(be.mg, IPHI)
    eps = _upload_coefs(be, rng, be.mg.flux_coefficients())
    return be, ids, be.mg.get_level(1, IPHI), eps[1]


# -- 2. no coefficient: the gradient's bits ---------------------------------------------
@pytest.mark.parametrize("variant", ["tile", "generic"])
@pytest.mark.parametrize("centering", CENTRINGS)
def test_without_coefficients_the_bits_are_the_gradients(monkeypatch, geo, centering, variant):
    _switch(monkeypatch, variant)
    be, ids, filled, _ = geo
    nc = be.tree.box_size_lvl[1]
    shape = (3, len(ids)) + (nc + 2,) * 3
    a, b = _cuda(_base(None, shape, False)), _cuda(_base(None, shape, False))
    _, na = be.mg.get_blocks_grad(ids, IPHI, out=a, ghost_width=1, scale=0.37, fill=False, centering=centering)
    _, nb = be.mg.get_blocks_flux(ids, IPHI, coef=(0, 0, 0), out=b, ghost_width=1, scale=0.37, fill=False,
                                  centering=centering)
    assert na == nb
    assert np.array_equal(_bits(a), _bits(b))
    vals, mask = block_flux(filled, [None] * 3, be.tree.dr[1], 0.37, centering)
    assert np.array_equal(_bits(b), in_blocks(vals, mask, 1, _base(None, shape, False), False))


# -- 3. mixed coefficients, component masks -----------------------------------------------
@pytest.mark.parametrize("variant", ["tile", "generic"])
@pytest.mark.parametrize("centering", CENTRINGS)
def test_mixed_coefficients_and_component_masks(monkeypatch, geo, centering, variant):
    _switch(monkeypatch, variant)
    be, ids, filled, eps = geo
    nc = be.tree.box_size_lvl[1]
    shape = (3, len(ids)) + (nc + 2,) * 3
    rng = np.random.default_rng(3)
    vals, mask = block_flux(filled, [eps[5], None, eps[5]], be.tree.dr[1], -1.0, centering)
    plain, _ = block_flux(filled, [None] * 3, be.tree.dr[1], -1.0, centering)
    assert np.array_equal(vals[1], plain[1]) and not np.array_equal(vals[0], plain[0])
    for q, comps in enumerate(MASKS):
        acc = bool(q % 2)
        base = _base(rng, shape, acc)
        out = _cuda(base)
        _, n = be.mg.get_blocks_flux(ids, IPHI, coef=(5, 0, 5), out=out, ghost_width=1, scale=-1.0, fill=False,
                                     centering=centering, accumulate=acc, components=comps)
        assert n == len(ids) * int(mask[0].sum())
        want = in_blocks(vals, mask, 1, base, acc)
        for d in range(3):
            if not comps[d]:
                want[d] = base[d]   # (a masked component keeps its bits)
        assert np.array_equal(_bits(out), want), (comps, acc)


# -- 4. block geometry, accumulating ------------------------------------------------------
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


@pytest.mark.parametrize("variant", [None, "tile", "generic"], ids=["routed", "tile", "generic"])
@pytest.mark.parametrize("centering", CENTRINGS)
@pytest.mark.parametrize("width", [1, 2, 3])
def test_block_geometry_accumulating(monkeypatch, geo, width, centering, variant):
    _switch(monkeypatch, variant)
    be, all_ids, filled, eps = geo
    mg = be.mg
    mg.ctx.call("reset_stats")
    nc = be.tree.box_size_lvl[1]
    m = nc + 2 * width
    rng = np.random.default_rng(10 * nc + width)
    iv_coef = mg.flux_coefficients()
    vals, mask = block_flux(filled, _coefs_of(eps, iv_coef), be.tree.dr[1], -1.0, centering)
    for q, (name, layout) in enumerate(LAYOUTS.items()):
        for sub in (list(rng.permutation(all_ids)), list(rng.permutation(all_ids))[:len(all_ids) // 2 + 1]):
            sub = [int(i) for i in sub]
            where = [all_ids.index(i) for i in sub]
            n = len(sub)
            comps = MASKS[(q + n + width) % len(MASKS)] if name != "plain" else MASKS[0]
            big, view = layout(n, m)
            parts = view(big)   # (int64 views: the pool's bits)
            if name == "off8":
                assert parts[0].data_ptr() % 16 == 8
            if name == "odd-rows":
                assert parts[0].stride(2) % 2 == 1
            if name == "pool":
                assert parts[0].stride(0) == 5 * m ** 3
            base = _random_bits(rng, (3, n, m, m, m))
            for d in range(3):
                if comps[d]:
                    parts[d].copy_(torch.from_numpy(base[d]).cuda())
            want = in_blocks(vals[:, where], mask, width, base, True)
            res, cells = mg.get_blocks_flux(sub, IPHI, out=[t.view(torch.float64) for t in parts], ghost_width=width,
                                            scale=-1.0, fill=False, centering=centering, accumulate=True,
                                            components=comps)
            assert cells == n * int(mask[0].sum())
            for d in range(3):
                if comps[d]:
                    assert np.array_equal(parts[d].cpu().numpy(), want[d]), (name, n, d)
                    parts[d].fill_(SENT)
            # the skipped components and everything around the blocks still hold the sentinel
            for t in (big if isinstance(big, list) else [big]):
                assert bool((t == SENT).all()), ("wrote outside the blocks or into a skipped component", name, n)
    tile = variant == "tile"   # (routed: the per-cell kernel)
    assert (_launches(be, "boxes_flux_tile") > 0) == tile
    assert _launches(be, "boxes_flux") == 2 * len(LAYOUTS)


def test_face_centring_needs_a_ghost_layer_and_accumulate_needs_out(geo):
    be, ids, _, _ = geo
    nc = be.tree.box_size_lvl[1]
    with pytest.raises(ValueError, match="ghost_width >= 1"):
        be.mg.get_blocks_flux(ids, out=_cuda(_base(None, (3, len(ids)) + (nc,) * 3, False)), centering="face")
    with pytest.raises(ValueError, match="accumulate"):
        be.mg.get_blocks_flux(ids, ghost_width=1, accumulate=True)
    # the default `out` is a tensor [3, n, m, m, m] of its own
    res, c = be.mg.get_blocks_flux(ids, ghost_width=1, fill=False)
    assert tuple(res.shape) == (3, len(ids)) + (nc + 2,) * 3 and c == len(ids) * (nc + 1) * nc * nc


# -- 5. operator consistency ----------------------------------------------------------------
@pytest.mark.parametrize("variant", ["tile", "generic"])
@pytest.mark.parametrize("args,lvl", [(VL16, 1), (AH8R, 1), (AH8R, 2), (NONCUBE_VL, 1)],
                         ids=["vlpl16", "ahelm8", "ahelm8-refined", "noncube-vlpl"])
def test_face_divergence_of_the_flux_is_the_operator(monkeypatch, args, lvl, variant):
    """Per cell |div F - (op + lambda phi)| <= 32 * 2^-53 * sum_q |T_q| with the
    six terms T_q = c_q (u_q - u_0) / dr^2 in numpy.  The factor is derived, not
    measured: each path makes at most ten roundings per term, summation
    included: 20, taken to the next power of two."""
    _switch(monkeypatch, variant)
    be = _backend(args)
    mg, tree = be.mg, be.tree
    nc = tree.box_size_lvl[lvl]
    ids = _ids(be, lvl)
    if args == NONCUBE_VL:   # (each direction has its own dr)
        assert len({float(v) for v in tree.dr[lvl]}) == 3, tree.dr[lvl]
    rng = np.random.default_rng(77)
    for l in be.levels():
        mg.set_level(l, IPHI, rng.standard_normal((len(_ids(be, l)),) + (tree.box_size_lvl[l] + 2,) * 3))
    iv_coef = mg.flux_coefficients()
    assert iv_coef == ((5, 6, 7) if "ahelm" in args else (5, 5, 5))
    eps = _upload_coefs(be, rng, iv_coef)
    F, n = mg.get_blocks_flux(ids, IPHI, ghost_width=1, scale=1.0, fill=True, centering="face")
    assert n == len(ids) * (nc + 1) * nc * nc
    assert mg.set_blocks_div(IRES, F, ids, 1, scale=1.0, centering="face") == len(ids) * nc ** 3
    inner = (slice(None),) + (slice(1, -1),) * 3
    got = mg.get_level(lvl, IRES)[inner]
    cc = mg.get_level(lvl, IPHI)
    omg.mg_apply_op(mg, IRES)
    lam = float(parse(args)["lam"])
    want = mg.get_level(lvl, IRES)[inner] + lam * cc[inner]
    s = slice(1, nc + 1)
    total = np.zeros_like(got)
    for d in range(3):
        a = eps[lvl][iv_coef[d]]
        for side in (slice(0, nc), slice(2, nc + 2)):
            nb = [s, s, s]
            nb[2 - d] = side
            nb = (slice(None),) + tuple(nb)
            c = 2.0 * a[inner] * a[nb] / (a[inner] + a[nb])
            total += np.abs(c * (cc[nb] - cc[inner]) / float(tree.dr[lvl][d]) ** 2)
    bound = 32 * 2.0 ** -53 * total
    ratio = float((np.abs(got - want) / bound).max())
    print(f"div(flux) - (op + lambda phi): max err / bound = {ratio:.3f}")
    assert np.abs(want).max() > 0 and (np.abs(got - want) <= bound).all(), ratio


# -- 6. a refined tree's leaves in one call ------------------------------------------------
@pytest.mark.parametrize("variant", ["tile", "generic"])
def test_leaves_of_a_refined_tree_in_one_call_accumulating(monkeypatch, variant):
    _switch(monkeypatch, variant)
    be = _backend(VL8R)
    mg, tree = be.mg, be.tree
    rng = np.random.default_rng(31)
    lvls = [l for l in be.levels() if l >= 1]
    assert lvls == [1, 2] and all(len(tree.lvls[l].my_leaves) for l in lvls) and len(tree.lvls[1].my_parents)
    leaves = [int(i) for l in lvls for i in tree.lvls[l].my_leaves]
    lvl_of = [l for l in lvls for _ in tree.lvls[l].my_leaves]
    assert tree.dr[1][0] != tree.dr[2][0]   # (f_d is per level)
    filled = _filled_phi(be, rng)
    eps = _upload_coefs(be, rng, (5,))
    for centering in CENTRINGS:
        base = _random_bits(rng, (3, len(leaves), 10, 10, 10))
        b = _cuda(base)
        _, cells = mg.get_blocks_flux(leaves, IPHI, out=b, ghost_width=1, scale=-1.0, fill=centering == "cell",
                                      centering=centering, accumulate=True)
        assert cells == len(leaves) * (512 if centering == "cell" else 576)
        want = np.array(base)
        for l in lvls:
            ids = _ids(be, l)
            sel = [q for q, ll in enumerate(lvl_of) if ll == l]
            rows = [ids.index(leaves[q]) for q in sel]
            vals, mask = block_flux(filled[l][rows], [eps[l][5][rows]] * 3, tree.dr[l], -1.0, centering)
            want[:, sel] = in_blocks(vals, mask, 1, base[:, sel], True)
        assert np.array_equal(_bits(b), want), centering
    assert _launches(be, "boxes_flux") == 2
    assert _launches(be, "boxes_flux_tile") == (0 if variant == "generic" else 2 * 2)
    if variant == "tile":
        assert [_launches(be, f"boxes_flux_tile@{l}") for l in lvls] == [2, 2]


# -- 7. the lazy state two stand-alone cycles leave ------------------------------------------
def test_pending_state_is_resolved_and_the_next_cycle_is_unchanged(monkeypatch):
    # (the 64 boxes of the 64^3 tree's level 1 and the 8 of level 0 take the multi-substep passes)
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", "8")
    monkeypatch.delenv("OMG_BLOCK3_COLUMN", raising=False)
    _switch(monkeypatch, "tile")
    trio = []
    eps = _random_coef(np.random.default_rng(7), 64, 16)
    for _ in range(3):
        be = DeviceBackend(parse(STREAM64))
        setup_problem(be)
        # (variable 5, the Laplacian tree's spare, holds the coefficient, ghosts included, before the cycles)
        be.mg.set_level(be.tree.highest_lvl, 5, eps)
        be.mg.ctx.call("set_profiling", 1)
        be.vcycle(False)
        be.vcycle(False)
        trio.append(be)
    a, b, c = trio   # a: the flux calls; b: the reference download; c: cycles alone
    tree, top = a.tree, a.tree.highest_lvl
    ids = _ids(a, top)
    assert len(ids) == 64
    # (the cycles ended in k_gsrb4's correction form, the one that defers the ghosts)
    assert _launches(a, f"smoother_gsrb4p@{top}") >= 2
    shape = (3, len(ids), 18, 18, 18)
    got = {}
    for centering in CENTRINGS:
        out = _cuda(_base(None, shape, False))
        _, cells = a.mg.get_blocks_flux(ids, IPHI, coef=5, out=out, ghost_width=1, scale=-1.0, fill=True,
                                        centering=centering)
        assert cells == len(ids) * (16 + (centering == "face")) * 256
        got[centering] = _bits(out)
    assert _launches(a, f"boxes_flux_tile@{top}") == 2
    omg.mg_fill_ghost_cells_lvl(b.mg, top, IPHI)
    phi = b.mg.get_level(top, IPHI)
    assert np.abs(phi[:, 1:-1, 1:-1, 1:-1]).max() > 0
    for centering in CENTRINGS:
        vals, mask = block_flux(phi, [eps] * 3, tree.dr[top], -1.0, centering)
        assert np.array_equal(got[centering], in_blocks(vals, mask, 1, _base(None, shape, False), False)), centering
    ha, hc = a.vcycle(True), c.vcycle(True)
    assert float(ha).hex() == float(hc).hex()
    assert phi_digest(a) == phi_digest(c)


# -- 8. the record cache and its host waits -------------------------------------------------
def test_cached_lists_make_no_host_wait_whatever_the_launch_arguments(monkeypatch, geo):
    _switch(monkeypatch, "tile")
    be, ids, filled, eps = geo
    mg, ctx = be.mg, be.mg.ctx
    nc = be.tree.box_size_lvl[1]
    shape = (3, len(ids)) + (nc + 2,) * 3
    rng = np.random.default_rng(8)
    full = mg.flux_coefficients()
    lists = {"flux-first": ids[::-1], "grad-first": ids[1:] + ids[:1]}
    ctx.call("synchronize")

    def flux(lst, coef, acc, scale):
        base = _base(rng, shape, acc)
        out = _cuda(base)
        torch.cuda.synchronize()
        before = ctx.host_sync_count()
        mg.get_blocks_flux(lst, IPHI, coef=coef, out=out, ghost_width=1, scale=scale, fill=False, centering="face",
                           accumulate=acc)
        waits = ctx.host_sync_count() - before
        where = [ids.index(i) for i in lst]
        iv_coef = mg.flux_coefficients(coef)
        vals, mask = block_flux(filled[where], [None if not v else eps[v][where] for v in iv_coef], be.tree.dr[1],
                                scale, "face")
        assert np.array_equal(_bits(out), in_blocks(vals, mask, 1, base, acc)), (coef, acc, scale)
        return waits

    # four other lists push everything older out of the cache, so the next two are built here
    for k in range(4):
        mg.get_blocks(IRHS, ids[k:k + 2], ghost_width=1, ghosts=True, fill=False)
    flux(lists["flux-first"], None, False, 1.0)
    assert flux(lists["flux-first"], None, False, 1.0) == 0            # a repeated list
    g = _cuda(_base(None, shape, False))
    mg.get_blocks_grad(lists["grad-first"], IPHI, out=g, ghost_width=1, fill=False, centering="face")
    assert flux(lists["grad-first"], None, False, 1.0) == 0            # a list the gradient cached
    # iv_coef, accumulate and scale are launch arguments, not part of the key
    assert [flux(lists["grad-first"], (0, 0, 0), False, 1.0), flux(lists["grad-first"], full, True, 1.0),
            flux(lists["grad-first"], (full[0], 0, 0), True, -0.37), flux(lists["flux-first"], 0, True, 2.0)] == [0] * 4
    # and the gradient is served by the list the flux entry cached
    torch.cuda.synchronize()
    before = ctx.host_sync_count()
    mg.get_blocks_grad(lists["flux-first"], IPHI, out=g, ghost_width=1, fill=False, centering="face")
    assert ctx.host_sync_count() == before


# -- 9. stream ordering under a loaded side stream -------------------------------------------
def test_three_queued_accumulating_calls_add_three_times_without_a_host_wait(monkeypatch):
    _switch(monkeypatch, "tile")
    be = _backend(STREAM64, profile=False)
    mg, ctx, tree = be.mg, be.mg.ctx, be.tree
    ids = _ids(be, 1)
    rng = np.random.default_rng(9)
    mg.set_level(1, IPHI, _random_phi(rng, len(ids), 16))
    omg.mg_fill_ghost_cells_lvl(mg, 1, IPHI)
    eps = _random_coef(rng, len(ids), 16)
    mg.set_level(1, 5, eps)
    vals, mask = block_flux(mg.get_level(1, IPHI), [eps] * 3, tree.dr[1], 1.0, "face")
    shape = (3, len(ids), 18, 18, 18)
    base = _random_bits(rng, shape)
    want = base
    for _ in range(3):
        want = in_blocks(vals, mask, 1, want, True)
    scratch = torch.zeros(32 * 1024 * 1024, dtype=torch.float64, device="cuda")   # 256 MB
    out = _cuda(base)
    warm = _cuda(base)
    mg.get_blocks_flux(ids, coef=5, out=warm, ghost_width=1, accumulate=True)   # (the list's records go up here)
    side = torch.cuda.Stream()
    ctx.call("synchronize")
    torch.cuda.synchronize()
    syncs = ctx.host_sync_count()
    with torch.cuda.stream(side):
        for _ in range(200):   # (tens of milliseconds of queued passes)
            scratch.add_(1.0)
        out.mul_(1.0)          # a writer of the pool queued ahead of the calls
        for _ in range(3):
            _, n = mg.get_blocks_flux(ids, coef=5, out=out, ghost_width=1, accumulate=True)
            assert n == len(ids) * 17 * 256
        kept = out.clone()     # the consumer queued behind them
        still_running = not side.query()
    assert ctx.host_sync_count() == syncs
    assert still_running, "the queued passes had finished: the calls were not made under load"
    torch.cuda.synchronize()
    assert np.array_equal(_bits(kept), want) and np.array_equal(_bits(out), want)
    assert np.array_equal(_bits(warm), in_blocks(vals, mask, 1, base, True))
    assert float(scratch[0]) == 200.0


# -- 10. two loopback ranks ------------------------------------------------------------------
def _by_id(id_, nc=8):
    """The data of a box (phi, coefficient), the same on whichever rank owns it."""
    rng = np.random.default_rng(1000 + int(id_))
    return _random_phi(rng, 1, nc)[0], _random_coef(rng, 1, nc)[0]


def _leaf_run(be, rank, reduce):
    mg, tree = be.mg, be.tree
    lvls = [l for l in be.levels() if l >= 1]
    for l in be.levels():   # every box by its id (collective for phi, and on every rank for empty levels too)
        ids, nc = _ids(be, l), tree.box_size_lvl[l]
        empty = np.zeros((0,) + (nc + 2,) * 3)
        mg.set_level(l, IPHI, np.stack([_by_id(i, nc)[0] for i in ids]) if ids else empty)
        if ids:
            mg.set_level(l, IEPS, np.stack([_by_id(i, nc)[1] for i in ids]))
    leaves = [int(i) for l in lvls for i in tree.lvls[l].my_leaves]
    if tree.n_cpu > 1:   # a box of another rank is an error, and the context goes on
        other = next(int(i) for l in lvls for i in tree.lvls[l].leaves if int(tree.rank[int(i)]) != rank)
        with pytest.raises(omg.device.OmgError, match="omg_get_boxes_flux.*not owned"):
            mg.get_blocks_flux([other], ghost_width=1, fill=False)
    res = {}
    for centering in CENTRINGS:   # (fill=True: collective, across rank and refinement boundaries)
        out = _cuda(_base(None, (3, len(leaves), 10, 10, 10), False))
        _, cells = mg.get_blocks_flux(leaves, IPHI, out=out, ghost_width=1, scale=-1.0, fill=True,
                                      centering=centering)
        assert cells == len(leaves) * (512 if centering == "cell" else 576)
        h = _bits(out) if leaves else np.zeros((3, 0, 10, 10, 10), np.int64)
        res[centering] = {id_: h[:, q] for q, id_ in enumerate(leaves)}
    remote = int(sum(tree.rank[tree.neighbors[i, nb]] != rank for i in leaves for nb in range(6)
                     if tree.neighbors[i, nb] > 0))
    return res, remote


@pytest.fixture(scope="module")
def one_rank_leaves():
    """The leaves' fluxes of the refined vlpl tree on one rank, checked against numpy."""
    be = _backend(VL8R, False)
    res, _ = _leaf_run(be, 0, None)
    tree = be.tree
    for l in (1, 2):
        ids, phi = _ids(be, l), be.mg.get_level(l, IPHI)
        leaves = [int(i) for i in tree.lvls[l].my_leaves]
        sel = [ids.index(i) for i in leaves]
        eps = np.stack([_by_id(i)[1] for i in leaves])
        for centering in CENTRINGS:
            vals, mask = block_flux(phi[sel], [eps] * 3, tree.dr[l], -1.0, centering)
            want = in_blocks(vals, mask, 1, _base(None, (3, len(leaves), 10, 10, 10), False), False)
            for q, id_ in enumerate(leaves):
                assert np.array_equal(res[centering][id_], want[:, q]), (l, id_, centering)
    return res


def test_two_ranks_give_the_one_rank_bits(monkeypatch, one_rank_leaves):
    _switch(monkeypatch, "tile")
    out = run_loopback(VL8R, 2, _leaf_run, timeout=120)
    assert all(r[1] > 0 for r in out)   # (both ranks have leaf faces whose neighbour is remote)
    for centering in CENTRINGS:
        merged = {}
        for r, _ in out:
            assert r[centering] and not set(r[centering]) & set(merged)
            merged.update(r[centering])
        assert sorted(merged) == sorted(one_rank_leaves[centering])
        for id_, want in one_rank_leaves[centering].items():
            assert np.array_equal(merged[id_], want), (centering, id_)


# -- 11. errors before any launch -------------------------------------------------------------
def test_bad_pointers_and_a_bad_iv_coef_are_errors_before_any_launch(monkeypatch, geo):
    _switch(monkeypatch, "tile")
    be, ids, filled, eps = geo
    ctx = be.mg.ctx
    ctx.call("reset_stats")
    nc = be.tree.box_size_lvl[1]
    n_vars = be.mg.n_vars
    m, n = nc + 2, len(ids)
    stride = (1, m, m * m)
    off = np.arange(n, dtype=np.int64) * m ** 3 + (1 + m + m * m)
    base = _random_bits(np.random.default_rng(11), (3, n, m, m, m))
    good = _cuda(base)
    host = np.zeros(n * m ** 3)
    p = [good[d].data_ptr() for d in range(3)]
    far = off.copy()
    far[-1] += 1 << 34    # (a block 128 GiB up: past the end of any allocation)
    low = off.copy()
    low[0] -= 1 << 34
    past = "a block reaches past the end of the pointer's allocation"
    before = "a block starts before the pointer's allocation"
    ok = (5, 5, 5)
    cases = [("the pointer is not device memory", ok, (host.ctypes.data, 0, 0), off, 0),
             ("the pointer is not device memory", ok, (p[0], p[1], host.ctypes.data), off, 1),
             (past, ok, (0, p[1], 0), far, 0),
             (past, None, (p[0], p[1], p[2]), far, 1),
             (before, ok, (p[0], 0, 0), low, 0),
             (before, ok, (0, 0, p[2]), low, 1),
             ("components 0 and 1 share one pointer", ok, (p[0], p[0], 0), off, 0),
             ("components 1 and 2 share one pointer", ok, (p[2], p[1], p[1]), off, 1),
             (f"iv_coef[1] = {n_vars + 1} is not 0 or a variable 1..{n_vars}", (5, n_vars + 1, 5), p, off, 1),
             ("iv_coef[2] = -3 is not 0 or a variable 1..%d" % n_vars, (5, 5, -3), p, off, 0),
             ("iv_coef[0] is iv itself", (IPHI, 5, 5), p, off, 1)]
    for acc in (False, True):
        for what, coef, ptrs, o, centering in cases:
            with pytest.raises(omg.device.OmgError) as ex:
                ctx.get_boxes_flux(IPHI, coef, ids, ptrs, o, stride, -1.0, centering, acc, False)
            assert str(ex.value) == "omg_get_boxes_flux: " + what
            assert _launches(be, "boxes_flux") == 0
            assert np.array_equal(_bits(good), base)
    # the context stays usable
    iv_coef = be.mg.flux_coefficients()
    for centering in (0, 1):
        ok_pool = _cuda(base)
        cells = ctx.get_boxes_flux(IPHI, iv_coef, ids, [ok_pool[d].data_ptr() for d in range(3)], off, stride, -1.0,
                                   centering, True, False)
        assert cells == n * (nc + centering) * nc * nc
        vals, mask = block_flux(filled, _coefs_of(eps, iv_coef), be.tree.dr[1], -1.0, CENTRINGS[centering])
        assert np.array_equal(_bits(ok_pool), in_blocks(vals, mask, 1, base, True))
