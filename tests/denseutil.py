"""Helpers shared by tests/test_dense_host.py and tests/test_gpu_dense.py: the
box table of a tree as numpy sees it, dense windows of a level's cell grid,
and their coverage counted without the library."""
import numpy as np

from tests.mgdriver import DeviceBackend, T, build_tree, omg, parse

# a NaN with a payload no computation produces: "never written"
SENTINEL = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.int64)[0]

UNIFORM = "8 32 32 32 1 v gsrb lpl 0 per sol 1 lb 0"
NONCUBE = "8 16 24 8 1 v gs lpl 0 d0 sol 1 lb 0"
REFINED = "8 32 32 32 1 v gs lpl 0 sol sol 3 lb 0"


def odd_box_tree(cfg, tree, n_ranks=1, my_rank=0):
    """The tree of a uniform configuration with an odd box size and 2 x 2 x 2
    boxes, which mg_build_rectangle refuses as the reference does ("box_size
    should be even") while the library's box layout pads odd boxes
    (omg_device.h).  The tree of 2^3 boxes with 2^3 cells each has the same
    boxes, neighbours and levels (eight boxes on level 1, one on level 0: a
    4^3 domain coarsens once, a 10^3 one too); it is built by the builder and
    its sizes are then set to the odd box's, as the builder would have."""
    box, dom = cfg["box"], np.array(cfg["domain"], dtype=np.int64)
    assert box % 2 == 1 and cfg["n_levels"] == 1 and np.all(dom == 2 * box) and cfg["smoother"] == "gsrb"
    tree.smoother_type = T.MG_SMOOTHER_GSRB
    tree.n_cpu, tree.my_rank = n_ranks, my_rank
    tree.build_rectangle(np.array([4, 4, 4]), 2, np.full(3, 0.25), [0.0] * 3, [cfg["bc"] == "per"] * 3, 0)
    assert (tree.lowest_lvl, tree.highest_lvl) == (0, 1)
    tree.box_size = box
    for lvl in list(tree.box_size_lvl):
        tree.box_size_lvl[lvl] = box
        tree.domain_size_lvl[lvl] = tree.domain_size_lvl[lvl] * box // 2
        tree.dr[lvl] = tree.dr[lvl] * 2.0 / box
    tree.box_dr[:] = tree.box_dr * 2.0 / box   # (box_r_min stands: the boxes are where they were)
    tree.load_balance()
    return tree


class OddBoxBackend(DeviceBackend):
    """mgdriver.DeviceBackend over odd_box_tree (constant boundary conditions)."""

    def _build(self, shift):
        cfg, mg = self.cfg, self.mg
        odd_box_tree(cfg, mg, mg.n_cpu, mg.my_rank)
        bc = {"d0": T.MG_BC_DIRICHLET, "n0": T.MG_BC_NEUMANN}[cfg["bc"]]
        for nb in range(1, 7):
            mg.bc[nb][T.MG_IPHI] = omg.BC(bc, 0.0)
        omg.mg_allocate_storage(mg)
        self.tree = mg
        self.rep_lvl = mg.ctx.replicated_level()


def host_tree(args, rank=0, world=1):
    return build_tree(parse(args), T.MGTree(), world, rank)


def plan_context(tree, rank=0, world=1, n_vars=5):
    """A plan-only context (OMG_DEVICE_NONE) of the tree: no GPU."""
    ctx = omg.device.Context(-2, rank, world)
    arrs = omg.mg._tree_arrays(tree)
    ctx.call("tree_setup", tree.n_boxes, *arrs[:6], tree.lowest_lvl, tree.highest_lvl,
             tree.first_normal_lvl, tree.box_size, arrs[6], arrs[7], arrs[8], arrs[9], n_vars)
    return ctx


def grid(tree, lvl):
    """(nx, ny, nz) of the level's cell grid."""
    return tuple(int(v) for v in tree.domain_size_lvl[lvl])


def contiguous(n):
    """Strides (x, y, z) in doubles of a contiguous window of extents n."""
    return (1, n[0], n[0] * n[1])


def box_origin(tree, lvl, id_):
    """0-based global cell index (x, y, z) of the box's local cell (1, 1, 1)."""
    return (np.asarray(tree.ix[id_], dtype=np.int64) - 1) * tree.box_size_lvl[lvl]


def count_cells(tree, lvl, lo, n, ids=None):
    """Cells of the level's boxes (ids: the ones counted, default all of them)
    inside the window: a numpy count over the box table."""
    ids = tree.lvls[lvl].ids if ids is None else ids
    if not len(ids):
        return 0
    nc = tree.box_size_lvl[lvl]
    g0 = (np.asarray(tree.ix)[np.asarray(ids, dtype=np.int64)] - 1) * nc
    lo, n = np.asarray(lo, dtype=np.int64), np.asarray(n, dtype=np.int64)
    cover = np.clip(np.minimum(g0 + nc, lo + n) - np.maximum(g0, lo), 0, None)
    return int(cover.prod(axis=1).sum())


def cut_windows(tree, lvl):
    """Three windows (lo, n) that cut through the level's boxes, the last one
    reaching outside the domain in x."""
    g = np.array(grid(tree, lvl), dtype=np.int64)
    return [((3 * g // 8 + 1).tolist(), (g // 2 + 1).tolist()),
            ([1, 0, int(g[2] // 3)], [int(g[0]) - 1, max(int(g[1]) // 2, 1), int(g[2]) - int(g[2] // 3)]),
            ([-3, 0, int(g[2]) // 2 - 2], [int(g[0]) + 5, int(g[1]), 5])]


def assemble(tree, lvl, ids, boxes, fill):
    """The dense array [nz, ny, nx] of the level's grid with the interiors of
    `boxes` [box, k, j, i] (reference layout, ids order) in place and `fill`
    (an int64 bit pattern) elsewhere; returned as int64 bits."""
    nx, ny, nz = grid(tree, lvl)
    nc = tree.box_size_lvl[lvl]
    out = np.full((nz, ny, nx), fill, dtype=np.int64)
    for q, id_ in enumerate(ids):
        x, y, z = box_origin(tree, lvl, id_)
        out[z:z + nc, y:y + nc, x:x + nc] = boxes[q, 1:nc + 1, 1:nc + 1, 1:nc + 1].view(np.int64)
    return out


def scatter(tree, lvl, ids, boxes, dense, lo=(0, 0, 0)):
    """`boxes` [box, k, j, i] with the interior cells inside the window `dense`
    [nz, ny, nx] at lo replaced by its values (a copy)."""
    out = boxes.copy()
    nc = tree.box_size_lvl[lvl]
    nz, ny, nx = dense.shape
    for q, id_ in enumerate(ids):
        o = box_origin(tree, lvl, id_)
        a = [max(int(o[d]), int(lo[d])) for d in range(3)]
        e = [min(int(o[d]) + nc, int(lo[d]) + (nx, ny, nz)[d]) for d in range(3)]
        if any(a[d] >= e[d] for d in range(3)):
            continue
        bx, by, bz = (slice(a[d] - int(o[d]) + 1, e[d] - int(o[d]) + 1) for d in range(3))
        wx, wy, wz = (slice(a[d] - int(lo[d]), e[d] - int(lo[d])) for d in range(3))
        out[q, bz, by, bx] = dense[wz, wy, wx]
    return out


def stored_mask(nc):
    """Interior and face ghosts of a (nc+2)^3 box: edges and corners are not stored."""
    ix = np.arange(nc + 2)
    bnd = ((ix == 0) | (ix == nc + 1)).astype(int)
    return (bnd[:, None, None] + bnd[None, :, None] + bnd[None, None, :]) < 2
