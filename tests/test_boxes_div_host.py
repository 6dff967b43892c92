"""omg_put_boxes_div on plan-only contexts (OMG_DEVICE_NONE): the count n_cells
of both centrings against a numpy count over the box table, the argument
checks (each followed by the same valid call), a box of another rank, a
replicated level, and the checks MG.set_blocks_div makes before the C call.
No GPU: a plan-only context validates, counts and launches nothing."""
import ctypes

import numpy as np
import pytest
import torch

from tests import denseutil as U
from tests.mgdriver import build_tree, omg, parse

CASES = [(args, world) for args in (U.UNIFORM, U.NONCUBE, U.REFINED) for world in (1, 2, 3)]
IDS = [f"{name}-{world}" for name in ("uniform", "noncube", "refined") for world in (1, 2, 3)]
# (non-NULL, 16-B aligned addresses: never dereferenced without a device)
PTRS = (4096, 4096 + (1 << 30), 4096 + (2 << 30))
CELL, FACE = 0, 1
WHO = "omg_put_boxes_div: "


def _contexts(args, world, rep_cells=0):
    out = []
    for r in range(world):
        tree = U.host_tree(args, r, world)
        if rep_cells:
            ctx = omg.device.Context(-2, r, world)
            ctx.call("set_coarse_replication", rep_cells)
            arrs = omg.mg._tree_arrays(tree)
            ctx.call("tree_setup", tree.n_boxes, *arrs[:6], tree.lowest_lvl, tree.highest_lvl,
                     tree.first_normal_lvl, tree.box_size, arrs[6], arrs[7], arrs[8], arrs[9], 5)
        else:
            ctx = U.plan_context(tree, r, world)
        out.append((tree, ctx))
    return out


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def ranks(request):
    out = _contexts(*request.param)
    yield out
    for _, ctx in out:
        ctx.close()


def _my_ids(tree):
    """Every box of the rank, all levels, in level order."""
    return [int(i) for lvl in range(tree.lowest_lvl, tree.highest_lvl + 1) for i in tree.lvls[lvl].my_ids]


def _layout(tree, ids, centering):
    """Blocks of the largest box size + 2 (cells) or + 1 (faces), one after
    the other, the interior one layer in: (box_off, stride)."""
    m = max(tree.box_size_lvl[int(tree.lvl[i])] for i in ids) + 2 - centering if len(ids) else 2
    off = np.arange(len(ids), dtype=np.int64) * m ** 3 + (1 + m + m * m)
    return off, (1, m, m * m)


def _want(tree, ids):
    nc = np.array([tree.box_size_lvl[int(tree.lvl[i])] for i in ids], dtype=np.int64)
    return int((nc ** 3).sum())


def _count(ctx, tree, ids, centering, iv=2, ptrs=PTRS):
    off, stride = _layout(tree, ids, centering)
    return ctx.put_boxes_div(iv, ids, ptrs, off, stride, -1.0, centering)


def test_the_symbol_and_the_binding_exist():
    assert "omg_put_boxes_div" in omg.device.SIGNATURES
    assert hasattr(ctypes.CDLL(omg.device.lib_path()), "omg_put_boxes_div")
    assert hasattr(omg.device.Context, "put_boxes_div")
    assert hasattr(omg.MG, "set_blocks_div")


def test_counts_match_the_box_table(ranks):
    seen = []
    for tree, ctx in ranks:
        ids = _my_ids(tree)
        seen += ids
        rng = np.random.default_rng(len(ids))
        perm = [ids[q] for q in rng.permutation(len(ids))]
        sub = perm[:max(len(perm) // 3, 1)]
        for centering in (CELL, FACE):
            for iv in (1, 2, 4):
                assert _count(ctx, tree, ids, centering, iv) == _want(tree, ids), (centering, iv)
            assert _count(ctx, tree, perm, centering) == _want(tree, ids)
            assert _count(ctx, tree, sub, centering) == _want(tree, sub) < _want(tree, ids)
            # (a skipped component does not change the count: cells written)
            assert _count(ctx, tree, ids, centering, ptrs=(0, PTRS[1], 0)) == _want(tree, ids)
            # (the pools are read-only: one pointer may serve two components)
            assert _count(ctx, tree, ids, centering, ptrs=(PTRS[0], PTRS[0], PTRS[0])) == _want(tree, ids)
    # the ranks' lists cover every box exactly once
    assert sorted(seen) == list(range(1, ranks[0][0].n_boxes + 1))
    for centering in (CELL, FACE):
        total = sum(_count(ctx, tree, _my_ids(tree), centering) for tree, ctx in ranks)
        assert total == _want(ranks[0][0], range(1, ranks[0][0].n_boxes + 1))


def test_an_empty_list_with_null_pointers_counts_zero(ranks):
    ctx = ranks[0][1]
    assert ctx.put_boxes_div(2, None, (0, 0, 0), None, (1, 2, 4), 1.0, CELL) == 0
    assert ctx.put_boxes_div(1, [], (0, 0, 0), [], (1, 2, 4), 1.0, FACE) == 0
    assert ctx.put_boxes_div(1, [], PTRS, [], (1, 2, 4), 1.0, FACE) == 0


def test_n_cells_may_be_null(ranks):
    tree, ctx = ranks[0]
    ids = np.array(_my_ids(tree)[:2], dtype=np.int32)
    off, stride = _layout(tree, ids, FACE)
    C = omg.device.C
    dev = (C.c_void_p * 3)(*PTRS)
    ctx.call("put_boxes_div", 2, len(ids), ids.ctypes.data_as(C.c_void_p), dev, off.ctypes.data_as(C.c_void_p),
             np.array(stride, dtype=np.int64), 1.0, FACE, None, None)


def _top_ids(tree):
    return [int(i) for i in tree.lvls[tree.highest_lvl].my_ids][:4]


# (every tree's finest boxes hold 8^3 cells: m = 10 for cells, 9 for faces)
# (the change, the message after "omg_put_boxes_div: "; {id}: the id put first in the list)
FACE_OK = dict(centering=1, stride=(1, 9, 81))
BAD = {
    "stride0": (dict(stride=(2, 10, 100)), "stride[0] must be 1"),
    "stride1": (dict(stride=(1, 9, 100)), "stride[1] < nc + 2"),
    "stride1-face": (dict(centering=1, stride=(1, 8, 81), good=FACE_OK), "stride[1] < nc + 1"),
    "stride2": (dict(stride=(1, 10, 99)), "stride[2] < stride[1]*(nc + 2)"),
    "stride2-face": (dict(centering=1, stride=(1, 9, 80), good=FACE_OK), "stride[2] < stride[1]*(nc + 1)"),
    "stride-range": (dict(stride=(1, 10, (1 << 40) + 1)), "stride out of range"),
    "centering2": (dict(centering=2), "centering must be 0 (cells) or 1 (faces)"),
    "centering-1": (dict(centering=-1), "centering must be 0 (cells) or 1 (faces)"),
    "iv0": (dict(iv=0), "bad variable index"),
    "iv_past": (dict(iv=6), "bad variable index"),           # (the contexts hold n_vars = 5)
    "id0": (dict(first=0), "box id {id} is out of range"),
    "id_past": (dict(first="past"), "box id {id} is out of range"),
    "twice": (dict(first="second"), "box id {id} is listed twice"),
    "off-range": (dict(off0=(1 << 40) + 1), "box_off out of range"),
    "null_ids": (dict(ids=None), "NULL ids or box_off with n_boxes > 0"),
    "null_off": (dict(off=None), "NULL ids or box_off with n_boxes > 0"),
    "null_array": (dict(ptrs=None), "the array of component pointers is required"),
    "all_null": (dict(ptrs=(0, 0, 0)), "NULL pointers for all three components with n_boxes > 0"),
    "negative": (dict(n=-1), "negative n_boxes"),
}


def _call(ctx, a):
    ids = None if a["ids"] is None else np.array(a["ids"], dtype=np.int32)
    off = None if a["off"] is None else np.array(a["off"], dtype=np.int64)
    C = omg.device.C
    cells = C.c_longlong(-1)
    dev = None if a["ptrs"] is None else (C.c_void_p * 3)(*[C.c_void_p(p or None) for p in a["ptrs"]])
    ctx.call("put_boxes_div", a["iv"], a["n"], None if ids is None else ids.ctypes.data_as(C.c_void_p), dev,
             None if off is None else off.ctypes.data_as(C.c_void_p),
             np.array(a["stride"], dtype=np.int64), 0.37, a["centering"], None, C.byref(cells))
    return cells.value


@pytest.mark.parametrize("bad", sorted(BAD))
def test_bad_arguments_are_errors(ranks, bad):
    tree, ctx = ranks[0]
    ids = _top_ids(tree)
    assert len(ids) >= 2 and tree.box_size_lvl[tree.highest_lvl] == 8
    b, text = dict(BAD[bad][0]), BAD[bad][1]
    good = dict(iv=2, n=len(ids), ids=ids, ptrs=PTRS, off=[q * 1000 + 111 for q in range(len(ids))],
                stride=(1, 10, 100), centering=0)
    good.update(b.pop("good", {}))
    want = len(ids) * 512
    assert _call(ctx, good) == want
    a = dict(good)
    first = b.pop("first", None)
    if first is not None:
        a["ids"] = [{"past": tree.n_boxes + 1, "second": ids[1]}.get(first, first)] + ids[1:]
    off0 = b.pop("off0", None)
    if off0 is not None:
        a["off"] = [off0] + a["off"][1:]
    a.update(b)
    with pytest.raises(omg.device.OmgError) as ex:
        _call(ctx, a)
    assert str(ex.value) == WHO + text.format(id=(a["ids"] or [0])[0])
    assert omg.device.lib().omg_last_error().decode() == str(ex.value)
    assert _call(ctx, good) == want   # (the context is as it was)


def test_equal_and_interleaved_pools_are_accepted(ranks):
    """The slices [:, d] of one pool [n, 3, m, m, m], and one pointer for all components."""
    tree, ctx = ranks[0]
    ids = _top_ids(tree)
    m = 10
    off = np.arange(len(ids), dtype=np.int64) * 3 * m ** 3 + (1 + m + m * m)
    ptrs = [PTRS[0] + 8 * d * m ** 3 for d in range(3)]
    for centering in (CELL, FACE):
        assert ctx.put_boxes_div(1, ids, ptrs, off, (1, m, m * m), 1.0, centering) == len(ids) * 512
        assert ctx.put_boxes_div(2, ids, (ptrs[0], ptrs[0], 0), off, (1, m, m * m), 1.0, centering) == len(ids) * 512


def test_a_box_of_another_rank_is_an_error():
    ranks = _contexts(U.REFINED, 2)
    try:
        (t0, c0), (t1, _) = ranks
        mine, theirs = _top_ids(t0), _top_ids(t1)
        assert mine and theirs and not set(mine) & set(theirs)
        for centering in (CELL, FACE):
            assert _count(c0, t0, mine, centering) == len(mine) * 512
            with pytest.raises(omg.device.OmgError, match="omg_put_boxes_div") as ex:
                _count(c0, t0, mine[:1] + theirs[:1], centering)
            assert "not owned" in str(ex.value)
            assert _count(c0, t0, mine, centering) == len(mine) * 512
    finally:
        for _, ctx in ranks:
            ctx.close()


def test_a_replicated_level_is_refused():
    ranks = _contexts(U.UNIFORM, 2, rep_cells=8 * 8 ** 3)
    try:
        (t0, c0), _ = ranks
        assert c0.replicated_level() == 0
        mine = [int(i) for i in t0.lvls[0].my_ids]
        top = _top_ids(t0)
        assert mine and top
        for centering in (CELL, FACE):
            assert _count(c0, t0, top, centering) == len(top) * 512
            for lst in (mine, top + mine[:1]):   # (its own boxes too: it is a put)
                with pytest.raises(omg.device.OmgError) as ex:
                    _count(c0, t0, lst, centering)
                assert str(ex.value) == WHO + "level 0 is replicated on every rank: use omg_upload_level"
            assert _count(c0, t0, top, centering) == len(top) * 512
    finally:
        for _, ctx in ranks:
            ctx.close()


def test_binding_checks_the_tensors_before_the_call():
    mg = build_tree(parse(U.REFINED), omg.MG())   # (never allocated: tensors let through raise RuntimeError)
    ids = [int(i) for i in mg.lvls[2].my_ids][:3]
    small = [int(i) for i in mg.lvls[-2].my_ids]
    assert mg.box_size_lvl[2] == 8 and mg.box_size_lvl[-2] == 4 and small
    f64 = torch.float64
    z = lambda *shape, **kw: torch.zeros(*shape, dtype=kw.get("dtype", f64))   # noqa: E731
    # (blocks, ids, ghost_width, centering, components)
    bad = {
        "wrong-m": (z(3, 3, 9, 9, 9), ids, 1, "cell", (True,) * 3),
        "not-cubic": (z(3, 3, 10, 10, 12), ids, 1, "cell", (True,) * 3),
        "dtype": (z(3, 3, 10, 10, 10, dtype=torch.float32), ids, 1, "cell", (True,) * 3),
        "cell-without-a-ghost-layer": (z(3, 3, 8, 8, 8), ids, 0, "cell", (True,) * 3),
        "face-without-a-ghost-layer": (z(3, 3, 8, 8, 8), ids, 0, "face", (True,) * 3),
        "centering": (z(3, 3, 10, 10, 10), ids, 1, "edge", (True,) * 3),
        "mixed-sizes": (z(3, 4, 10, 10, 10), ids + small[:1], 1, "cell", (True,) * 3),
        "len-ids": (z(3, 2, 10, 10, 10), ids, 1, "cell", (True,) * 3),
        "last-stride": (z(3, 3, 10, 10, 20)[..., ::2], ids, 1, "cell", (True,) * 3),
        "transposed": (z(3, 3, 10, 10, 10).transpose(2, 3), ids, 1, "cell", (True,) * 3),
        "rank": (z(3, 10, 10, 10), ids, 1, "cell", (True,) * 3),
        "two-components": (z(2, 3, 10, 10, 10), ids, 1, "cell", (True,) * 3),
        "numpy": (np.zeros((3, 3, 10, 10, 10)), ids, 1, "cell", (True,) * 3),
        "two-tensors": ([z(3, 10, 10, 10), z(3, 10, 10, 10)], ids, 1, "cell", (True,) * 3),
        "differing-shapes": ([z(3, 10, 10, 10), z(3, 12, 12, 12), None], ids, 1, "cell", (True,) * 3),
        "differing-strides": ([z(3, 10, 10, 10), z(3, 10, 10, 12)[..., :10], None], ids, 1, "face", (True,) * 3),
        "no-component": ([None, None, None], ids, 1, "cell", (True,) * 3),
        "masked-away": (z(3, 3, 10, 10, 10), ids, 1, "cell", (False,) * 3),
        "two-flags": (z(3, 3, 10, 10, 10), ids, 1, "cell", (True, True)),
        "cpu": (z(3, 3, 10, 10, 10), ids, 1, "cell", (True,) * 3),
        "cpu-face": (z(3, 3, 10, 10, 10), ids, 1, "face", (True, False, True)),
        "cpu-pool-slices": ([z(3, 3, 12, 12, 12)[:, d] for d in range(3)], ids, 2, "face", (True,) * 3),
        "cpu-one-tensor-twice": ([z(3, 12, 12, 12)] * 2 + [None], ids, 2, "cell", (True,) * 3),
    }
    for what, (blocks, lst, width, centering, comps) in bad.items():
        with pytest.raises(ValueError):
            mg.set_blocks_div(2, blocks, lst, width, centering=centering, components=comps)
    for what in ("cell-without-a-ghost-layer", "face-without-a-ghost-layer"):
        blocks, lst, width, centering, comps = bad[what]
        with pytest.raises(ValueError, match="ghost_width >= 1"):
            mg.set_blocks_div(2, blocks, lst, width, centering=centering, components=comps)
    # (the last four pass the layout checks and are refused for their device)
    for what in ("cpu", "cpu-face", "cpu-pool-slices", "cpu-one-tensor-twice"):
        blocks, lst, width, centering, comps = bad[what]
        with pytest.raises(ValueError, match="cpu"):
            mg.set_blocks_div(2, blocks, lst, width, centering=centering, components=comps)
