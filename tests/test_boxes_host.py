"""omg_put_boxes / omg_get_boxes on plan-only contexts (OMG_DEVICE_NONE): the
count n_cells against a numpy count over the box table, the argument checks,
and the checks MG.set_blocks / MG.get_blocks make before the C call.
No GPU: a plan-only context validates, counts and copies nothing."""
import numpy as np
import pytest
import torch

from tests import denseutil as U
from tests.mgdriver import build_tree, omg, parse

CASES = [(args, world) for args in (U.UNIFORM, U.NONCUBE, U.REFINED) for world in (1, 2, 3)]
IDS = [f"{name}-{world}" for name in ("uniform", "noncube", "refined") for world in (1, 2, 3)]
PTR = 4096   # (a non-NULL, 16-B aligned address: never dereferenced without a device)


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


def _layout(tree, ids, ghost):
    """Blocks of the largest box size, one after the other: (box_off, stride)."""
    m = max(tree.box_size_lvl[int(tree.lvl[i])] for i in ids) + 2 * ghost if len(ids) else 2
    off = np.arange(len(ids), dtype=np.int64) * m ** 3 + ghost * (1 + m + m * m)
    return off, (1, m, m * m)


def _want(tree, ids, ghost):
    nc = np.array([tree.box_size_lvl[int(tree.lvl[i])] for i in ids], dtype=np.int64)
    return int((nc ** 3 + ghost * 6 * nc ** 2).sum())


def _count(ctx, tree, ids, ghost, get, iv=2):
    off, stride = _layout(tree, ids, ghost)
    if get:
        return ctx.get_boxes(iv, ids, PTR, off, stride, ghost, False)
    return ctx.put_boxes(iv, ids, PTR, off, stride, ghost)


def test_counts_match_the_box_table(ranks):
    seen = []
    for tree, ctx in ranks:
        ids = _my_ids(tree)
        seen += ids
        rng = np.random.default_rng(len(ids))
        perm = [ids[q] for q in rng.permutation(len(ids))]
        sub = perm[:max(len(perm) // 3, 1)]
        for ghost in (0, 1):
            for get in (False, True):
                assert _count(ctx, tree, ids, ghost, get) == _want(tree, ids, ghost), (ghost, get)
                assert _count(ctx, tree, perm, ghost, get) == _want(tree, ids, ghost)
                assert _count(ctx, tree, sub, ghost, get) == _want(tree, sub, ghost) < _want(tree, ids, ghost)
    # the ranks' lists cover every box exactly once
    assert sorted(seen) == list(range(1, ranks[0][0].n_boxes + 1))
    total = sum(_count(ctx, tree, _my_ids(tree), 1, True) for tree, ctx in ranks)
    assert total == _want(ranks[0][0], range(1, ranks[0][0].n_boxes + 1), 1)


def test_an_empty_list_with_null_pointers_counts_zero(ranks):
    ctx = ranks[0][1]
    assert ctx.put_boxes(2, None, 0, None, (1, 2, 4), 0) == 0
    assert ctx.get_boxes(2, None, 0, None, (1, 2, 4), 1, True) == 0
    assert ctx.put_boxes(1, [], 0, [], (1, 2, 4), 1) == 0


def test_n_cells_may_be_null(ranks):
    tree, ctx = ranks[0]
    ids = np.array(_my_ids(tree)[:2], dtype=np.int32)
    off, stride = _layout(tree, ids, 0)
    C = omg.device.C
    ctx.call("put_boxes", 2, len(ids), ids.ctypes.data_as(C.c_void_p), C.c_void_p(PTR),
             off.ctypes.data_as(C.c_void_p), np.array(stride, dtype=np.int64), 0, None, None)


def _top_ids(tree):
    return [int(i) for i in tree.lvls[tree.highest_lvl].my_ids][:4]


# (every tree's finest boxes hold 8^3 cells: m = 8 + 2*ghost)
# (the change, the message after "omg_put_boxes: " / "omg_get_boxes: "; {id}: the id put first in the list)
BAD = {
    "stride0": (dict(stride=(2, 8, 64)), "stride[0] must be 1"),
    "stride1": (dict(stride=(1, 7, 64)), "stride[1] < nc + 2*ghost"),
    "stride1-ghost": (dict(ghost=1, stride=(1, 9, 100), good=dict(ghost=1, stride=(1, 10, 100))),
                      "stride[1] < nc + 2*ghost"),
    "stride2": (dict(stride=(1, 8, 63)), "stride[2] < stride[1]*(nc + 2*ghost)"),
    "stride2-ghost": (dict(ghost=1, stride=(1, 10, 99), good=dict(ghost=1, stride=(1, 10, 100))),
                      "stride[2] < stride[1]*(nc + 2*ghost)"),
    "ghost2": (dict(ghost=2), "ghost must be 0 or 1"),
    "ghost-1": (dict(ghost=-1), "ghost must be 0 or 1"),
    "iv0": (dict(iv=0), "bad variable index"),
    "iv_past": (dict(iv=6), "bad variable index"),           # (the contexts hold n_vars = 5)
    "id0": (dict(first=0), "box id {id} is out of range"),
    "id_past": (dict(first="past"), "box id {id} is out of range"),
    "twice": (dict(first="second"), "box id {id} is listed twice"),
    "null_ids": (dict(ids=None), "NULL ids or box_off with n_boxes > 0"),
    "null_off": (dict(off=None), "NULL ids or box_off with n_boxes > 0"),
    "null_dev": (dict(ptr=0), "NULL pointer with n_boxes > 0"),
    "negative": (dict(n=-1), "negative n_boxes"),
}


def _call(ctx, a, get):
    ids = None if a["ids"] is None else np.array(a["ids"], dtype=np.int32)
    off = None if a["off"] is None else np.array(a["off"], dtype=np.int64)
    C = omg.device.C
    cells = C.c_longlong(-1)
    args = [a["iv"], a["n"], None if ids is None else ids.ctypes.data_as(C.c_void_p),
            C.c_void_p(a["ptr"] or None), None if off is None else off.ctypes.data_as(C.c_void_p),
            np.array(a["stride"], dtype=np.int64), a["ghost"]]
    ctx.call("get_boxes" if get else "put_boxes", *args, *([0] if get else []), None, C.byref(cells))
    return cells.value


@pytest.mark.parametrize("get", [False, True], ids=["put", "get"])
@pytest.mark.parametrize("bad", sorted(BAD))
def test_bad_arguments_are_errors(ranks, bad, get):
    tree, ctx = ranks[0]
    ids = _top_ids(tree)
    assert len(ids) >= 2 and tree.box_size_lvl[tree.highest_lvl] == 8
    b, text = dict(BAD[bad][0]), BAD[bad][1]
    good = dict(iv=2, n=len(ids), ids=ids, ptr=PTR, off=[q * 1000 + 111 for q in range(len(ids))],
                stride=(1, 8, 64), ghost=0)
    good.update(b.pop("good", {}))
    want = len(ids) * (512 + good["ghost"] * 384)
    assert _call(ctx, good, get) == want
    a = dict(good)
    first = b.pop("first", None)
    if first is not None:
        a["ids"] = [{"past": tree.n_boxes + 1, "second": ids[1]}.get(first, first)] + ids[1:]
    a.update(b)
    with pytest.raises(omg.device.OmgError) as ex:
        _call(ctx, a, get)
    assert str(ex.value) == ("omg_get_boxes: " if get else "omg_put_boxes: ") + text.format(id=(a["ids"] or [0])[0])
    assert omg.device.lib().omg_last_error().decode() == str(ex.value)
    assert _call(ctx, good, get) == want   # (the context is as it was)


@pytest.mark.parametrize("get", [False, True], ids=["put", "get"])
def test_a_box_of_another_rank_is_an_error(get):
    ranks = _contexts(U.REFINED, 2)
    try:
        (t0, c0), (t1, _) = ranks
        mine, theirs = _top_ids(t0), _top_ids(t1)
        assert mine and theirs and not set(mine) & set(theirs)
        assert _count(c0, t0, mine, 1, get) == len(mine) * (512 + 384)
        with pytest.raises(omg.device.OmgError, match="omg_get_boxes" if get else "omg_put_boxes") as ex:
            _count(c0, t0, mine[:1] + theirs[:1], 1, get)
        assert "not owned" in str(ex.value)
        assert _count(c0, t0, mine, 1, get) == len(mine) * (512 + 384)
    finally:
        for _, ctx in ranks:
            ctx.close()


def test_replicated_level_put_refused_get_own_boxes_only():
    ranks = _contexts(U.UNIFORM, 2, rep_cells=8 * 8 ** 3)
    try:
        (t0, c0), (t1, _) = ranks
        assert c0.replicated_level() == 0
        mine, theirs = [int(i) for i in t0.lvls[0].my_ids], [int(i) for i in t1.lvls[0].my_ids]
        assert mine and theirs
        top = _top_ids(t0)
        assert _count(c0, t0, mine + top, 1, True) == (len(mine) + len(top)) * (512 + 384)
        with pytest.raises(omg.device.OmgError, match="omg_get_boxes"):
            _count(c0, t0, mine + theirs[:1], 0, True)
        with pytest.raises(omg.device.OmgError, match="omg_put_boxes.*omg_upload_level"):
            _count(c0, t0, top + mine[:1], 0, False)
        assert _count(c0, t0, top, 0, False) == len(top) * 512
    finally:
        for _, ctx in ranks:
            ctx.close()


def test_binding_checks_the_tensor_before_the_call():
    mg = build_tree(parse(U.REFINED), omg.MG())   # (never allocated: a tensor let through raises RuntimeError)
    ids = [int(i) for i in mg.lvls[2].my_ids][:3]
    small = [int(i) for i in mg.lvls[-2].my_ids]
    assert mg.box_size_lvl[2] == 8 and mg.box_size_lvl[-2] == 4 and small
    f64 = torch.float64
    bad = {
        "wrong-m": (torch.zeros(3, 9, 9, 9, dtype=f64), ids, 0, False),
        "wrong-m-ghosts": (torch.zeros(3, 8, 8, 8, dtype=f64), ids, 1, True),
        "not-cubic": (torch.zeros(3, 8, 8, 10, dtype=f64), ids, 0, False),
        "dtype": (torch.zeros(3, 8, 8, 8, dtype=torch.float32), ids, 0, False),
        "ghosts-without-width": (torch.zeros(3, 8, 8, 8, dtype=f64), ids, 0, True),
        "mixed-sizes": (torch.zeros(4, 8, 8, 8, dtype=f64), ids + small[:1], 0, False),
        "len-ids": (torch.zeros(2, 8, 8, 8, dtype=f64), ids, 0, False),
        "last-stride": (torch.zeros(3, 8, 8, 16, dtype=f64)[..., ::2], ids, 0, False),
        "transposed": (torch.zeros(3, 8, 8, 8, dtype=f64).transpose(1, 2), ids, 0, False),
        "rank": (torch.zeros(3, 8, 8, dtype=f64), ids, 0, False),
        "numpy": (np.zeros((3, 8, 8, 8)), ids, 0, False),
        "cpu": (torch.zeros(3, 8, 8, 8, dtype=f64), ids, 0, False),
        "cpu-pool-slice": (torch.zeros(3, 2, 12, 12, 12, dtype=f64)[:, 1], ids, 2, True),
    }
    for what, (t, lst, width, ghosts) in bad.items():
        with pytest.raises(ValueError):
            mg.set_blocks(2, t, lst, ghost_width=width, ghosts=ghosts)
        with pytest.raises(ValueError):
            mg.get_blocks(2, lst, out=t, ghost_width=width, ghosts=ghosts)
    # (the last two pass the layout checks and are refused for their device)
    for what in ("cpu", "cpu-pool-slice"):
        t, lst, width, ghosts = bad[what]
        with pytest.raises(ValueError, match="cpu"):
            mg.set_blocks(2, t, lst, ghost_width=width, ghosts=ghosts)
    assert "omg_put_boxes" in omg.device.SIGNATURES and "omg_get_boxes" in omg.device.SIGNATURES
