"""omg_put_dense / omg_get_dense on plan-only contexts (OMG_DEVICE_NONE): the
coverage count n_cells against a numpy count over the box table, the argument
checks, and the checks MG.set_dense / MG.get_dense make before the C call.
No GPU: a plan-only context validates, counts and copies nothing."""
import numpy as np
import pytest
import torch

from tests import denseutil as U
from tests.mgdriver import omg

# (tree, ranks)
CASES = [(U.UNIFORM, 1), (U.NONCUBE, 1), (U.REFINED, 1), (U.NONCUBE, 2), (U.NONCUBE, 3), (U.REFINED, 2),
         (U.REFINED, 3)]
IDS = ["uniform", "noncube", "refined", "noncube-2", "noncube-3", "refined-2", "refined-3"]
PTR = 4096   # (a non-NULL, 16-B aligned address: never dereferenced without a device)


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def ranks(request):
    args, world = request.param
    out = []
    for r in range(world):
        tree = U.host_tree(args, r, world)
        out.append((tree, U.plan_context(tree, r, world)))
    yield out
    for _, ctx in out:
        ctx.close()


def _count(ctx, lvl, lo, n, get):
    f = ctx.get_dense if get else ctx.put_dense
    return f(lvl, 2, PTR, lo, n, U.contiguous(n))


def test_full_grid_covers_every_box(ranks):
    tree = ranks[0][0]
    for lvl in range(tree.lowest_lvl, tree.highest_lvl + 1):
        g = U.grid(tree, lvl)
        want = len(tree.lvls[lvl].ids) * tree.box_size_lvl[lvl] ** 3
        for get in (False, True):
            assert sum(_count(ctx, lvl, (0, 0, 0), g, get) for _, ctx in ranks) == want, (lvl, get)


def test_cut_windows_match_the_box_table(ranks):
    for lvl in range(ranks[0][0].lowest_lvl, ranks[0][0].highest_lvl + 1):
        for lo, n in U.cut_windows(ranks[0][0], lvl):
            total = 0
            for tree, ctx in ranks:
                got = _count(ctx, lvl, lo, n, True)
                assert got == _count(ctx, lvl, lo, n, False)
                assert got == U.count_cells(tree, lvl, lo, n, tree.lvls[lvl].my_ids), (lvl, lo, n)
                total += got
            assert total == U.count_cells(ranks[0][0], lvl, lo, n), (lvl, lo, n)
    # (the windows do cut: on the finest level neither empty nor everything)
    tree = ranks[0][0]
    hi = tree.highest_lvl
    for lo, n in U.cut_windows(tree, hi):
        assert 0 < U.count_cells(tree, hi, lo, n) < len(tree.lvls[hi].ids) * tree.box_size_lvl[hi] ** 3


def test_strided_and_empty_windows_count_alike(ranks):
    tree, ctx = ranks[0]
    lo, n = U.cut_windows(tree, 1)[0]
    want = U.count_cells(tree, 1, lo, n, tree.lvls[1].my_ids)
    assert ctx.put_dense(1, 2, PTR, lo, n, (1, n[0] + 3, (n[0] + 3) * (n[1] + 2))) == want
    assert ctx.put_dense(1, 2, PTR + 8, lo, n, U.contiguous(n)) == want
    assert ctx.get_dense(1, 2, 0, lo, (n[0], 0, n[2]), (1, n[0], 0)) == 0   # (empty: NULL is fine)


# (the change, the message after "omg_put_dense: " / "omg_get_dense: ")
def test_six_windows_through_four_slots_are_each_counted_afresh(ranks):
    """The level keeps the clipping of four windows, which omg_get_dense and
    omg_get_dense_grad share: six windows in turn and the first again, through
    the two entries alternately.  A slot that is reused is rebuilt completely."""
    tree0 = ranks[0][0]
    hi = tree0.highest_lvl
    assert tree0.box_size_lvl[hi] == 8
    # six windows inside the bounding box of the level's boxes, each smaller than the one before
    org = np.array([U.box_origin(tree0, hi, i) for i in tree0.lvls[hi].ids])
    b0, b1 = org.min(axis=0), org.max(axis=0) + 8
    wins = [(tuple(int(v) for v in b0 + (q, 0, q // 2)), tuple(int(v) for v in b1 - b0 - (2 * q, q, q)))
            for q in range(6)]
    wins.append(wins[0])
    totals = []
    for tree, ctx in ranks:
        want = [U.count_cells(tree, hi, lo, n, tree.lvls[hi].my_ids) for lo, n in wins]
        got = []
        for q, (lo, n) in enumerate(wins):
            if q % 2:
                got.append(ctx.get_dense_grad(hi, 1, (1 << 40, 2 << 40, 3 << 40), lo, n, U.contiguous(n)))
            else:
                got.append(ctx.get_dense(hi, 2, PTR, lo, n, U.contiguous(n)))
        assert got == want
        totals.append(want)
    # (the windows differ in what they cover, so a count left over from the slot's last window would show)
    assert len({sum(t[q] for t in totals) for q in range(6)}) == 6


BAD = {
    "stride0": (dict(stride=(2, 8, 64)), "stride[0] must be 1"),
    "stride1": (dict(stride=(1, 7, 64)), "stride[1] < n[0]"),
    "stride2": (dict(stride=(1, 8, 63)), "stride[2] < stride[1]*n[1]"),
    "negative": (dict(n=(8, -1, 8)), "negative extent"),
    "iv0": (dict(iv=0), "bad variable index"),
    "iv_past": (dict(iv=6), "bad variable index"),           # (the contexts hold n_vars = 5)
    "no_level": (dict(lvl=99), "no such level"),
    "null": (dict(ptr=0), "NULL pointer with a non-empty window"),
}


@pytest.mark.parametrize("get", [False, True], ids=["put", "get"])
@pytest.mark.parametrize("bad", sorted(BAD))
def test_bad_arguments_are_errors(ranks, bad, get):
    ctx = ranks[0][1]
    a = dict(lvl=1, iv=2, ptr=PTR, lo=(0, 0, 0), n=(8, 8, 8), stride=(1, 8, 64))
    f = ctx.get_dense if get else ctx.put_dense
    assert f(a["lvl"], a["iv"], a["ptr"], a["lo"], a["n"], a["stride"]) == 512
    change, text = BAD[bad]
    a.update(change)
    with pytest.raises(omg.device.OmgError) as ex:
        f(a["lvl"], a["iv"], a["ptr"], a["lo"], a["n"], a["stride"])
    assert str(ex.value) == ("omg_get_dense: " if get else "omg_put_dense: ") + text
    assert omg.device.lib().omg_last_error().decode() == str(ex.value)


def test_n_cells_may_be_null(ranks):
    ctx = ranks[0][1]
    i64 = lambda a: np.array(a, dtype=np.int64)  # noqa: E731
    ctx.call("put_dense", 1, 2, PTR, i64((0, 0, 0)), i64((8, 8, 8)), i64((1, 8, 64)), None, None)


def test_binding_checks_the_tensor_before_the_call():
    mg = omg.MG()   # (never allocated: a check that let the tensor through would raise RuntimeError)
    ok = torch.zeros(4, 4, 4, dtype=torch.float64)
    for what, t in (("dtype", torch.zeros(4, 4, 4, dtype=torch.float32)),
                    ("stride", torch.zeros(4, 4, 8, dtype=torch.float64)[:, :, ::2]),
                    ("transposed", torch.zeros(6, 4, 8, dtype=torch.float64).transpose(0, 1)),
                    ("expanded", torch.zeros(1, 4, 8, dtype=torch.float64).expand(3, 4, 8)),
                    ("overlapping", torch.zeros(64, dtype=torch.float64).as_strided((3, 4, 8), (16, 4, 1))),
                    ("device", ok),
                    ("rank", torch.zeros(4, 4, dtype=torch.float64)),
                    ("tensor", np.zeros((4, 4, 4)))):
        with pytest.raises(ValueError):
            mg.set_dense(1, 2, t)
        with pytest.raises(ValueError):
            mg.get_dense(1, 2, out=t)
    # the strides handed on are the tensor's own; those of size-1 dimensions (arbitrary in torch) the dense ones
    big = torch.zeros(5, 7, 9, dtype=torch.float64)
    for t, want in ((big, (1, 9, 63)), (big[1:4, 2:6, 3:8], (1, 9, 63)), (big[:, 3:4, :], (1, 9, 63)),
                    (big[2:3, :, :4], (1, 9, 63)), (big[2:3, 3:4, :4], (1, 4, 4)),
                    (torch.zeros(3, 1, 8, dtype=torch.float64).as_strided((3, 1, 8), (8, 1000, 1)), (1, 8, 8))):
        assert omg.mg.dense_strides(t)[1] == want, (tuple(t.shape), tuple(t.stride()))
        with pytest.raises(ValueError, match="cpu"):   # (past the stride checks: refused for its device)
            mg.set_dense(1, 2, t)
    assert "omg_put_dense" in omg.device.SIGNATURES and "omg_get_dense" in omg.device.SIGNATURES
    assert callable(omg.MG.set_dense) and callable(omg.MG.get_dense)
