"""omg_get_dense_grad on plan-only contexts (OMG_DEVICE_NONE): the binding, the
coverage count n_cells against a numpy count over the box table, and the
argument checks.  No GPU: a plan-only context validates, counts and launches
nothing.  `get_dense_grad` below is the C entry through Context.get_dense_grad."""
import ctypes

import numpy as np
import pytest
import torch

from tests import denseutil as U
from tests.mgdriver import omg

# (tree, ranks)
CASES = [(U.UNIFORM, 1), (U.NONCUBE, 1), (U.REFINED, 1), (U.NONCUBE, 2), (U.REFINED, 2)]
IDS = ["uniform", "noncube", "refined", "noncube-2", "refined-2"]
# non-NULL, 16-B aligned addresses far apart: never dereferenced without a device
PTRS = (1 << 40, 2 << 40, 3 << 40)


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


def _count(ctx, lvl, lo, n, ptrs=PTRS, **kw):
    return ctx.get_dense_grad(lvl, 1, ptrs, lo, n, U.contiguous(n), **kw)


def test_the_entry_is_bound_and_exported():
    assert "omg_get_dense_grad" in omg.device.SIGNATURES
    assert hasattr(ctypes.CDLL(omg.device.lib_path()), "omg_get_dense_grad")
    assert callable(omg.device.Context.get_dense_grad) and callable(omg.MG.get_dense_grad)


def test_whole_windows_cover_every_box(ranks):
    tree = ranks[0][0]
    for lvl in range(tree.lowest_lvl, tree.highest_lvl + 1):
        g = U.grid(tree, lvl)
        want = len(tree.lvls[lvl].ids) * tree.box_size_lvl[lvl] ** 3
        assert want == U.count_cells(tree, lvl, (0, 0, 0), g)
        got = [_count(ctx, lvl, (0, 0, 0), g) for _, ctx in ranks]
        assert got == [U.count_cells(t, lvl, (0, 0, 0), g, t.lvls[lvl].my_ids) for t, _ in ranks], lvl
        assert sum(got) == want, lvl
    if tree.highest_lvl > 1:   # (a refined level: part of its grid has no box)
        hi, g = tree.highest_lvl, U.grid(tree, tree.highest_lvl)
        assert 0 < U.count_cells(tree, hi, (0, 0, 0), g) < g[0] * g[1] * g[2]
    if len(ranks) > 1:         # (two ranks: both hold a part of the top level)
        assert all(0 < c < want for c in got)


def test_cut_windows_match_the_box_table(ranks):
    tree = ranks[0][0]
    for lvl in range(tree.lowest_lvl, tree.highest_lvl + 1):
        for lo, n in U.cut_windows(tree, lvl):
            total = 0
            for t, ctx in ranks:
                got = _count(ctx, lvl, lo, n)
                assert got == U.count_cells(t, lvl, lo, n, t.lvls[lvl].my_ids), (lvl, lo, n)
                # the count depends on neither the mask, the scale nor the fill flag
                assert got == _count(ctx, lvl, lo, n, ptrs=(0, PTRS[1], 0), scale=-1.0, fill=False)
                total += got
            assert total == U.count_cells(tree, lvl, lo, n), (lvl, lo, n)
    hi = tree.highest_lvl
    wins = U.cut_windows(tree, hi)
    for lo, n in wins:   # (the windows do cut: neither empty nor everything)
        assert 0 < U.count_cells(tree, hi, lo, n) < len(tree.lvls[hi].ids) * tree.box_size_lvl[hi] ** 3
    lo, n = wins[-1]     # (the last one reaches outside the domain)
    assert lo[0] < 0 and lo[0] + n[0] > U.grid(tree, hi)[0]


def test_strided_unaligned_and_empty_windows_count_alike(ranks):
    tree, ctx = ranks[0]
    lo, n = U.cut_windows(tree, 1)[0]
    want = U.count_cells(tree, 1, lo, n, tree.lvls[1].my_ids)
    assert ctx.get_dense_grad(1, 2, PTRS, lo, n, (1, n[0] + 3, (n[0] + 3) * (n[1] + 2))) == want
    assert ctx.get_dense_grad(1, 2, (PTRS[0] + 8, PTRS[1], PTRS[2]), lo, n, U.contiguous(n)) == want
    # (empty: every pointer may be NULL)
    assert ctx.get_dense_grad(1, 2, (0, 0, 0), lo, (n[0], 0, n[2]), (1, n[0], 0)) == 0


# (the change, the message after "omg_get_dense_grad: ")
BAD = {
    "no_level": (dict(lvl=99), "no such level"),
    "iv0": (dict(iv=0), "bad variable index"),
    "iv_past": (dict(iv=6), "bad variable index"),           # (the contexts hold n_vars = 5)
    "negative": (dict(n=(8, -1, 8)), "negative extent"),
    "stride0": (dict(stride=(2, 8, 64)), "stride[0] must be 1"),
    "stride1": (dict(stride=(1, 7, 64)), "stride[1] < n[0]"),
    "stride2": (dict(stride=(1, 8, 63)), "stride[2] < stride[1]*n[1]"),
    "all_null": (dict(ptrs=(0, 0, 0)), "NULL pointers for all three components with a non-empty window"),
    "overlap": (dict(ptrs=(PTRS[0], PTRS[0] + 8 * 511, 0)), "the windows of components 0 and 1 overlap"),
}


@pytest.mark.parametrize("bad", sorted(BAD))
def test_bad_arguments_are_errors(ranks, bad):
    ctx = ranks[0][1]
    a = dict(lvl=1, iv=2, ptrs=PTRS, lo=(0, 0, 0), n=(8, 8, 8), stride=(1, 8, 64))
    call = lambda: ctx.get_dense_grad(a["lvl"], a["iv"], a["ptrs"], a["lo"], a["n"], a["stride"])  # noqa: E731
    assert call() == 512
    change, text = BAD[bad]
    a.update(change)
    with pytest.raises(omg.device.OmgError) as ex:
        call()
    assert str(ex.value) == "omg_get_dense_grad: " + text
    assert omg.device.lib().omg_last_error().decode() == str(ex.value)
    a.update(dict(lvl=1, iv=2, ptrs=(PTRS[0], PTRS[0] + 8 * 512, 0), n=(8, 8, 8), stride=(1, 8, 64)))
    assert call() == 512   # (the context stays usable; windows that only touch do not overlap)


def test_n_cells_may_be_null(ranks):
    ctx = ranks[0][1]
    i64 = lambda a: np.array(a, dtype=np.int64)  # noqa: E731
    dev = (ctypes.c_void_p * 3)(*PTRS)
    ctx.call("get_dense_grad", 1, 1, dev, i64((0, 0, 0)), i64((8, 8, 8)), i64((1, 8, 64)), 1.0, 1, None, None)


def test_binding_checks_the_tensors_before_the_call():
    mg = omg.MG()   # (never allocated: a check that let the tensors through would raise RuntimeError)
    ok = torch.zeros(3, 4, 4, 4, dtype=torch.float64)
    for what, t in (("dtype", torch.zeros(3, 4, 4, 4, dtype=torch.float32)),
                    ("stride", torch.zeros(3, 4, 4, 8, dtype=torch.float64)[..., ::2]),
                    ("transposed", torch.zeros(3, 6, 4, 8, dtype=torch.float64).transpose(1, 2)),
                    ("device", ok),
                    ("rank", torch.zeros(4, 4, 4, dtype=torch.float64)),
                    ("two", torch.zeros(2, 4, 4, 4, dtype=torch.float64)),
                    ("tensor", np.zeros((3, 4, 4, 4))),
                    ("list-of-two", [ok[0], ok[1]]),
                    ("nothing", [None, None, None])):
        with pytest.raises(ValueError):
            mg.get_dense_grad(1, out=t)
    for t in ([ok[0], ok[1][:2], None], [ok[0], torch.zeros(4, 4, 8, dtype=torch.float64)[:, :, :4], None]):
        with pytest.raises(ValueError, match="differ in shape or strides"):
            mg.get_dense_grad(1, out=t)
    with pytest.raises(ValueError):
        mg.get_dense_grad(1, out=ok, components=(False, False, False))
    with pytest.raises(ValueError, match="cpu"):   # (past the layout checks: refused for its device)
        mg.get_dense_grad(1, out=[None, ok[1], None])
