"""omg_get_boxes_flux on plan-only contexts (OMG_DEVICE_NONE): the count n_cells
of both centrings on mixed-level lists, every argument check with its message,
the record cache shared with omg_get_boxes_grad, the checks
MG.get_blocks_flux makes before the C call and its default coefficients for
the five operators.  No GPU: a plan-only context validates, counts and
launches nothing."""
import ctypes

import numpy as np
import pytest
import torch

from tests import denseutil as U
from tests.mgdriver import build_tree, omg, parse

CASES = [(args, world) for args in (U.UNIFORM, U.NONCUBE, U.REFINED) for world in (1, 2, 3)]
IDS = [f"{name}-{world}" for name in ("uniform", "noncube", "refined") for world in (1, 2, 3)]
# (non-NULL, 16-B aligned, distinct addresses: never dereferenced without a device)
PTRS = (4096, 4096 + (1 << 30), 4096 + (2 << 30))
CELL, FACE = 0, 1
N_VARS = 7   # (the contexts of this file: room for eps1..3 in variables 5..7)


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def ranks(request):
    args, world = request.param
    out = []
    for r in range(world):
        tree = U.host_tree(args, r, world)
        out.append((tree, U.plan_context(tree, r, world, n_vars=N_VARS)))
    yield out
    for _, ctx in out:
        ctx.close()


def _my_ids(tree):
    """Every box of the rank, all levels, in level order."""
    return [int(i) for lvl in range(tree.lowest_lvl, tree.highest_lvl + 1) for i in tree.lvls[lvl].my_ids]


def _layout(tree, ids, centering):
    """Blocks of the largest box size (+ 1 for faces), one after the other: (box_off, stride)."""
    m = max(tree.box_size_lvl[int(tree.lvl[i])] for i in ids) + centering if len(ids) else 2
    off = np.arange(len(ids), dtype=np.int64) * m ** 3 + centering * (1 + m + m * m)
    return off, (1, m, m * m)


def _want(tree, ids, centering):
    nc = np.array([tree.box_size_lvl[int(tree.lvl[i])] for i in ids], dtype=np.int64)
    return int(((nc + centering) * nc ** 2).sum())


def _count(ctx, tree, ids, centering, iv=1, coef=(5, 5, 5), ptrs=PTRS, accumulate=False):
    off, stride = _layout(tree, ids, centering)
    return ctx.get_boxes_flux(iv, coef, ids, ptrs, off, stride, -1.0, centering, accumulate, False)


def test_the_symbol_and_the_binding_exist():
    assert "omg_get_boxes_flux" in omg.device.SIGNATURES
    assert hasattr(ctypes.CDLL(omg.device.lib_path()), "omg_get_boxes_flux")
    assert hasattr(omg.MG, "get_blocks_flux") and hasattr(omg.device.Context, "get_boxes_flux")


def test_counts_match_the_box_table(ranks):
    seen = []
    for tree, ctx in ranks:
        ids = _my_ids(tree)
        seen += ids
        rng = np.random.default_rng(len(ids))
        perm = [ids[q] for q in rng.permutation(len(ids))]
        sub = perm[:max(len(perm) // 3, 1)]
        for centering in (CELL, FACE):
            for coef in ((5, 5, 5), (5, 6, 7), (0, 0, 0), None, (0, 6, 0)):
                for acc in (False, True):
                    assert _count(ctx, tree, ids, centering, coef=coef, accumulate=acc) == _want(tree, ids, centering)
            assert _count(ctx, tree, perm, centering) == _want(tree, ids, centering)
            assert _count(ctx, tree, sub, centering) == _want(tree, sub, centering) < _want(tree, ids, centering)
            # (a skipped component does not change the count: it is per component)
            assert _count(ctx, tree, ids, centering, ptrs=(0, PTRS[1], 0)) == _want(tree, ids, centering)
        assert _want(tree, ids, FACE) > _want(tree, ids, CELL)
    assert sorted(seen) == list(range(1, ranks[0][0].n_boxes + 1))
    # (rank 0's list mixes levels and box sizes)
    t0 = ranks[0][0]
    assert len({int(t0.lvl[i]) for i in _my_ids(t0)}) > 1 and len({t0.box_size_lvl[int(t0.lvl[i])] for i in _my_ids(t0)}) > 1


def test_an_empty_list_with_null_pointers_counts_zero(ranks):
    ctx = ranks[0][1]
    assert ctx.get_boxes_flux(2, None, None, (0, 0, 0), None, (1, 2, 4), 1.0, CELL, False, True) == 0
    assert ctx.get_boxes_flux(1, (5, 0, 7), [], (0, 0, 0), [], (1, 2, 4), 1.0, FACE, True, False) == 0
    assert ctx.get_boxes_flux(1, (5, 5, 5), [], PTRS, [], (1, 2, 4), 1.0, FACE, False, False) == 0


def _top_ids(tree):
    return [int(i) for i in tree.lvls[tree.highest_lvl].my_ids][:4]


# (every tree's finest boxes hold 8^3 cells: m = 8 for cells, 9 for faces)
# (the change, the message after "omg_get_boxes_flux: "; {id}: the id put first in the list)
FACE_OK = dict(centering=1, stride=(1, 9, 81))
BAD = {
    "stride0": (dict(stride=(2, 8, 64)), "stride[0] must be 1"),
    "stride1": (dict(stride=(1, 7, 64)), "stride[1] < nc"),
    "stride1-face": (dict(centering=1, stride=(1, 8, 81), good=FACE_OK), "stride[1] < nc + 1"),
    "stride2": (dict(stride=(1, 8, 63)), "stride[2] < stride[1]*nc"),
    "stride2-face": (dict(centering=1, stride=(1, 9, 80), good=FACE_OK), "stride[2] < stride[1]*(nc + 1)"),
    "stride-range": (dict(stride=(1, 8, (1 << 40) + 1)), "stride out of range"),
    "centering2": (dict(centering=2), "centering must be 0 (cells) or 1 (faces)"),
    "centering-1": (dict(centering=-1), "centering must be 0 (cells) or 1 (faces)"),
    "iv0": (dict(iv=0), "bad variable index"),
    "iv_past": (dict(iv=N_VARS + 1), "bad variable index"),
    "coef_past": (dict(coef=(5, N_VARS + 1, 5)), f"iv_coef[1] = {N_VARS + 1} is not 0 or a variable 1..{N_VARS}"),
    "coef_negative": (dict(coef=(5, 5, -1)), f"iv_coef[2] = -1 is not 0 or a variable 1..{N_VARS}"),
    "coef_is_iv": (dict(coef=(2, 5, 5)), "iv_coef[0] is iv itself"),
    "coef_is_iv-face": (dict(coef=(0, 0, 2), good=FACE_OK), "iv_coef[2] is iv itself"),
    "id0": (dict(first=0), "box id {id} is out of range"),
    "id_past": (dict(first="past"), "box id {id} is out of range"),
    "twice": (dict(first="second"), "box id {id} is listed twice"),
    "off-range": (dict(off0=(1 << 40) + 1), "box_off out of range"),
    "null_ids": (dict(ids=None), "NULL ids or box_off with n_boxes > 0"),
    "null_off": (dict(off=None), "NULL ids or box_off with n_boxes > 0"),
    "null_array": (dict(ptrs=None), "the array of component pointers is required"),
    "all_null": (dict(ptrs=(0, 0, 0)), "NULL pointers for all three components with n_boxes > 0"),
    "equal01": (dict(ptrs=(PTRS[0], PTRS[0], 0)), "components 0 and 1 share one pointer"),
    "equal02": (dict(ptrs=(PTRS[1], 0, PTRS[1])), "components 0 and 2 share one pointer"),
    "equal12": (dict(ptrs=(PTRS[0], PTRS[2], PTRS[2])), "components 1 and 2 share one pointer"),
    "negative": (dict(n=-1), "negative n_boxes"),
}


def _call(ctx, a):
    ids = None if a["ids"] is None else np.array(a["ids"], dtype=np.int32)
    off = None if a["off"] is None else np.array(a["off"], dtype=np.int64)
    coef = None if a["coef"] is None else np.array(a["coef"], dtype=np.int32)
    C = omg.device.C
    cells = C.c_longlong(-1)
    dev = None if a["ptrs"] is None else (C.c_void_p * 3)(*[C.c_void_p(p or None) for p in a["ptrs"]])
    ctx.call("get_boxes_flux", a["iv"], None if coef is None else coef.ctypes.data_as(C.c_void_p), a["n"],
             None if ids is None else ids.ctypes.data_as(C.c_void_p), dev,
             None if off is None else off.ctypes.data_as(C.c_void_p),
             np.array(a["stride"], dtype=np.int64), 0.37, a["centering"],
             a["accumulate"], 0, None, C.byref(cells))
    return cells.value


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("bad", sorted(BAD))
def test_bad_arguments_are_errors(ranks, bad, accumulate):
    tree, ctx = ranks[0]
    ids = _top_ids(tree)
    assert len(ids) >= 2 and tree.box_size_lvl[tree.highest_lvl] == 8
    b, text = dict(BAD[bad][0]), BAD[bad][1]
    good = dict(iv=2, coef=(5, 6, 7), n=len(ids), ids=ids, ptrs=PTRS, off=[q * 1000 + 111 for q in range(len(ids))],
                stride=(1, 8, 64), centering=0, accumulate=accumulate)
    good.update(b.pop("good", {}))
    want = len(ids) * (8 + good["centering"]) * 64
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
    assert str(ex.value) == "omg_get_boxes_flux: " + text.format(id=(a["ids"] or [0])[0])
    assert omg.device.lib().omg_last_error().decode() == str(ex.value)
    assert _call(ctx, good) == want   # (the context is as it was)


def test_a_null_iv_coef_means_no_coefficient(ranks):
    tree, ctx = ranks[0]
    ids = _top_ids(tree)
    a = dict(iv=2, coef=None, n=len(ids), ids=ids, ptrs=PTRS, off=[q * 1000 + 111 for q in range(len(ids))],
             stride=(1, 8, 64), centering=0, accumulate=0)
    assert _call(ctx, a) == len(ids) * 512


def test_a_list_the_gradient_saw_first_is_served_and_the_other_way_round(ranks):
    """The two entries share one key (the gradient's centring 0 / 1): a list
    either saw first gives the other the same count, whatever iv_coef,
    accumulate and scale are.  (A plan-only context uploads no records, so that
    the cached records are reused without a host wait is checked on the GPU:
    tests/test_gpu_boxes_flux.py.)"""
    tree, ctx = ranks[0]
    ids = _top_ids(tree)
    off, stride = _layout(tree, ids, FACE)
    want = len(ids) * 9 * 64
    assert ctx.get_boxes_grad(1, ids, PTRS, off, stride, 1.0, FACE, False) == want
    for acc in (False, True):
        for coef in ((5, 5, 5), None, (5, 6, 7)):
            assert ctx.get_boxes_flux(1, coef, ids, PTRS, off, stride, -0.5, FACE, acc, False) == want
    # the other way round: a list the flux entry saw first
    sub = ids[::-1]
    assert ctx.get_boxes_flux(1, (5, 5, 5), sub, PTRS, off, stride, 1.0, CELL, False, False) == len(ids) * 512
    assert ctx.get_boxes_grad(1, sub, PTRS, off, stride, 1.0, CELL, False) == len(ids) * 512


def test_pools_that_interleave_are_accepted(ranks):
    """The slices [:, d] of one pool [n, 3, m, m, m]: distinct bases 8*m^3 bytes apart."""
    tree, ctx = ranks[0]
    ids = _top_ids(tree)
    m = 9
    off = np.arange(len(ids), dtype=np.int64) * 3 * m ** 3 + (1 + m + m * m)
    ptrs = [PTRS[0] + 8 * d * m ** 3 for d in range(3)]
    assert ctx.get_boxes_flux(1, (5, 5, 5), ids, ptrs, off, (1, m, m * m), 1.0, FACE, True, False) == len(ids) * 576
    assert ctx.get_boxes_flux(1, (5, 5, 5), ids, ptrs, off, (1, m, m * m), 1.0, CELL, True, False) == len(ids) * 512


def test_a_box_of_another_rank_is_an_error():
    ranks = []
    for r in range(2):
        tree = U.host_tree(U.REFINED, r, 2)
        ranks.append((tree, U.plan_context(tree, r, 2, n_vars=N_VARS)))
    try:
        (t0, c0), (t1, _) = ranks
        mine, theirs = _top_ids(t0), _top_ids(t1)
        assert mine and theirs and not set(mine) & set(theirs)
        for centering in (CELL, FACE):
            assert _count(c0, t0, mine, centering) == len(mine) * (8 + centering) * 64
            with pytest.raises(omg.device.OmgError, match="omg_get_boxes_flux") as ex:
                _count(c0, t0, mine[:1] + theirs[:1], centering)
            assert "not owned" in str(ex.value)
            assert _count(c0, t0, mine, centering) == len(mine) * (8 + centering) * 64
    finally:
        for _, ctx in ranks:
            ctx.close()


def test_default_coefficients_of_the_five_operators():
    want = {U.T.MG_LAPLACIAN: (0, 0, 0), U.T.MG_HELMHOLTZ: (0, 0, 0), U.T.MG_VLAPLACIAN: (5, 5, 5),
            U.T.MG_VHELMHOLTZ: (5, 5, 5), U.T.MG_AHELMHOLTZ: (5, 6, 7)}
    assert len(want) == 5
    mg = omg.MG()
    for op, coef in want.items():
        mg.operator_type = op
        assert mg.flux_coefficients() == coef == mg.flux_coefficients(None)
        # an explicit coef overrides the operator's
        assert mg.flux_coefficients(6) == (6, 6, 6)
        assert mg.flux_coefficients((5, None, 0)) == (5, 0, 0)
        assert mg.flux_coefficients([7, 6, 5]) == (7, 6, 5)
    for bad in ((5, 5), (5, 5, 5, 5), "eps", 1.5):
        with pytest.raises(ValueError):
            mg.flux_coefficients(bad)
    mg.operator_type = 99
    with pytest.raises(ValueError):
        mg.flux_coefficients()


def test_binding_checks_before_the_call():
    mg = build_tree(parse(U.REFINED), omg.MG())   # (never allocated: tensors let through raise RuntimeError)
    ids = [int(i) for i in mg.lvls[2].my_ids][:3]
    small = [int(i) for i in mg.lvls[-2].my_ids]
    assert mg.box_size_lvl[2] == 8 and mg.box_size_lvl[-2] == 4 and small
    mg.n_extra_vars = 3
    f64 = torch.float64
    z = lambda *shape, **kw: torch.zeros(*shape, dtype=kw.get("dtype", f64))   # noqa: E731
    ok = dict(ids=ids, out=z(3, 3, 10, 10, 10), ghost_width=1, centering="face", components=(True,) * 3,
              coef=(5, 6, 7), accumulate=False, iv=1)
    bad = {
        "accumulate-without-out": dict(out=None, accumulate=True),
        "wrong-m": dict(out=z(3, 3, 9, 9, 9)),
        "not-cubic": dict(out=z(3, 3, 10, 10, 12)),
        "dtype": dict(out=z(3, 3, 10, 10, 10, dtype=torch.float32)),
        "face-without-a-ghost-layer": dict(out=z(3, 3, 8, 8, 8), ghost_width=0),
        "centering": dict(centering="edge"),
        "mixed-sizes": dict(out=z(3, 4, 10, 10, 10), ids=ids + small[:1]),
        "len-ids": dict(out=z(3, 2, 10, 10, 10)),
        "last-stride": dict(out=z(3, 3, 10, 10, 20)[..., ::2]),
        "rank": dict(out=z(3, 10, 10, 10)),
        "two-components": dict(out=z(2, 3, 10, 10, 10)),
        "numpy": dict(out=np.zeros((3, 3, 10, 10, 10))),
        "two-tensors": dict(out=[z(3, 10, 10, 10), z(3, 10, 10, 10)]),
        "differing-strides": dict(out=[z(3, 10, 10, 10), z(3, 10, 10, 12)[..., :10], None]),
        "no-component": dict(out=[None, None, None]),
        "masked-away": dict(components=(False,) * 3),
        "two-flags": dict(components=(True, True)),
        "coef-two": dict(coef=(5, 6)),
        "coef-past": dict(coef=8),
        "coef-negative": dict(coef=(5, -1, 5)),
        "coef-is-iv": dict(coef=(5, 1, 5)),
        "coef-is-iv-rhs": dict(coef=2, iv=2),
        "cpu": dict(),
        "cpu-cell-accumulate": dict(out=z(3, 3, 8, 8, 8), ghost_width=0, centering="cell", accumulate=True),
    }
    for what, change in bad.items():
        a = dict(ok, **change)
        with pytest.raises(ValueError):
            mg.get_blocks_flux(a.pop("ids"), **a)
    # (the last two pass the layout checks and are refused for their device)
    for what in ("cpu", "cpu-cell-accumulate"):
        a = dict(ok, **bad[what])
        with pytest.raises(ValueError, match="cpu"):
            mg.get_blocks_flux(a.pop("ids"), **a)
