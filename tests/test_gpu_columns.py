"""The block passes' tables as a GPU context holds them against a plan-only
context of the same tree (omg_plan_columns): identical arrays, the column
records and the coarse records, on every level.  What the plan-only ones must
be is tests/test_columns_host.py's subject, without a GPU."""
import numpy as np
import pytest

from tests.mgdriver import DeviceBackend, omg, parse

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bc", ["per", "d0"])
def test_gpu_context_holds_the_plan_only_tables(monkeypatch, bc):
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", "1")   # (read at context creation)
    be = DeviceBackend(parse(f"16 64 64 64 1 v gsrb lpl 0 {bc} sol 1 lb 0"))
    mg = be.mg
    host = omg.device.Context(-2, 0, 1)   # OMG_DEVICE_NONE
    arrs = omg.mg._tree_arrays(mg)
    host.call("tree_setup", mg.n_boxes, *arrs[:6], mg.lowest_lvl, mg.highest_lvl, mg.first_normal_lvl,
              mg.box_size, arrs[6], arrs[7], arrs[8], arrs[9], 5)
    n = [0, 0]
    for lvl in be.levels():
        for which in (0, 1):
            a, b = mg.ctx.plan_columns(lvl, which), host.plan_columns(lvl, which)
            assert a.shape == b.shape and np.array_equal(a, b), (lvl, which)
            n[which] += a.shape[0]
    # (level 1: 16 columns, level 0: 2; the periodic tree has coarse records for both)
    assert n == ([18, 18] if bc == "per" else [18, 0])
    host.close()
    omg.mg_deallocate_storage(mg)
