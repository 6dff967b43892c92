"""The leaf rhs mean shifts a stand-alone periodic cycle leaves pending
(octree-mg_amd/csrc/omg_mean.cpp, Level::rhs_pend) against the C oracle, every
stored cell of variables 1-4 on every level.

mg_fas_vcycle begins every periodic cycle with rhs <- rhs - mean(rhs).  The
device keeps up to kRhsPendMax of those means in a list instead of writing
rhs: k_gsrb4, k_resid_restrict and the box sums subtract the list from the
rhs values they load, and the cycle after writes it out.  The tests of the
other files read rhs back after every cycle, which writes the list out at
depth 1; here cycles run back to back, and what then reads rhs comes only
after several of them: a download, FMG, apply_op, an upload, a cycle whose
smoothing runs one substep per launch (each must write the list out first),
and the max residual (which takes the list)."""
import os
import re

import numpy as np
import pytest

from tests.mgdriver import OPS, DeviceBackend, OracleBackend, parse, setup_problem
from tests.test_gpu_block3 import _assert_same, _pair

pytestmark = pytest.mark.gpu

ARGS = "16 128 128 128 3 v gsrb lpl 0 per sol 1 lb 0"
HELM = "16 128 128 128 3 v gsrb helm 2 per sol 1 lb 0"


def _k_max():
    """kRhsPendMax of the library's source."""
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "octree-mg_amd", "csrc", "omg_internal.h")) as f:
        m = re.search(r"constexpr int kRhsPendMax = (\d+);", f.read())
    return int(m.group(1))


K = _k_max()


@pytest.fixture(autouse=True, params=["512", "64"])
def _small_levels(monkeypatch, request):
    """The 512-box finest level of the 128^3 tree (and at 64 the 64-box level
    below it) takes the block passes, as C3's levels of 4096 boxes and more do
    by default (kB3MinBoxes; read at context creation)."""
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", request.param)


def _set_counts(dev, orc, down, up):
    import pyoracle
    dev.mg.n_cycle_down, dev.mg.n_cycle_up = down, up
    dev.mg._push_methods()
    orc.o.configure(op=OPS[dev.cfg["op"]], lam=dev.cfg["lam"], smoother=pyoracle.GSRB, n_cycle_down=down,
                    n_cycle_up=up, subtract_mean=True)


# 1. every list depth, the cycle that writes the list out and the one after it
@pytest.mark.parametrize("n", range(1, K + 3))
def test_back_to_back_cycles_match_oracle(n):
    dev, orc = _pair(ARGS, 2, 2)
    for _ in range(n):
        dev.vcycle(False)
        orc.vcycle(False)
    _assert_same(dev, orc)


def _read_download(dev, orc):
    top = dev.levels()[-1]
    a, b = dev.get_level(top, 2), orc.get_level(top, 2)
    assert np.array_equal(a[:, 1:-1, 1:-1, 1:-1].view(np.uint64), b[:, 1:-1, 1:-1, 1:-1].view(np.uint64))


def _read_fmg(dev, orc):
    assert dev.fmg(True, True) == orc.fmg(True, True)


def _read_apply_op(dev, orc):
    # (i_out = 2: the operator's result replaces rhs on every level, on both sides)
    dev.apply_op(2)
    orc.apply_op(2)


def _read_upload(dev, orc):
    # rhs of the finest level goes up again, scaled: a write that must not
    # meet shifts still pending (they would then apply to the new values)
    top = dev.levels()[-1]
    new = 0.5 * orc.get_level(top, 2)
    dev.set_level(top, 2, new)
    orc.set_level(top, 2, new)


def _read_one_substep(dev, orc):
    # one substep per launch on the way down and up: kernels that take no list
    _set_counts(dev, orc, 1, 1)
    assert dev.vcycle(True) == orc.vcycle(True)
    _set_counts(dev, orc, 2, 2)


def _read_max_res(dev, orc):
    # the max residual at the end of the cycle takes the list (k_resid_restrict)
    assert dev.vcycle(True) == orc.vcycle(True)


# 2. each kind of reader at depth >= 2
@pytest.mark.parametrize("reader", [_read_download, _read_fmg, _read_apply_op, _read_upload, _read_one_substep,
                                    _read_max_res], ids=lambda f: f.__name__[6:])
def test_reader_after_two_cycles(reader):
    dev, orc = _pair(ARGS, 2, 2)
    for _ in range(2):
        dev.vcycle(False)
        orc.vcycle(False)
    reader(dev, orc)
    _assert_same(dev, orc)
    for _ in range(2):
        dev.vcycle(False)
        orc.vcycle(False)
    _assert_same(dev, orc)


# 3. OMG_NO_RHS_PEND=1: every cycle writes rhs - mean at once
def test_switch_off_same_bits(monkeypatch):
    dev, orc = _pair(ARGS, 2, 2)
    monkeypatch.setenv("OMG_NO_RHS_PEND", "1")
    ref = DeviceBackend(parse(ARGS))
    ref.mg.n_cycle_down, ref.mg.n_cycle_up = 2, 2
    ref.mg._push_methods()
    setup_problem(ref)
    for _ in range(3):
        dev.vcycle(False)
        ref.vcycle(False)
        orc.vcycle(False)
        _assert_same(dev, ref)
        _assert_same(dev, orc)


# 4. other smoothing counts; Helmholtz with the mean subtracted
@pytest.mark.parametrize("down,up", [(3, 1), (1, 3), (4, 4)])
def test_other_counts_back_to_back(down, up):
    dev, orc = _pair(ARGS, down, up)
    for _ in range(3):
        dev.vcycle(False)
        orc.vcycle(False)
    _assert_same(dev, orc)


def test_helmholtz_subtract_mean_back_to_back():
    dev, orc = _pair(HELM, 2, 2, subtract_mean=True)
    for _ in range(3):
        dev.vcycle(False)
        orc.vcycle(False)
    _assert_same(dev, orc)


# 5. the list is really kept: over kRhsPendMax + 1 cycles one launch writes rhs
def _launches(dev, n_cycles):
    c, top = dev.mg.ctx, dev.levels()[-1]
    for _ in range(K + 1):   # (ends on the cycle that writes the list out; the rhs sums are chained from here on)
        dev.vcycle(False)
    c.call("reset_stats")
    c.call("set_profiling", 1)
    for _ in range(n_cycles):
        dev.vcycle(False)
    c.call("set_profiling", 0)
    return c.kernel_stats(f"subtract_rhs@{top}")[0], c.kernel_stats(f"box_sums@{top}")[0]


def test_one_storing_launch_per_window(monkeypatch):
    dev, _ = _pair(ARGS, 2, 2)
    n_sub, n_sums = _launches(dev, K + 1)
    if os.environ["OMG_BLOCK3_MIN_BOXES"] == "64":
        # C3's arrangement: k_gsrb4 down, k_resid_restrict, k_gsrb4's correction form up
        assert n_sub == 1
        assert n_sums == (K + 1) + K   # phi's sums every cycle, the read-only rhs pass on K of them
    else:
        # the 64-box level below runs no block pass, so the finest level's
        # up-smoothing is k_gsrb3's correction form and a one-substep launch,
        # which take no list: the first cycle had to write the shifts out, and
        # the level's cycles subtract at once from then on (never two passes)
        assert n_sub == K + 1
        assert n_sums == K + 1
    monkeypatch.setenv("OMG_NO_RHS_PEND", "1")
    ref = DeviceBackend(parse(ARGS))
    ref.mg.n_cycle_down, ref.mg.n_cycle_up = 2, 2
    ref.mg._push_methods()
    setup_problem(ref)
    n_sub, n_sums = _launches(ref, K + 1)
    assert n_sub == K + 1
    assert n_sums == K + 1
