"""The top level's res a stand-alone cycle leaves unstored
(octree-mg_amd/csrc/omg_cycle.cpp, Level::res_pend) against the C oracle, every
stored cell of variables 1-4 on every level; res is variable 4.

update_coarse's residual on the top level of a stand-alone cycle over the
whole tree runs without its store of res where nothing reads it: the
restriction leaves the same launch, the up leg reads the coarse level's res,
and the next cycle (or this cycle's max residual) overwrites every box.  The
level notes the phi buffer the launch read; whoever may read res, or is about
to write that buffer, launches the storing form over it first.  The tests of
the other files read res back after every cycle; here cycles run back to
back, and each kind of reader comes only after several of them."""
import numpy as np
import pytest

import tests.denseutil as U
from tests.mgdriver import OPS, DeviceBackend, parse, setup_problem
from tests.test_gpu_block3 import _assert_same, _pair

pytestmark = pytest.mark.gpu

ARGS = "16 128 128 128 3 v gsrb lpl 0 per sol 1 lb 0"
HELM = "16 128 128 128 3 v gsrb helm 2 per sol 1 lb 0"
DIRICHLET = "16 128 128 128 3 v gsrb lpl 0 d0 sol 1 lb 0"
IRES = 4


@pytest.fixture(autouse=True, params=["512", "64"])
def _small_levels(monkeypatch, request):
    """The 512-box finest level of the 128^3 tree (and at 64 the 64-box level
    below it) takes the block passes, as C3's levels of 4096 boxes and more do
    by default (kB3MinBoxes; read at context creation).  At 64 the finest
    level's passes are C3's: k_gsrb4 down, k_resid_restrict, k_gsrb4's
    correction form up; at 512 its up-smoothing is k_gsrb3's correction form
    and a one-substep launch."""
    monkeypatch.setenv("OMG_BLOCK3_MIN_BOXES", request.param)


def _set_counts(dev, orc, down, up):
    import pyoracle
    dev.mg.n_cycle_down, dev.mg.n_cycle_up = down, up
    dev.mg._push_methods()
    orc.o.configure(op=OPS[dev.cfg["op"]], lam=dev.cfg["lam"], smoother=pyoracle.GSRB, n_cycle_down=down,
                    n_cycle_up=up, subtract_mean=True)


def _cycles(dev, orc, n):
    for _ in range(n):
        dev.vcycle(False)
        orc.vcycle(False)


class _Count:
    """Launches of the Prof name `residual` on the top level (materialize_res,
    residual_lvl) while the block runs."""

    def __init__(self, dev):
        self.c, self.top = dev.mg.ctx, dev.levels()[-1]

    def __enter__(self):
        self.c.call("reset_stats")
        self.c.call("set_profiling", 1)
        return self

    def __exit__(self, *exc):
        self.c.call("set_profiling", 0)

    def n(self):
        self.c.call("set_profiling", 0)
        n = self.c.kernel_stats(f"residual@{self.top}")[0]
        self.c.call("set_profiling", 1)
        return n


# 1. cycles back to back, the last one without and with the max residual
@pytest.mark.parametrize("max_res", [False, True])
@pytest.mark.parametrize("n", range(1, 5))
def test_back_to_back_cycles_match_oracle(n, max_res):
    dev, orc = _pair(ARGS, 2, 2)
    _cycles(dev, orc, n - 1)
    assert dev.vcycle(max_res) == orc.vcycle(max_res)
    _assert_same(dev, orc)


# 2. each kind of reader after two cycles
def _read_download_res(dev, orc):
    top = dev.levels()[-1]
    a, b = dev.get_level(top, IRES), orc.get_level(top, IRES)
    assert np.array_equal(a[:, 1:-1, 1:-1, 1:-1].view(np.uint64), b[:, 1:-1, 1:-1, 1:-1].view(np.uint64))


def _read_download_phi(dev, orc):
    top = dev.levels()[-1]
    a, b = dev.get_level(top, 1), orc.get_level(top, 1)
    assert np.array_equal(a[:, 1:-1, 1:-1, 1:-1].view(np.uint64), b[:, 1:-1, 1:-1, 1:-1].view(np.uint64))


def _read_upload_phi(dev, orc):
    # phi of the finest level goes up again, scaled: the write lands in the
    # buffer the up leg left current, and the res still to store is the one of
    # the values before it
    top = dev.levels()[-1]
    new = 0.5 * orc.get_level(top, 1)
    dev.set_level(top, 1, new)
    orc.set_level(top, 1, new)


def _read_upload_rhs(dev, orc):
    top = dev.levels()[-1]
    new = 0.5 * orc.get_level(top, 2)
    dev.set_level(top, 2, new)
    orc.set_level(top, 2, new)


def _read_apply_op(dev, orc):
    dev.apply_op(2)
    orc.apply_op(2)


def _read_fmg(dev, orc):
    assert dev.fmg(True, True) == orc.fmg(True, True)


def _read_partial_cycle(dev, orc):
    # a cycle up to the level below the top: the top level's res stays as the
    # cycle before left it
    k = dev.levels()[-1] - 1
    assert dev.vcycle_to(k, True, True) == orc.vcycle_to(k, True, True)


def _read_subtract_mean(dev, orc):
    dev.call("subtract_mean", 1, 1)
    orc.call("subtract_mean", 1, 1)


def _read_smooth_boxes(dev, orc):
    top = dev.levels()[-1]
    dev.call("smooth_boxes", top, 1)
    orc.call("smooth_boxes", top, 1)


def _read_one_substep(dev, orc):
    _set_counts(dev, orc, 1, 1)
    assert dev.vcycle(True) == orc.vcycle(True)
    _set_counts(dev, orc, 2, 2)


def _read_get_dense(dev, orc):
    top = dev.levels()[-1]
    ids = dev.tree.lvls[top].my_ids
    got, cells = dev.mg.get_dense(top, IRES)
    assert cells == len(ids) * dev.tree.box_size_lvl[top] ** 3
    want = U.assemble(dev.tree, top, ids, orc.get_level(top, IRES), U.SENTINEL)
    assert np.array_equal(got.cpu().numpy().view(np.int64), want)


@pytest.mark.parametrize("reader", [_read_download_res, _read_download_phi, _read_upload_phi, _read_upload_rhs,
                                    _read_apply_op, _read_fmg, _read_partial_cycle, _read_subtract_mean,
                                    _read_smooth_boxes, _read_one_substep, _read_get_dense],
                         ids=lambda f: f.__name__[6:])
def test_reader_after_two_cycles(reader):
    dev, orc = _pair(ARGS, 2, 2)
    _cycles(dev, orc, 2)
    reader(dev, orc)
    _assert_same(dev, orc)
    _cycles(dev, orc, 2)
    _assert_same(dev, orc)


# 3. other smoothing counts.  (4, 4): the up-smoothing's second pass writes
# the buffer the residual read, so the first cycle stores the res before it
# (one `residual` launch) and the level's cycles store at once from then on
@pytest.mark.parametrize("down,up", [(3, 1), (1, 3), (4, 4), (0, 2)])
def test_other_counts_back_to_back(down, up):
    dev, orc = _pair(ARGS, down, up)
    with _Count(dev) as k:
        _cycles(dev, orc, 3)
        first = k.n()
    _assert_same(dev, orc)
    if (down, up) == (4, 4):
        assert first == 1
        with _Count(dev) as k:
            _cycles(dev, orc, 3)
            assert k.n() == 0
        _assert_same(dev, orc)


# 4. Helmholtz with the mean subtracted
def test_helmholtz_subtract_mean_back_to_back():
    dev, orc = _pair(HELM, 2, 2, subtract_mean=True)
    _cycles(dev, orc, 3)
    _assert_same(dev, orc)


# 5. physical faces: the down-smoothing ends in k_smooth_resid, which stores
def test_dirichlet_never_pends():
    dev, orc = _pair(DIRICHLET, 2, 2)
    with _Count(dev) as k:
        _cycles(dev, orc, 2)
        _assert_same(dev, orc)
        assert k.n() == 0


# 6. the store is really skipped, and stored once when somebody reads
def test_one_storing_launch_per_read(monkeypatch):
    # (either level bound: k_gsrb4 down, then the plain unfused k_resid_restrict)
    dev, orc = _pair(ARGS, 2, 2)
    top = dev.levels()[-1]
    _cycles(dev, orc, 3)
    with _Count(dev) as k:
        _cycles(dev, orc, 3)
        assert k.n() == 0
        dev.get_level(top, IRES)
        assert k.n() == 1
        dev.get_level(top, IRES)
        assert k.n() == 1
    _assert_same(dev, orc)
    # OMG_NO_RES_PEND=1: every cycle stores, a download launches nothing, the same bits
    dev, orc = _pair(ARGS, 2, 2)
    monkeypatch.setenv("OMG_NO_RES_PEND", "1")
    ref = DeviceBackend(parse(ARGS))
    ref.mg.n_cycle_down, ref.mg.n_cycle_up = 2, 2
    ref.mg._push_methods()
    setup_problem(ref)
    with _Count(ref) as k:
        for _ in range(3):
            dev.vcycle(False)
            ref.vcycle(False)
            _assert_same(dev, ref)
        ref.get_level(top, IRES)
        assert k.n() == 0


# 7. captured cycles (OMG_GRAPH=1) leave nothing pending: Dirichlet, as the
# graph tests of the other files, and the periodic Helmholtz problem without a
# subtracted mean, whose direct cycles do leave the res pending
@pytest.mark.parametrize("args", [DIRICHLET, HELM])
def test_graph_cycles_leave_nothing_pending(monkeypatch, args):
    monkeypatch.setenv("OMG_GRAPH", "1")
    dev, orc = _pair(args, 2, 2, subtract_mean=False)
    _cycles(dev, orc, 2)
    top = dev.levels()[-1]
    with _Count(dev) as k:
        dev.get_level(top, IRES)
        assert k.n() == 0
    _assert_same(dev, orc)
    assert dev.vcycle(True) == orc.vcycle(True)
    _assert_same(dev, orc)
