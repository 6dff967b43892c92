"""Problem runner of the free-space tests: replays oracle/omg_free_golden.f90
(the reference's tests/test_free_space.f90 set-up) on

* ``device`` — the product: octree_mg_amd.MG + free_space.mg_poisson_free_3d
  driving libomg.so (Green's function, hipFFT solve, boundary table, FMG) on
  the GPU, one rank or several through the loopback transport;
* ``oracle`` — the checker: the C restatement of the multigrid
  (oracle/liboracle.so) with oracle/free_space_oracle.py's direct-convolution
  restatement of PSolver.

Both start from the same inputs.  The Green's-function solve sums in another
order on each (and in the reference), so results agree at round-off, which
the tests state as tolerances (see tolerances()).
"""
from __future__ import annotations

import math
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import __graft_entry__  # noqa: E402

omg = __graft_entry__.load_package()
T = omg.tree

I_SOL = 5

# The problems of oracle/omg_free_golden.f90 (its 9th argument), as
# (charges [(amplitude, sigma, position)], r_min).  c is the reference's
# tests/test_free_space.f90:9-13; a has three off-centre charges of both signs
# that no axis flip or permutation maps onto themselves; b is a with the
# domain's origin moved (every component different and non-zero), the charges
# moved with it.
_CHARGES_A = [(0.6, 0.08, (0.30, 0.55, 0.62)), (-0.35, 0.10, (0.66, 0.34, 0.45)),
              (0.25, 0.07, (0.45, 0.70, 0.30))]
_R_MIN_B = (-0.25, 0.5, 1.0)
LAYOUTS = {
    "c": ([(1.0, 0.1, (0.5, 0.5, 0.5))], (0.0, 0.0, 0.0)),
    "a": (_CHARGES_A, (0.0, 0.0, 0.0)),
    "b": ([(a, s, tuple(np.array(r) + np.array(_R_MIN_B))) for a, s, r in _CHARGES_A], _R_MIN_B),
}


def parse(args: str) -> dict:
    """A golden entry's args: box nx ny nz n_its fft_frac cycle [layout]."""
    f = args.split()
    layout = f[7] if len(f) > 7 else "c"
    if layout not in LAYOUTS:
        raise ValueError("unknown charge layout %r" % layout)
    return dict(box=int(f[0]), domain=[int(f[1]), int(f[2]), int(f[3])], n_its=int(f[4]),
                frac=float(f[5]), cycle=f[6], layout=layout)


def driver_argv(args: str, dump=None):
    """The command line of oracle/omg_free_golden.f90 (and of the drop-in's
    build of it) for a golden entry's args: the dump file, or x, goes
    between the cycle and the optional layout."""
    f = args.split()
    return f[:7] + [dump or "x"] + f[7:]


def build_tree(cfg, tree, n_ranks=1, my_rank=0):
    tree.smoother_type = T.MG_SMOOTHER_GSRB
    tree.n_cpu, tree.my_rank = n_ranks, my_rank
    dom = np.array(cfg["domain"], dtype=np.int64)
    r_min = list(LAYOUTS[cfg.get("layout", "c")][1])
    tree.build_rectangle(dom, cfg["box"], 1.0 / dom.astype(np.float64), r_min, [False] * 3, 0)
    tree.load_balance()
    return tree


def _erf(x):
    return np.vectorize(math.erf, otypes=[np.float64])(x)


def level_fields(tree, lvl, ids, layout="c"):
    """rhs and solution of test_free_space (:127-165) on boxes ids, as
    [box, k, j, i] arrays of (nc+2)^3 with zero ghosts: the sum over the
    layout's charges, accumulated from 0 in their order as the driver does."""
    charges = LAYOUTS[layout][0]
    nc = tree.box_size_lvl[lvl]
    dr = np.asarray(tree.dr[lvl])
    rhs = np.zeros((len(ids), nc + 2, nc + 2, nc + 2))
    sol = np.zeros_like(rhs)
    c = np.arange(1, nc + 1) - 0.5
    pi = math.acos(-1.0)
    for n, id_ in enumerate(ids):
        r0 = tree.box_r_min[id_]
        x = r0[0] + c * dr[0]
        y = r0[1] + c * dr[1]
        z = r0[2] + c * dr[2]
        Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
        fac = 1.0 / (4.0 * pi)
        rhs_sum = np.zeros(X.shape)
        sol_sum = np.zeros(X.shape)
        for ampl, sigma, r0c in charges:
            s2 = ((X - r0c[0]) / sigma) ** 2 + ((Y - r0c[1]) / sigma) ** 2 + ((Z - r0c[2]) / sigma) ** 2
            rhs_sum = rhs_sum + -ampl / (sigma ** 3 * pi * math.sqrt(pi)) * np.exp(-s2)
            rn = np.sqrt((X - r0c[0]) ** 2 + (Y - r0c[1]) ** 2 + (Z - r0c[2]) ** 2)
            with np.errstate(divide="ignore", invalid="ignore"):
                v = fac * ampl * _erf(rn / sigma) / rn
            v = np.where(rn < math.sqrt(np.finfo(np.float64).eps),
                         2.0 * fac * ampl / (math.sqrt(pi) * sigma), v)
            sol_sum = sol_sum + v
        rhs[n, 1:-1, 1:-1, 1:-1] = rhs_sum
        sol[n, 1:-1, 1:-1, 1:-1] = sol_sum
    return rhs, sol


def _errors(tree, phi, sol):
    """print_error (:167-195): max |phi - sol| and the squared-error sum over
    the highest level (this rank's boxes)."""
    d = np.abs(phi[:, 1:-1, 1:-1, 1:-1] - sol[:, 1:-1, 1:-1, 1:-1])
    return float(d.max()) if d.size else 0.0, float(np.sum(d ** 2))


def _history_entry(it, e, e2sum, n_unknowns, mres):
    return {"it": it, "err": e, "err2": math.sqrt(e2sum / n_unknowns), "max_res": mres}


def _box_errors(phi, sol):
    """print_error's two sums per box: (max |phi - sol|, sum (phi - sol)^2)
    over each box's interior, arrays over the boxes."""
    d = np.abs(phi[:, 1:-1, 1:-1, 1:-1] - sol[:, 1:-1, 1:-1, 1:-1]).reshape(len(phi), -1)
    return d.max(axis=1), np.sum(d ** 2, axis=1)


def stored_mask(nc):
    """Interior + face ghosts of a (nc+2)^3 box: the cells the reference
    reads and the device stores (edge and corner ghosts are neither)."""
    ix = np.arange(nc + 2)
    bnd = ((ix == 0) | (ix == nc + 1)).astype(int)
    return (bnd[:, None, None] + bnd[None, :, None] + bnd[None, None, :]) < 2


def split_planes(nx, flat):
    """omg_free_planes' buffer (include/omg.h: bc_x0, bc_x1 of nx2*nx3, bc_y0,
    bc_y1 of nx1*nx3, bc_z0, bc_z1 of nx1*nx2, first index fastest) as six
    flat arrays."""
    n1, n2, n3 = (int(v) for v in nx)
    out, pos = [], 0
    for s in (n2 * n3, n2 * n3, n1 * n3, n1 * n3, n1 * n2, n1 * n2):
        out.append(np.array(flat[pos:pos + s]))
        pos += s
    assert pos == len(flat)
    return out


def device_planes(mg):
    """(fft_lvl, nx, six flat planes) from omg_free_planes."""
    import ctypes as C
    lvl, nx = C.c_int(0), np.zeros(3, np.int32)
    mg.ctx.call("free_planes", C.byref(lvl), nx, None, 0)
    n1, n2, n3 = (int(v) for v in nx)
    flat = np.full(2 * (n2 * n3 + n1 * n3 + n1 * n2), np.nan)
    mg.ctx.call("free_planes", C.byref(lvl), nx, flat.ctypes.data_as(C.c_void_p), flat.size)
    return lvl.value, [n1, n2, n3], split_planes(nx, flat)


def run_oracle(args: str):
    """The configuration on the CPU oracle; returns history and the final
    phi of the highest level [box, k, j, i] (ids order), and per stage:
    fft_lvl, nx and planes (the six boundary planes, flat in omg_free_planes'
    order), phi_fft_1 (phi of the FFT level after iteration 1, with ghosts),
    phi_lvls (the final phi of every level) and box_err (per iteration the
    (max, sum of squares) error arrays over the highest level's boxes)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import free_space_oracle as F   # checker only
    import pyoracle
    cfg = parse(args)
    tree = build_tree(cfg, T.MGTree())
    o = pyoracle.Oracle(tree, I_SOL)
    o.configure(op=pyoracle.LAPLACIAN, smoother=pyoracle.GSRB)
    for lvl in range(tree.lowest_lvl, tree.highest_lvl + 1):
        rhs, sol = level_fields(tree, lvl, tree.lvls[lvl].ids, cfg["layout"])
        o.set_level(lvl, T.MG_IRHS, rhs)
        o.set_level(lvl, I_SOL, sol)
    S = F.FreeState()
    hl = tree.highest_lvl
    sol_h = o.get_level(hl, I_SOL)
    hist, box_err, phi_fft_1 = [], [], None
    for n in range(1, cfg["n_its"] + 1):
        m = F.poisson_free_3d(o, tree, S, n == 1, cfg["frac"], cfg["cycle"] == "f", True)
        phi = o.get_level(hl, T.MG_IPHI)
        e, e2 = _errors(tree, phi, sol_h)
        hist.append(_history_entry(n, e, e2, tree.number_of_unknowns(), m))
        box_err.append(_box_errors(phi, sol_h))
        if n == 1:
            phi_fft_1 = o.get_level(S.fft_lvl, T.MG_IPHI)
    nx = [S.planes[2].shape[1], S.planes[0].shape[1], S.planes[0].shape[0]]
    return {"history": hist, "phi": o.get_level(hl, T.MG_IPHI), "tree": tree,
            "fft_lvl": S.fft_lvl, "nx": nx, "planes": [np.ascontiguousarray(P).reshape(-1) for P in S.planes],
            "planes_2d": S.planes, "phi_fft_1": phi_fft_1, "box_err": box_err,
            "phi_lvls": {l: o.get_level(l, T.MG_IPHI) for l in range(tree.lowest_lvl, hl + 1)}}


class _Device:
    def __init__(self, cfg, comm=None, rep_cells=0):
        mg = omg.MG()
        mg.coarse_replication_cells = rep_cells
        mg.n_extra_vars = 1
        mg.operator_type = T.MG_LAPLACIAN
        mg.smoother_type = T.MG_SMOOTHER_GSRB
        omg.mg_set_methods(mg)
        omg.mg_comm_init(mg, comm)
        build_tree(cfg, mg, mg.n_cpu, mg.my_rank)
        omg.mg_allocate_storage(mg)
        self.mg = mg
        rep = mg.ctx.replicated_level()
        for lvl in range(mg.lowest_lvl, mg.highest_lvl + 1):
            ids = mg.lvls[lvl].my_ids
            if len(ids) or lvl <= rep:
                rhs, sol = level_fields(mg, lvl, ids, cfg["layout"])
                mg.set_level(lvl, T.MG_IRHS, rhs)
                mg.set_level(lvl, I_SOL, sol)
        hl = mg.highest_lvl
        self.sol_h = mg.get_level(hl, I_SOL) if len(mg.lvls[hl].my_ids) else None

    def step(self, cfg, n):
        return omg.mg_poisson_free_3d(self.mg, n == 1, cfg["frac"], cfg["cycle"] == "f", max_res=True)

    def errors(self):
        hl = self.mg.highest_lvl
        if self.sol_h is None:
            return 0.0, 0.0
        return _errors(self.mg, self.mg.get_level(hl, T.MG_IPHI), self.sol_h)


def run_device(args: str):
    """The configuration on one GPU rank."""
    cfg = parse(args)
    d = _Device(cfg)
    hist = []
    for n in range(1, cfg["n_its"] + 1):
        m = d.step(cfg, n)
        e, e2 = d.errors()
        hist.append(_history_entry(n, e, e2, d.mg.number_of_unknowns(), m))
    out = {"history": hist, "phi": d.mg.get_level(d.mg.highest_lvl, T.MG_IPHI), "mg": d.mg}
    return out


def run_device_loopback(args: str, n_ranks: int, timeout=600, rep_cells=0):
    """n_ranks device contexts of this process (one thread each, loopback
    transport, all on GPU 0); err by max and the squared errors summed over
    ranks, as print_error's MPI_Allreduce.  Besides that reduced history,
    "ranks" holds what each rank had before any reduction: errs (its own
    (max err, sum err^2) per iteration), fft_lvl, nx and planes
    (omg_free_planes after iteration 1), fft_ids and phi_fft_1 (its boxes of
    the FFT level and their phi after iteration 1), hl_ids and phi_hl (its
    boxes of the highest level and their final phi); phi with ghosts."""
    cfg = parse(args)
    tag = int.from_bytes(os.urandom(6), "little")
    bar = threading.Barrier(n_ranks)
    slots = [None] * n_ranks
    hists = [None] * n_ranks
    per_rank = [None] * n_ranks
    errors = []

    def worker(rank):
        try:
            d = _Device(cfg, omg.Loopback(tag, rank, n_ranks), rep_cells)
            hist = []
            mine = per_rank[rank] = {"errs": []}
            for n in range(1, cfg["n_its"] + 1):
                m = d.step(cfg, n)
                slots[rank] = d.errors()
                mine["errs"].append(slots[rank])
                if n == 1:
                    mine["fft_lvl"], mine["nx"], mine["planes"] = device_planes(d.mg)
                    mine["fft_ids"] = [int(i) for i in d.mg.lvls[mine["fft_lvl"]].my_ids]
                    mine["phi_fft_1"] = d.mg.get_level(mine["fft_lvl"], T.MG_IPHI) if mine["fft_ids"] else None
                bar.wait()
                e = max(s[0] for s in slots)
                e2 = sum(s[1] for s in slots)
                bar.wait()
                hist.append(_history_entry(n, e, e2, d.mg.number_of_unknowns(), m))
            hists[rank] = hist
            hl = d.mg.highest_lvl
            mine["hl_ids"] = [int(i) for i in d.mg.lvls[hl].my_ids]
            mine["phi_hl"] = d.mg.get_level(hl, T.MG_IPHI) if mine["hl_ids"] else None
            d.mg.ctx.call("synchronize")
            omg.mg_deallocate_storage(d.mg)
        except BaseException as ex:  # noqa: BLE001  (re-raised below)
            errors.append((rank, ex))
            bar.abort()

    th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(n_ranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout)
    if errors:
        real = [(r, e) for r, e in errors if not isinstance(e, threading.BrokenBarrierError)]
        r, e = (real or errors)[0]
        raise RuntimeError(f"rank {r}: {type(e).__name__}: {e}")
    if any(t.is_alive() for t in th):
        raise TimeoutError("loopback run did not finish")
    return {"history": hists[0], "all": hists, "ranks": per_rank}


def golden_history(entry, ranks=1):
    """The reference's history of a free_golden.json entry as floats."""
    import struct
    f = lambda h: struct.unpack(">d", bytes.fromhex(h))[0]
    return [{"it": h["it"], "err": f(h["err"]), "err2": f(h["err2"]), "max_res": f(h["max_res"])}
            for h in entry["runs"][str(ranks)]["history"]]


def tolerances(cfg):
    """Agreement stated for free-space results.  The Green's-function solve
    is exact up to summation order, so phi agrees to a few ulps of its scale
    (max |phi| < 1); errors against the analytic solution (~1e-3) inherit
    that absolutely; residuals are second differences of phi, so a phi
    difference of delta moves them by up to delta * 2*sum(1/dr^2)."""
    dr = 1.0 / np.asarray(cfg["domain"], dtype=np.float64)
    op_norm = 2.0 * float(np.sum(1.0 / dr ** 2))
    phi_abs = 2e-14
    return {"phi_abs": phi_abs, "err_abs": phi_abs, "res_abs": 4 * phi_abs * op_norm}


def compare_history(got, ref, cfg, what=""):
    tol = tolerances(cfg)
    assert len(got) == len(ref), (what, len(got), len(ref))
    # the worst deviation in units of its tolerance (shown by pytest -s, and with a failure)
    print("compare_history", what, "worst deviation/tolerance:",
          max([0.0] + [abs(g[k] - r[k]) / tol[t] for g, r in zip(got, ref)
                       for k, t in (("err", "err_abs"), ("err2", "err_abs"), ("max_res", "res_abs"))]))
    for g, r in zip(got, ref):
        assert abs(g["err"] - r["err"]) <= tol["err_abs"], (what, g, r)
        assert abs(g["err2"] - r["err2"]) <= tol["err_abs"], (what, g, r)
        assert abs(g["max_res"] - r["max_res"]) <= tol["res_abs"], (what, g, r)
