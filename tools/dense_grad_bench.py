#!/usr/bin/env python3
"""omg_get_dense_grad on one MI355X: the tile kernel against the per-cell
kernel, and against what a caller had before the entry.

For C3's tree (512^3, box 16, periodic, level 1) and C2's (256^3):

* omg_get_dense_grad of phi (all three components, ghosts already filled), the
  tile kernel and the per-cell kernel (OMG_DENSE_GENERIC=1) in alternating
  rounds of one process, timed by HIP events on the library's stream
  (omg_kernel_stats, family dense_grad);
* the composition it replaces: omg_get_dense of phi, then three torch central
  differences on the interior of the dense array (no boundary values at all:
  the comparison is of time only), timed by events on torch's stream;
* one stand-alone V-cycle.

Bytes are computed from the shapes at 32 B per cell (8 B read + 24 B written);
"share" is that traffic over 8 TB/s.  One JSON line on stdout.  No GPU, no
result: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
TREES = {"C3": 512, "C2": 256}
BOX = 16
IPHI, IRHS = 1, 2
ENV = "OMG_DENSE_GENERIC"


def build(omg, n):
    T = omg.tree
    mg = omg.MG()
    mg.operator_type = T.MG_LAPLACIAN
    mg.smoother_type = T.MG_SMOOTHER_GSRB
    omg.mg_set_methods(mg)
    omg.mg_comm_init(mg)
    dom = np.array([n, n, n])
    omg.mg_build_rectangle(mg, dom, BOX, 1.0 / dom.astype(np.float64), [0.0] * 3, [True] * 3, 0)
    omg.mg_load_balance(mg)
    omg.mg_set_methods(mg)
    omg.mg_allocate_storage(mg, device_index=0)
    return mg


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def rate(cells, ms):
    gbs = 32.0 * cells / (ms * 1e-3) / 1e9
    return {"GB_per_s": round(gbs, 1), "share_of_8TBps": round(gbs * 1e9 / HBM_BYTES_PER_S, 4)}


def timed(mg, call, reps):
    """`reps` calls between two reads of the family's event time (ms per call)."""
    mg.ctx.call("reset_stats")
    for _ in range(reps):
        call()
    n, ms, _ = mg.ctx.kernel_stats("dense_grad")
    assert n == reps, (n, reps)
    return ms / reps


def composition(mg, torch, phi, f):
    """omg_get_dense, then the three central differences of the interior."""
    mg.get_dense(1, IPHI, out=phi)
    gx = (phi[:, :, 2:] - phi[:, :, :-2]) * f[0]
    gy = (phi[:, 2:, :] - phi[:, :-2, :]) * f[1]
    gz = (phi[2:, :, :] - phi[:-2, :, :]) * f[2]
    return gx, gy, gz


def measure(omg, torch, name, n, rounds, reps):
    mg = build(omg, n)
    ctx = mg.ctx
    cells = n ** 3
    src = torch.rand((n, n, n), dtype=torch.float64, device="cuda")
    assert mg.set_dense(1, IPHI, src) == cells
    omg.mg_fill_ghost_cells_lvl(mg, 1, IPHI)
    out = torch.empty((3, n, n, n), dtype=torch.float64, device="cuda")
    # correctness of what is timed: both kernels give the same bits, and in the
    # interior those of the composition
    os.environ[ENV] = "1"
    ref = torch.empty_like(out)
    assert mg.get_dense_grad(1, out=ref, scale=-1.0)[1] == cells
    os.environ[ENV] = "0"
    assert mg.get_dense_grad(1, out=out, scale=-1.0)[1] == cells
    assert bool((out.view(torch.int64) == ref.view(torch.int64)).all()), "tile and per-cell kernels differ"
    f = [(0.5 * -1.0) / float(d) for d in mg.dr[1]]
    gx, gy, gz = composition(mg, torch, src.clone(), f)
    assert bool((gx.view(torch.int64) == out[0][:, :, 1:-1].view(torch.int64)).all())
    assert bool((gy.view(torch.int64) == out[1][:, 1:-1, :].view(torch.int64)).all())
    assert bool((gz.view(torch.int64) == out[2][1:-1, :, :].view(torch.int64)).all())
    del ref, gx, gy, gz
    ctx.call("set_profiling", 1)
    for _ in range(3):   # warm-up of every shape and kernel the timed rounds use
        for generic in ("0", "1"):
            os.environ[ENV] = generic
            mg.get_dense_grad(1, out=out, scale=-1.0)
    ctx.call("synchronize")

    ab = {"0": [], "1": []}
    for _ in range(rounds):
        for v in ("0", "1"):
            os.environ[ENV] = v
            ab[v].append(timed(mg, lambda: mg.get_dense_grad(1, out=out, scale=-1.0), reps))
    os.environ.pop(ENV, None)
    torch.cuda.synchronize()
    ctx.call("set_profiling", 0)
    res = {"tree": f"{name}: {n}^3, box {BOX}, periodic, level 1", "cells": cells, "bytes_per_call": 32 * cells,
           "rounds": rounds, "calls_per_round": reps}
    for key, v in (("tile", "0"), ("generic", "1")):
        res[key] = {**summary(ab[v]), **rate(cells, statistics.median(ab[v]))}
    res["tile_faster_than_generic_beyond_spread"] = max(ab["0"]) < min(ab["1"])

    # what the parent offers: get_dense + three torch differences (events on torch's stream)
    phi = torch.empty_like(src)
    for _ in range(3):
        composition(mg, torch, phi, f)
    comp = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            composition(mg, torch, phi, f)
        e1.record()
        torch.cuda.synchronize()
        comp.append(e0.elapsed_time(e1) / reps)
    res["get_dense_plus_torch_differences"] = summary(comp)
    res["composition_over_tile"] = round(statistics.median(comp) / res["tile"]["median_ms"], 2)

    # the call as a caller sees it: wall time ending in a synchronise
    wall = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        ctx.call("synchronize")
        t0 = time.perf_counter()
        mg.get_dense_grad(1, out=out, scale=-1.0)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["call_wall_ms"] = summary(wall)

    # one stand-alone V-cycle of the tree (rhs = a zero-mean random field)
    rhs = torch.rand((n, n, n), dtype=torch.float64, device="cuda") - 0.5
    mg.set_dense(1, IRHS, rhs)
    for _ in range(3):
        omg.mg_fas_vcycle(mg)
    cyc = []
    for _ in range(10):
        ctx.call("synchronize")
        t0 = time.perf_counter()
        omg.mg_fas_vcycle(mg)
        ctx.call("synchronize")
        cyc.append((time.perf_counter() - t0) * 1e3)
    res["vcycle_wall_ms"] = summary(cyc)
    res["tile_over_vcycle"] = round(res["tile"]["median_ms"] / res["vcycle_wall_ms"]["median_ms"], 4)
    ctx.call("synchronize")
    omg.mg_deallocate_storage(mg)
    del src, out, phi, rhs
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trees", default="C3,C2", help="comma-separated: C3 (512^3), C2 (256^3)")
    ap.add_argument("--rounds", type=int, default=20, help="alternating rounds of (tile, generic)")
    ap.add_argument("--reps", type=int, default=5, help="calls per round")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("dense_grad_bench: no GPU (the tool measures on the device or not at all)")
    omg = __graft_entry__.load_package()
    out = {"tool": "dense_grad_bench", "device": torch.cuda.get_device_name(0),
           "timing": "HIP events on the library stream"}
    for name in a.trees.split(","):
        out[name] = measure(omg, torch, name, TREES[name], a.rounds, a.reps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
