#!/usr/bin/env python3
"""Dense device I/O against the host path it replaces, on one MI355X.

For C3's tree (512^3, box 16, periodic, level 1) and C2's (256^3):

* omg_put_dense / omg_get_dense of one variable of level 1, the row kernel and
  the per-cell kernel (OMG_DENSE_GENERIC=1) in alternating rounds of one
  process, timed by HIP events on the library's stream (omg_kernel_stats);
* the wall time of omg_upload_level + omg_download_level of the same variable
  (what a caller pays without the dense entries);
* one stand-alone V-cycle.

Bytes are computed from the shapes at 16 B per cell (8 B read + 8 B written);
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
IRHS, IRES = 2, 4


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
    gbs = 16.0 * cells / (ms * 1e-3) / 1e9
    return {"GB_per_s": round(gbs, 1), "share_of_8TBps": round(gbs * 1e9 / HBM_BYTES_PER_S, 4)}


def timed(mg, name, call, reps):
    """`reps` calls between two reads of the family's event time (ms per call)."""
    mg.ctx.call("reset_stats")
    for _ in range(reps):
        call()
    n, ms, _ = mg.ctx.kernel_stats(name)
    assert n == reps, (name, n, reps)
    return ms / reps


def alternating(mg, torch, src, dst, env, values, rounds, reps):
    """rounds x values: put and get with os.environ[env] = value, in turn."""
    out = {v: {"put": [], "get": []} for v in values}
    for _ in range(rounds):
        for v in values:
            os.environ[env] = v
            out[v]["put"].append(timed(mg, "dense_put", lambda: mg.set_dense(1, IRES, src), reps))
            out[v]["get"].append(timed(mg, "dense_get", lambda: mg.get_dense(1, IRES, out=dst), reps))
    os.environ.pop(env, None)
    torch.cuda.synchronize()
    return out


def measure(omg, torch, name, n, rounds, reps):
    mg = build(omg, n)
    ctx = mg.ctx
    cells = n ** 3
    src = torch.rand((n, n, n), dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    # correctness of what is timed: a round trip through each kernel returns the bits
    for generic in ("0", "1"):
        os.environ["OMG_DENSE_GENERIC"] = generic
        dst.zero_()
        assert mg.set_dense(1, IRES, src) == cells
        assert mg.get_dense(1, IRES, out=dst)[1] == cells
        assert bool((dst.view(torch.int64) == src.view(torch.int64)).all()), f"round trip differs (generic={generic})"
    os.environ.pop("OMG_DENSE_GENERIC", None)
    ctx.call("set_profiling", 1)
    for _ in range(3):   # warm-up of every shape and kernel the timed rounds use
        for generic in ("0", "1"):
            os.environ["OMG_DENSE_GENERIC"] = generic
            mg.set_dense(1, IRES, src)
            mg.get_dense(1, IRES, out=dst)
    os.environ.pop("OMG_DENSE_GENERIC", None)
    ctx.call("synchronize")

    ab = alternating(mg, torch, src, dst, "OMG_DENSE_GENERIC", ("0", "1"), rounds, reps)
    ctx.call("set_profiling", 0)
    res = {"tree": f"{name}: {n}^3, box {BOX}, periodic, level 1", "cells": cells, "bytes_per_call": 16 * cells,
           "rounds": rounds, "calls_per_round": reps}
    for key, v in (("row", "0"), ("generic", "1")):
        res[key] = {d: {**summary(ab[v][d]), **rate(cells, statistics.median(ab[v][d]))} for d in ("put", "get")}
    res["row_faster_than_generic"] = {d: max(ab["0"][d]) < min(ab["1"][d]) for d in ("put", "get")}

    # the host path: upload + download of the same variable (wall time, pageable numpy arrays)
    nb, nc = ctx.level_size(1)
    host = np.random.default_rng(1).standard_normal((nb, nc + 2, nc + 2, nc + 2))
    mg.set_level(1, IRES, host)   # (warm-up: the staging buffer)
    mg.get_level(1, IRES)
    walls = []
    for _ in range(3):
        ctx.call("synchronize")
        t0 = time.perf_counter()
        mg.set_level(1, IRES, host)
        mg.get_level(1, IRES)
        walls.append((time.perf_counter() - t0) * 1e3)
    res["upload_plus_download_wall_ms"] = summary(walls)
    del host

    # put + get as a caller sees them: wall time of the pair, ending in a synchronise
    pair = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        ctx.call("synchronize")
        t0 = time.perf_counter()
        mg.set_dense(1, IRES, src)
        mg.get_dense(1, IRES, out=dst)
        torch.cuda.synchronize()
        pair.append((time.perf_counter() - t0) * 1e3)
    res["put_plus_get_wall_ms"] = summary(pair)

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
    io = res["row"]["put"]["median_ms"] + res["row"]["get"]["median_ms"]
    res["put_plus_get_event_ms"] = round(io, 4)
    res["put_plus_get_over_vcycle"] = round(io / res["vcycle_wall_ms"]["median_ms"], 4)
    res["upload_download_over_put_get"] = round(res["upload_plus_download_wall_ms"]["median_ms"] /
                                                res["put_plus_get_wall_ms"]["median_ms"], 1)
    ctx.call("synchronize")
    omg.mg_deallocate_storage(mg)
    del src, dst, rhs
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trees", default="C3,C2", help="comma-separated: C3 (512^3), C2 (256^3)")
    ap.add_argument("--rounds", type=int, default=20, help="alternating rounds of (row, generic)")
    ap.add_argument("--reps", type=int, default=5, help="calls per round and direction")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("dense_io_bench: no GPU (the tool measures on the device or not at all)")
    omg = __graft_entry__.load_package()
    out = {"tool": "dense_io_bench", "device": torch.cuda.get_device_name(0), "timing": "HIP events on the library stream"}
    for name in a.trees.split(","):
        out[name] = measure(omg, torch, name, TREES[name], a.rounds, a.reps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
