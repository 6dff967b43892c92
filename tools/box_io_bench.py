#!/usr/bin/env python3
"""Device block I/O (omg_put_boxes / omg_get_boxes) on one MI355X.

Two trees: C3 (512^3, box 16, periodic: the 32,768 boxes of level 1) and C4
(BASELINE's 128^3 with one refined level, box 16: the leaves of both levels in
one call).  For each, the block pool of an AMR code with 0, 1 and 2 ghost
layers of its own:

* put and get of the interiors, and get with the six face-ghost layers at
  widths 1 and 2, timed by HIP events on the library's stream
  (omg_kernel_stats) in alternating rounds of one process over the kernel
  variants: the library's own routing, the tile kernel (OMG_BOXES_TILE=1), the
  per-cell kernel (OMG_BOXES_GENERIC=1) and, where the blocks are off a 16-B
  boundary (width 1), the tile kernel's two variants for that case
  (OMG_BOXES_ODD=16 / 8);
* on C3, omg_put_dense / omg_get_dense of the same level in the same run: the
  same 16 B per cell, the yardstick;
* the wall time of omg_upload_level + omg_download_level of the same boxes
  (the path this replaces).

Bytes are computed from the shapes at 16 B per cell moved (8 B read + 8 B
written); "share" is that traffic over 8 TB/s.  One JSON line on stdout.  No
GPU, no result: there is no fallback.
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
BOX = 16
IRES = 4


def build(omg, name):
    """C3: 512^3 periodic, uniform.  C4: 128^3, the boxes of level 1 whose
    centre lies in the middle half of the domain refined once (the reference's
    tests/test_refinement.f90 tree)."""
    T = omg.tree
    mg = omg.MG()
    mg.operator_type = T.MG_LAPLACIAN
    mg.smoother_type = T.MG_SMOOTHER_GSRB
    omg.mg_set_methods(mg)
    omg.mg_comm_init(mg)
    n = {"C3": 512, "C2": 256, "C4": 128}[name] if name in ("C3", "C2", "C4") else int(name[1:])   # (P<n>: n^3)
    dom = np.array([n, n, n])
    dr = 1.0 / dom.astype(np.float64)
    if name != "C4":
        omg.mg_build_rectangle(mg, dom, BOX, dr, [0.0] * 3, [True] * 3, 0)
    else:
        omg.mg_build_rectangle(mg, dom, BOX, dr, [0.0] * 3, [False] * 3, 2 * int(np.prod(dom // BOX)) + 1000)
        for id_ in list(mg.lvls[1].ids):
            centre = mg.box_r_min[id_] + 0.5 * BOX * mg.box_dr[id_]
            if np.all((centre >= 0.25) & (centre <= 0.75)):
                omg.mg_add_children(mg, int(id_))
        mg.set_leaves_parents(1)
        mg.set_next_level_ids(1)
        mg.set_neighbors_lvl(2)
        mg.set_leaves_parents(2)
        mg.highest_lvl = 2
        for lvl in (1, 2):
            mg.set_refinement_boundaries(lvl)
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


def set_variant(v):
    """default: the library's own routing; tile / generic: one kernel for
    every box; odd8 / odd16: the tile kernel with that variant for blocks off
    a 16-B boundary."""
    for k in ("OMG_BOXES_GENERIC", "OMG_BOXES_TILE", "OMG_BOXES_ODD"):
        os.environ.pop(k, None)
    if v == "generic":
        os.environ["OMG_BOXES_GENERIC"] = "1"
    elif v in ("tile", "odd8", "odd16"):
        os.environ["OMG_BOXES_TILE"] = "1"
        if v != "tile":
            os.environ["OMG_BOXES_ODD"] = v[3:]


def measure(omg, torch, name, rounds, reps):
    mg = build(omg, name)
    ctx = mg.ctx
    lvls = [l for l in range(1, mg.highest_lvl + 1)]
    ids = [int(i) for l in lvls for i in mg.lvls[l].my_leaves]
    n = len(ids)
    res = {"tree": "C4: 128^3 + one refined level, box 16, the leaves of levels 1 and 2 in one call" if name == "C4"
           else f"{name}: {int(round((n * BOX ** 3) ** (1 / 3)))}^3, box 16, periodic, the boxes of level 1",
           "boxes": n, "rounds": rounds, "calls_per_round": reps, "cases": {}}
    ctx.call("set_profiling", 1)
    for width in (0, 1, 2):
        print(f"box_io_bench: {name}, pool ghost width {width}", file=sys.stderr, flush=True)
        m = BOX + 2 * width
        pool = torch.rand((n, m, m, m), dtype=torch.float64, device="cuda")
        back = torch.zeros_like(pool)
        odd = (pool.data_ptr() // 8 + width * (1 + m + m * m)) % 2 == 1 or m % 2 == 1
        variants = ("default", "tile", "generic") + (("odd16", "odd8") if odd else ())
        cases = [("put", False), ("get", False)] + ([("get", True)] if width else [])
        # correctness of what is timed: a round trip through each variant returns the bits
        for v in variants:
            set_variant(v)
            for ghosts in ([False, True] if width else [False]):
                back.zero_()
                cells = mg.set_blocks(IRES, pool, ids, ghost_width=width, ghosts=ghosts)
                assert mg.get_blocks(IRES, ids, out=back, ghost_width=width, ghosts=ghosts, fill=False)[1] == cells
                moved = back.view(torch.int64) != 0
                assert int(moved.sum()) == cells, (v, width, ghosts)
                assert bool((back.view(torch.int64)[moved] == pool.view(torch.int64)[moved]).all()), (v, width)
                del moved
        calls = {}
        for d, ghosts in cases:
            if d == "put":
                calls[(d, ghosts)] = lambda g=ghosts: mg.set_blocks(IRES, pool, ids, ghost_width=width, ghosts=g)
            else:
                calls[(d, ghosts)] = lambda g=ghosts: mg.get_blocks(IRES, ids, out=back, ghost_width=width,
                                                                    ghosts=g, fill=False)
        for _ in range(2):   # warm-up of every kernel and list the timed rounds use
            for v in variants:
                set_variant(v)
                for c in calls.values():
                    c()
        ctx.call("synchronize")
        ms = {v: {k: [] for k in calls} for v in variants}
        for _ in range(rounds):
            for v in variants:
                set_variant(v)
                for (d, ghosts), c in calls.items():
                    ms[v][(d, ghosts)].append(timed(mg, "boxes_" + d, c, reps))
        set_variant(None)
        for (d, ghosts) in calls:
            cells = n * (BOX ** 3 + (6 * BOX * BOX if ghosts else 0))
            key = f"width{width}_{d}" + ("_ghosts" if ghosts else "")
            entry = {"cells": cells, "bytes_per_call": 16 * cells, "blocks_off_16B": bool(odd)}
            for v in variants:
                entry[v] = {**summary(ms[v][(d, ghosts)]), **rate(cells, statistics.median(ms[v][(d, ghosts)]))}
            entry["tile_faster_than_generic"] = max(ms["tile"][(d, ghosts)]) < min(ms["generic"][(d, ghosts)])
            if odd:
                entry["odd16_faster_than_odd8"] = max(ms["odd16"][(d, ghosts)]) < min(ms["odd8"][(d, ghosts)])
                entry["odd8_faster_than_odd16"] = max(ms["odd8"][(d, ghosts)]) < min(ms["odd16"][(d, ghosts)])
            if ghosts:   # the cost of the ghosts against their share of extra cells, 1 + 6/nc
                plain = statistics.median(ms["tile"][("get", False)])
                entry["time_over_interior_only"] = round(statistics.median(ms["tile"][(d, ghosts)]) / plain, 4)
                entry["cells_over_interior_only"] = round(1 + 6 / BOX, 4)
            res["cases"][key] = entry
        del pool, back
        torch.cuda.empty_cache()

    if name != "C4":   # the dense entries on the same level, same run
        g = int(mg.domain_size_lvl[1][0])
        src = torch.rand((g, g, g), dtype=torch.float64, device="cuda")
        dst = torch.empty_like(src)
        for _ in range(2):
            mg.set_dense(1, IRES, src)
            mg.get_dense(1, IRES, out=dst)
        put = [timed(mg, "dense_put", lambda: mg.set_dense(1, IRES, src), reps) for _ in range(rounds)]
        get = [timed(mg, "dense_get", lambda: mg.get_dense(1, IRES, out=dst), reps) for _ in range(rounds)]
        res["dense"] = {"put": {**summary(put), **rate(g ** 3, statistics.median(put))},
                        "get": {**summary(get), **rate(g ** 3, statistics.median(get))}}
        del src, dst
        torch.cuda.empty_cache()
    ctx.call("set_profiling", 0)

    # the host path: upload + download of the levels that hold the boxes (wall time, pageable numpy arrays)
    host = {l: np.random.default_rng(l).standard_normal((ctx.level_size(l)[0],) + (BOX + 2,) * 3) for l in lvls}
    for l in lvls:   # (warm-up: the staging buffer)
        mg.set_level(l, IRES, host[l])
        mg.get_level(l, IRES)
    walls = []
    for _ in range(3):
        ctx.call("synchronize")
        t0 = time.perf_counter()
        for l in lvls:
            mg.set_level(l, IRES, host[l])
        for l in lvls:
            mg.get_level(l, IRES)
        walls.append((time.perf_counter() - t0) * 1e3)
    res["upload_plus_download_wall_ms"] = summary(walls)
    del host
    # put + get of the width-1 pool with ghosts as a caller sees them: wall time of the pair, ending in a synchronise
    pool = torch.rand((n, BOX + 2, BOX + 2, BOX + 2), dtype=torch.float64, device="cuda")
    pair = []
    for _ in range(rounds + 2):
        torch.cuda.synchronize()
        ctx.call("synchronize")
        t0 = time.perf_counter()
        mg.set_blocks(IRES, pool, ids, ghost_width=1, ghosts=True)
        mg.get_blocks(IRES, ids, out=pool, ghost_width=1, ghosts=True, fill=False)
        torch.cuda.synchronize()
        pair.append((time.perf_counter() - t0) * 1e3)
    res["put_plus_get_ghosts_wall_ms"] = summary(pair[2:])
    res["upload_download_over_put_get"] = round(res["upload_plus_download_wall_ms"]["median_ms"] /
                                                res["put_plus_get_ghosts_wall_ms"]["median_ms"], 1)
    ctx.call("synchronize")
    omg.mg_deallocate_storage(mg)
    del pool
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trees", default="C3,C4",
                    help="comma-separated: C3 (512^3), C2 (256^3), C4 (128^3 + one refined level), P<n> (n^3, periodic)")
    ap.add_argument("--rounds", type=int, default=15, help="alternating rounds over the kernel variants")
    ap.add_argument("--reps", type=int, default=3, help="calls per round, case and variant")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("box_io_bench: no GPU (the tool measures on the device or not at all)")
    omg = __graft_entry__.load_package()
    out = {"tool": "box_io_bench", "device": torch.cuda.get_device_name(0), "timing": "HIP events on the library stream"}
    for name in a.trees.split(","):
        out[name] = measure(omg, torch, name, a.rounds, a.reps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
