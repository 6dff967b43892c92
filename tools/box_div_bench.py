#!/usr/bin/env python3
"""omg_put_boxes_div on one MI355X against the path it replaces.

One tree (P320: 320^3 periodic, box 16, the 8000 boxes of level 1; P<n> for
another size) and lists of its first k boxes, k from short lists to the whole
level.  For every list and both centrings, from a pool [3, k, m, m, m] with
m = 16 + 2 * width (--width 1, one ghost layer: the layout of an AMR host)
into rhs:

* the new call through the tile kernel (OMG_BOXES_TILE=1), the per-cell kernel
  (OMG_BOXES_GENERIC=1) and the library's own routing, in alternating rounds
  of one process, timed twice: by the library's HIP events around its kernels
  (omg_kernel_stats, family boxes_div) and by events on the caller's stream
  around the call;
* the path it replaces on the same tree: the torch slice differences of the
  pools (one subtraction and one multiplication per component, two additions)
  into a scratch pool [k, 16, 16, 16], then MG.set_blocks of it, by events on
  the caller's stream, in the same rounds;
* the host time of a call with a cached list (wall time of 1000 calls of an
  8-box list queued without a wait, per call).

Before anything is timed, both kernels and the replaced path must leave the
same bits in rhs.  One JSON line on stdout.  No GPU, no result: there is no
fallback.
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

BOX = 16
IRHS = 2
VARIANTS = ("default", "tile", "generic")


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


def set_variant(v):
    for k in ("OMG_BOXES_GENERIC", "OMG_BOXES_TILE"):
        os.environ.pop(k, None)
    if v == "generic":
        os.environ["OMG_BOXES_GENERIC"] = "1"
    elif v == "tile":
        os.environ["OMG_BOXES_TILE"] = "1"


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def old_path(mg, torch, ids, pool, scratch, tmp, f, face, width):
    """What a host does today: its own differences of the component pools into
    a scratch pool, (t_x + t_y) + t_z, then the copy of that pool into rhs."""
    w = slice(width, width + BOX)
    for d in range(3):
        ax = 3 - d
        hi, lo = [slice(None), w, w, w], [slice(None), w, w, w]
        lo[ax] = slice(width - 1, width + BOX - 1)
        if not face:
            hi[ax] = slice(width + 1, width + BOX + 1)
        dst = scratch if d == 0 else tmp
        torch.sub(pool[d][tuple(hi)], pool[d][tuple(lo)], out=dst)
        dst.mul_(f[d])
        if d:
            scratch.add_(tmp)
    mg.set_blocks(IRHS, scratch, ids)


def stream_ms(torch, call, reps):
    """ms per call between two events on the caller's (torch's current) stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def family_ms(mg, call, reps):
    """ms per call of the library's events around the family boxes_div."""
    mg.ctx.call("reset_stats")
    for _ in range(reps):
        call()
    n, ms, _ = mg.ctx.kernel_stats("boxes_div")
    assert n == reps, (n, reps)
    return ms / reps


def measure(omg, torch, n_dom, counts, rounds, reps, width):
    mg = build(omg, n_dom)
    ctx = mg.ctx
    all_ids = [int(i) for i in mg.lvls[1].my_ids]
    dr = [float(v) for v in mg.dr[1]]
    scale = 1.0
    m = BOX + 2 * width
    res = {"tree": f"P{n_dom}: {n_dom}^3, box 16, periodic, the first k of the {len(all_ids)} boxes of level 1",
           "pool": "[3, k, m, m, m], m = %d, ghost width %d" % (m, width),
           "rounds": rounds, "calls_per_round": reps, "lists": {}}
    ctx.call("set_profiling", 1)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    for k in counts:
        ids = all_ids[:k]
        print(f"box_div_bench: {k} boxes", file=sys.stderr, flush=True)
        pool = torch.randn((3, k, m, m, m), dtype=torch.float64, device="cuda", generator=gen)
        scratch = torch.zeros((k, BOX, BOX, BOX), dtype=torch.float64, device="cuda")
        tmp = torch.zeros_like(scratch)
        got = torch.zeros_like(scratch)
        ref = torch.zeros_like(scratch)
        entry = {"boxes": k}
        for centering in ("cell", "face"):
            face = centering == "face"
            f = [(scale if face else 0.5 * scale) / dr[d] for d in range(3)]
            cells = k * BOX ** 3

            def new():
                return mg.set_blocks_div(IRHS, pool, ids, width, scale=scale, centering=centering)

            def old():
                old_path(mg, torch, ids, pool, scratch, tmp, f, face, width)

            # what is timed leaves the same bits in rhs
            old()
            mg.get_blocks(IRHS, ids, out=ref, fill=False)
            assert int((ref != 0).sum()) > 0.9 * cells
            for v in ("tile", "generic"):
                set_variant(v)
                mg.set_blocks(IRHS, tmp.zero_(), ids)
                assert new() == cells
                mg.get_blocks(IRHS, ids, out=got, fill=False)
                assert bool((got.view(torch.int64) == ref.view(torch.int64)).all()), (k, centering, v)
            for _ in range(2):   # warm-up of every kernel and list of the timed rounds
                for v in VARIANTS:
                    set_variant(v)
                    new()
                old()
            torch.cuda.synchronize()
            fam = {v: [] for v in VARIANTS}
            strm = {v: [] for v in VARIANTS}
            repl = []
            for _ in range(rounds):
                for v in VARIANTS:
                    set_variant(v)
                    fam[v].append(family_ms(mg, new, reps))
                    strm[v].append(stream_ms(torch, new, reps))
                set_variant(None)
                repl.append(stream_ms(torch, old, reps))
            set_variant(None)
            case = {"cells": cells,
                    "new_call_library_events": {v: summary(fam[v]) for v in VARIANTS},
                    "new_call_caller_stream": {v: summary(strm[v]) for v in VARIANTS},
                    "replaced_path_caller_stream": summary(repl),
                    "tile_faster_than_generic": max(fam["tile"]) < min(fam["generic"]),
                    "generic_faster_than_tile": max(fam["generic"]) < min(fam["tile"]),
                    "replaced_over_new_default": round(statistics.median(repl) / statistics.median(strm["default"]), 2),
                    "new_faster_than_replaced": max(strm["default"]) < min(repl),
                    "new_slower_than_replaced": min(strm["default"]) > max(repl)}
            entry[centering] = case
        res["lists"][str(k)] = entry
        del pool, scratch, tmp, got, ref
        torch.cuda.empty_cache()
    ctx.call("set_profiling", 0)

    # the host's share of a call with a cached list
    ids = all_ids[:8]
    pool = torch.zeros((3, 8, m, m, m), dtype=torch.float64, device="cuda")
    calls = 1000
    host = []
    for _ in range(5):
        mg.set_blocks_div(IRHS, pool, ids, width)
        torch.cuda.synchronize()
        before = ctx.host_sync_count()
        t0 = time.perf_counter()
        for _ in range(calls):
            mg.set_blocks_div(IRHS, pool, ids, width)
        host.append((time.perf_counter() - t0) * 1e6 / calls)
        assert ctx.host_sync_count() == before
        torch.cuda.synchronize()
    res["cached_list_host_us_per_call"] = {"median": round(statistics.median(host), 2), "min": round(min(host), 2),
                                           "max": round(max(host), 2), "calls": calls, "boxes": 8,
                                           "through": "MG.set_blocks_div (the Python binding included)"}
    ctx.call("synchronize")
    omg.mg_deallocate_storage(mg)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default="P320", help="P<n>: n^3 periodic, box 16 (P320: 8000 boxes)")
    ap.add_argument("--counts", default="128,256,512,1024,1536,2048,4096,8000", help="comma-separated list lengths")
    ap.add_argument("--width", type=int, default=1, help="ghost layers of the component pools (>= 1)")
    ap.add_argument("--rounds", type=int, default=15, help="alternating rounds over the variants and the old path")
    ap.add_argument("--reps", type=int, default=3, help="calls per round and variant")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("box_div_bench: no GPU (the tool measures on the device or not at all)")
    omg = __graft_entry__.load_package()
    out = {"tool": "box_div_bench", "device": torch.cuda.get_device_name(0),
           "timing": "HIP events: the library's around its kernels, torch's on the caller's stream"}
    out[a.tree] = measure(omg, torch, int(a.tree[1:]), [int(c) for c in a.counts.split(",")], a.rounds, a.reps,
                          a.width)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
