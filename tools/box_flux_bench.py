#!/usr/bin/env python3
"""omg_get_boxes_flux on one MI355X against the path it replaces.

One tree (P320: 320^3 periodic, box 16, the 8000 boxes of level 1; P<n> for
another size) and lists of its first k boxes, k from short lists to the whole
level.  For every list, face centring, into a pool [3, k, m, m, m] with
m = 16 + 2 * width (--width 1, one ghost layer: the layout of an AMR host),
for {no coefficient, one coefficient (5, 5, 5), three coefficients (5, 6, 7)}
x {write, accumulate}:

(a) the new call through the tile kernel (OMG_BOXES_TILE=1), the per-cell
    kernel (OMG_BOXES_GENERIC=1) and the library's own routing, in alternating
    rounds of one process, timed twice: by the library's HIP events around its
    kernels (omg_kernel_stats, family boxes_flux) and by events on the
    caller's stream around the call;
(b) the path it replaces, on the entries that existed before this one:
    get_blocks_grad(face) into the pool (write) or into a scratch pool
    (accumulate), get_blocks(ghosts=True) of each distinct coefficient into a
    pool of its own, the harmonic means ((2 a_lo) a_hi) / (a_lo + a_hi) and the
    product as torch elementwise calls on slices, then add_ of the scratch
    pool; by events on the caller's stream, in the same rounds;
* the host time of a call with a cached list (wall time of 1000 calls of an
  8-box list queued without a wait, per call).

Before anything is timed, both kernels and the replaced path must leave the
same bits in the pool.  One JSON line on stdout.  No GPU, no result: there is
no fallback.
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
IPHI = 1
VARIANTS = ("default", "tile", "generic")
COEFS = {"none": (0, 0, 0), "one": (5, 5, 5), "three": (5, 6, 7)}


def build(omg, n):
    T = omg.tree
    mg = omg.MG()
    mg.operator_type = T.MG_LAPLACIAN
    mg.smoother_type = T.MG_SMOOTHER_GSRB
    mg.n_extra_vars = 3   # (variables 5..7: the coefficients)
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


def old_path(mg, torch, ids, out, scratch, cpools, tmp, tmp2, coef, acc, width):
    """What a host does without the entry: the face gradient, the coefficient
    with its ghosts, the harmonic means and the product elementwise, the add."""
    dst = scratch if acc else out
    mg.get_blocks_grad(ids, IPHI, out=dst, ghost_width=width, scale=-1.0, fill=False, centering="face")
    for v in sorted(set(coef) - {0}):
        mg.get_blocks(v, ids, out=cpools[v], ghost_width=width, ghosts=True, fill=False)
    w = slice(width, width + BOX)
    for d in range(3):
        if not coef[d]:
            continue
        ax = 3 - d
        lo, hi = [slice(None), w, w, w], [slice(None), w, w, w]
        lo[ax] = slice(width - 1, width + BOX)
        hi[ax] = slice(width, width + BOX + 1)
        c = cpools[coef[d]]
        a_lo, a_hi = c[tuple(lo)], c[tuple(hi)]
        h, s = tmp[d], tmp2[d]
        torch.mul(a_lo, 2.0, out=h)
        h.mul_(a_hi)
        torch.add(a_lo, a_hi, out=s)
        h.div_(s)
        dst[d][tuple(lo)].mul_(h)
    if acc:
        out.add_(scratch)


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
    """ms per call of the library's events around the family boxes_flux."""
    mg.ctx.call("reset_stats")
    for _ in range(reps):
        call()
    n, ms, _ = mg.ctx.kernel_stats("boxes_flux")
    assert n == reps, (n, reps)
    return ms / reps


def measure(omg, torch, n_dom, counts, rounds, reps, width):
    mg = build(omg, n_dom)
    ctx = mg.ctx
    all_ids = [int(i) for i in mg.lvls[1].my_ids]
    m = BOX + 2 * width
    res = {"tree": f"P{n_dom}: {n_dom}^3, box 16, periodic, the first k of the {len(all_ids)} boxes of level 1",
           "pool": "[3, k, m, m, m], m = %d, ghost width %d" % (m, width), "centering": "face", "scale": -1.0,
           "rounds": rounds, "calls_per_round": reps, "lists": {}}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    # phi random, the coefficients in [0.5, 2]; ghosts filled (periodic)
    n_all = len(all_ids)
    mg.set_blocks(IPHI, torch.randn((n_all, BOX, BOX, BOX), dtype=torch.float64, device="cuda", generator=gen),
                  all_ids)
    omg.mg_fill_ghost_cells(mg, IPHI)
    for v in (5, 6, 7):
        c = torch.rand((n_all, BOX, BOX, BOX), dtype=torch.float64, device="cuda", generator=gen) * 1.5 + 0.5
        mg.set_blocks(v, c, all_ids)
        omg.mg_fill_ghost_cells(mg, v)
        del c
    ctx.call("set_profiling", 1)
    for k in counts:
        ids = all_ids[:k]
        print(f"box_flux_bench: {k} boxes", file=sys.stderr, flush=True)
        base = torch.randn((3, k, m, m, m), dtype=torch.float64, device="cuda", generator=gen)
        out = base.clone()
        ref = base.clone()
        scratch = torch.zeros_like(base)
        cpools = {v: torch.zeros((k, m, m, m), dtype=torch.float64, device="cuda") for v in (5, 6, 7)}
        tmp = [torch.zeros((k, BOX + (d == 2), BOX + (d == 1), BOX + (d == 0)), dtype=torch.float64, device="cuda")
               for d in range(3)]
        tmp2 = [torch.zeros_like(t) for t in tmp]
        entry = {"boxes": k}
        values = k * (BOX + 1) * BOX * BOX
        for cname, coef in COEFS.items():
            for acc in (False, True):
                def new():
                    return mg.get_blocks_flux(ids, IPHI, coef=coef, out=out, ghost_width=width, scale=-1.0,
                                              fill=False, centering="face", accumulate=acc)[1]

                def old():
                    old_path(mg, torch, ids, out, scratch, cpools, tmp, tmp2, coef, acc, width)

                # what is timed leaves the same bits in the pool
                scratch.zero_()
                out.copy_(base)
                old()
                ref.copy_(out)
                assert not bool((ref == base).all())
                for v in ("tile", "generic"):
                    set_variant(v)
                    out.copy_(base)
                    assert new() == values
                    assert bool((out.view(torch.int64) == ref.view(torch.int64)).all()), (k, cname, acc, v)
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
                case = {"values_per_component": values,
                        "new_call_library_events": {v: summary(fam[v]) for v in VARIANTS},
                        "new_call_caller_stream": {v: summary(strm[v]) for v in VARIANTS},
                        "replaced_path_caller_stream": summary(repl),
                        "tile_faster_than_generic": max(fam["tile"]) < min(fam["generic"]),
                        "generic_faster_than_tile": max(fam["generic"]) < min(fam["tile"]),
                        "replaced_over_new_default": round(statistics.median(repl) /
                                                           statistics.median(strm["default"]), 2),
                        "new_faster_than_replaced": max(strm["default"]) < min(repl),
                        "new_slower_than_replaced": min(strm["default"]) > max(repl)}
                entry[f"{cname}-{'accumulate' if acc else 'write'}"] = case
        res["lists"][str(k)] = entry
        del base, out, ref, scratch, cpools, tmp, tmp2
        torch.cuda.empty_cache()
    ctx.call("set_profiling", 0)

    # the host's share of a call with a cached list
    ids = all_ids[:8]
    pool = torch.zeros((3, 8, m, m, m), dtype=torch.float64, device="cuda")
    calls = 1000
    host = []
    for _ in range(5):
        mg.get_blocks_flux(ids, IPHI, coef=(5, 6, 7), out=pool, ghost_width=width, fill=False, accumulate=True)
        torch.cuda.synchronize()
        before = ctx.host_sync_count()
        t0 = time.perf_counter()
        for _ in range(calls):
            mg.get_blocks_flux(ids, IPHI, coef=(5, 6, 7), out=pool, ghost_width=width, fill=False, accumulate=True)
        host.append((time.perf_counter() - t0) * 1e6 / calls)
        assert ctx.host_sync_count() == before
        torch.cuda.synchronize()
    res["cached_list_host_us_per_call"] = {"median": round(statistics.median(host), 2), "min": round(min(host), 2),
                                           "max": round(max(host), 2), "calls": calls, "boxes": 8,
                                           "through": "MG.get_blocks_flux (the Python binding included)"}
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
        sys.exit("box_flux_bench: no GPU (the tool measures on the device or not at all)")
    omg = __graft_entry__.load_package()
    out = {"tool": "box_flux_bench", "device": torch.cuda.get_device_name(0),
           "timing": "HIP events: the library's around its kernels, torch's on the caller's stream"}
    out[a.tree] = measure(omg, torch, int(a.tree[1:]), [int(c) for c in a.counts.split(",")], a.rounds, a.reps,
                          a.width)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
