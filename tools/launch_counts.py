"""Launch counts of a sequence of cycles on one tree: for every step, the
launches of every kernel family (every `Prof p(c, "...")` name in
octree-mg_amd/csrc) at every level and the host waits on the context's
streams (omg_host_sync_count), per rank.  Nothing in the output is a time, so
two builds that launch alike print the same bytes: compare a parent build
(OMG_LIB=...) against this tree's with `cmp`.

    python tools/launch_counts.py ARGS [--ranks N] [--counts D,U] [--warmup W] [--steps S]

ARGS is a driver argument string (tests/mgdriver.py's parse); C4 stands for
bench.py's c4_refined tree.  N > 1 runs N loopback ranks on one GPU.  S is a
comma-separated list of v0 (a stand-alone V-cycle), v1 (one with the max
residual), fmg (FMG with a guess), op (mg_apply_op into res); the default is
three cycles without the max residual, one with it, an FMG cycle, and
mg_apply_op followed by a cycle, after W = 2 warm-up cycles.  The switches
(OMG_BLOCK3_MIN_BOXES, OMG_NO_DEEP, ...) come from the environment and are
echoed in the header.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.mgdriver import DeviceBackend, T, omg, parse, run_loopback, setup_problem  # noqa: E402

C4_ARGS = "16 128 128 128 1 v gsrb lpl 0 sol sol 2 lb 0"
FAMILIES = ["box_sums", "boxes_get", "boxes_get_tile", "boxes_put", "boxes_put_tile", "coarse_rhs", "coarse_tail",
            "comm", "comm_overlap", "deep_faces", "deep_phi", "deep_res", "deep_rhs", "dense_get", "dense_get_row",
            "dense_grad", "dense_grad_row", "dense_put", "dense_put_row", "face_gc", "fill_crhs", "fill_gc",
            "free_fft_solve", "prolong", "prolong_fill", "prolong_smooth", "resid_restrict", "residual", "restrict",
            "rhs_lex", "seq_sum", "smooth_resid", "smoother_gs", "smoother_gsrb", "smoother_gsrb3", "smoother_gsrb3p",
            "smoother_gsrb3r", "smoother_gsrb4", "smoother_gsrb4p", "sub_parents", "subtract", "subtract_rhs"]
DEFAULT_STEPS = "v0,v0,v0,v1,fmg,op,v0"


def run_step(be, step):
    if step in ("v0", "v1"):
        be.vcycle(step == "v1")
    elif step == "fmg":
        be.fmg(True, False)
    elif step == "op":
        be.apply_op(T.MG_IRES)
    else:
        raise SystemExit(f"unknown step {step!r}")


def body_for(steps, warmup, counts):
    def body(be, rank=0, reduce=None):
        mg, c = be.mg, be.mg.ctx
        if counts:
            mg.n_cycle_down, mg.n_cycle_up = counts
            mg._push_methods()
        for _ in range(warmup):
            omg.mg_fas_vcycle(mg)
        c.call("synchronize")
        c.call("set_profiling", 1)
        out = []
        for step in steps:
            c.call("reset_stats")
            syncs = c.host_sync_count()
            run_step(be, step)
            c.call("synchronize")
            n = {}
            for lvl in range(mg.lowest_lvl, mg.highest_lvl + 1):
                for f in FAMILIES:
                    k = c.kernel_stats(f"{f}@{lvl}")[0]
                    if k:
                        n[(f, lvl)] = k
            for f in FAMILIES:   # (the families that carry no level)
                k = c.kernel_stats(f)[0] - sum(v for (g, _), v in n.items() if g == f)
                if k:
                    n[(f, None)] = k
            out.append((n, c.host_sync_count() - syncs))
        c.call("set_profiling", 0)
        return out
    return body


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("args")
    ap.add_argument("--ranks", type=int, default=1)
    ap.add_argument("--counts", default="")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", default=DEFAULT_STEPS)
    a = ap.parse_args()
    args = C4_ARGS if a.args == "C4" else a.args
    steps = a.steps.split(",")
    counts = tuple(int(x) for x in a.counts.split(",")) if a.counts else None
    body = body_for(steps, a.warmup, counts)
    if a.ranks > 1:
        res = run_loopback(args, a.ranks, body)
    else:
        be = DeviceBackend(parse(args))
        setup_problem(be)
        res = [body(be)]
    env = " ".join(f"{k}={v}" for k, v in sorted(os.environ.items()) if k.startswith("OMG_") and k != "OMG_LIB")
    print(f"# {args} | ranks {a.ranks} | counts {a.counts or 'default'} | warmup {a.warmup} | {env or 'no switches'}")
    for i, step in enumerate(steps):
        print(f"step {i + 1} {step}: host syncs " + " ".join(str(r[i][1]) for r in res))
        keys = sorted(set(k for r in res for k in r[i][0]), key=lambda k: (-(k[1] if k[1] is not None else 99), k[0]))
        for f, lvl in keys:
            n = " ".join("%-4d" % r[i][0].get((f, lvl), 0) for r in res)
            print(("  %-16s %5s " % (f, "-" if lvl is None else lvl) + n).rstrip())
        print(("  %-16s %5s " % ("total", "") + " ".join("%-4d" % sum(r[i][0].values()) for r in res)).rstrip())


if __name__ == "__main__":
    main()
