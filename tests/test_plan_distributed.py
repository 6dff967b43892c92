"""Multi-rank communication plans on CPU: world_size 2 and 3 gloo process
groups, each rank building its own plan-only context (OMG_DEVICE_NONE) of
libomg.so from its own copy of the tree, exactly as mg_allocate_storage does on
a GPU rank.  The plans are exchanged over gloo and checked pairwise:

* what rank a sends to rank b in a transfer (ghost faces, restriction,
  prolongation, refinement-boundary faces) is, key for key and in wire order,
  what b expects from a — the property sort_and_transfer_buffers relies on
  (src/m_communication.f90:37-66);
* every face of a box whose neighbour lives on another rank is received
  exactly once (6*id+nb), and every refinement-boundary face whose coarse
  neighbour lives elsewhere arrives in the refinement-boundary transfer.

The data path over those plans is checked bit for bit against the reference
at 2-8 ranks on the GPU (tests/test_gpu_multirank.py)."""
import os
import socket

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.mgdriver import T, build_tree, omg, parse

CASES = [
    ("8 32 32 32 1 v gsrb lpl 0 per sol 1 lb 0", 2, 0),     # periodic halo
    ("8 64 32 32 1 v gs lpl 0 d0 sol 1 lbp 0", 2, 0),       # non-cube, parents balanced
    ("8 32 32 32 1 v gs lpl 0 sol sol 3 lb 0", 2, 0),       # 3-level refined tree
    ("8 32 32 32 1 v gs lpl 0 sol sol 2 lb 0", 3, 0),       # refinement boundaries across ranks
    ("8 32 32 32 1 v gsrb lpl 0 d0 sol 3 lb 0", 3, 0),
    # replicated coarse levels (omg_set_coarse_replication): all coarse
    # levels, or only those of at most 4096 cells
    ("8 64 64 64 1 v gsrb lpl 0 per sol 1 lb 0", 3, 1 << 40),
    ("8 64 64 64 1 v gsrb lpl 0 per sol 1 lb 0", 2, 4096),
    ("8 32 32 32 1 v gs lpl 0 sol sol 2 lb 0", 3, 1 << 40),  # + refinement boundaries
]
WHICH = {0: "halo", 1: "restrict", 2: "prolong", 3: "refinement-boundary", 4: "replica", 5: "deep"}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _plans(args, rank, world, rep):
    cfg = parse(args)
    tree = build_tree(cfg, T.MGTree(), world, rank)
    ctx = omg.device.Context(-2, rank, world)   # OMG_DEVICE_NONE
    if rep:
        ctx.call("set_coarse_replication", rep)
    arrs = omg.mg._tree_arrays(tree)
    ctx.call("tree_setup", tree.n_boxes, *arrs[:6], tree.lowest_lvl, tree.highest_lvl,
             tree.first_normal_lvl, tree.box_size, arrs[6], arrs[7], arrs[8], arrs[9], 5)
    out = {}
    for lvl in range(tree.lowest_lvl, tree.highest_lvl + 1):
        for w in WHICH:
            for d in (0, 1):
                out[(lvl, w, d)] = ctx.plan_transfer(lvl, w, d)
    rep_lvl = ctx.replicated_level()
    ctx.close()
    return out, rep_lvl


def _expected_remote(args, rank, world, rep_lvl):
    """Faces of my boxes that need data from another rank, from the tree
    alone (a box of a replicated level is on every rank)."""
    cfg = parse(args)
    t = build_tree(cfg, T.MGTree(), world, rank)
    mine = lambda i: t.lvl[i] <= rep_lvl or t.rank[i] == rank  # noqa: E731
    halo, rb = {}, {}
    for lvl in range(t.lowest_lvl, t.highest_lvl + 1):
        h, r = set(), set()
        for id_ in t.lvls[lvl].ids:
            if not mine(id_):
                continue
            for nb in range(1, 7):
                nid = t.neighbors[id_][nb - 1]
                if nid > 0 and not mine(nid):
                    h.add(6 * int(id_) + nb)
                elif nid == 0:
                    pn = t.neighbors[t.parent[id_]][nb - 1]
                    if not mine(pn):
                        r.add(6 * int(id_) + nb)
        halo[lvl], rb[lvl] = h, r
    return halo, rb


def _expected_deep(args, rank, world):
    """The deep halo of the finest level from box coordinates alone: whether
    the level takes it (16^3 leaves, every rank's x pairs of boxes on one rank,
    split over ranks) and the bricks (64*id + brick) this rank's k_gsrb3 /
    k_gsrb4 columns read of other ranks' boxes: a box B at periodic offset
    (dx, dy, dz) in -1..1 from one of my boxes shows it its 4 layers toward
    it (brick index 3 where B is below, 0 where above) and all 16 across."""
    cfg = parse(args)
    t = build_tree(cfg, T.MGTree(), world, rank)
    lvl = t.highest_lvl
    ids = [int(i) for i in t.lvls[lvl].ids]
    ix = {i: [int(v) for v in t.ix[i]] for i in ids}
    n = [max(ix[i][d] for i in ids) for d in range(3)]
    own = {i: int(t.rank[i]) for i in ids}
    at = {tuple(ix[i]): i for i in ids}
    pairs_ok = all(own[i] == own[at[((ix[i][0] - 1) ^ 1) + 1, ix[i][1], ix[i][2]]] for i in ids)
    split = len(set(own.values())) > 1
    deep = cfg["box"] == 16 and cfg["n_levels"] == 1 and cfg["bc"] == "per" and pairs_ok and split
    want = set()
    for a in ids:
        if own[a] != rank:
            continue
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    o = (dx, dy, dz)
                    if o == (0, 0, 0):
                        continue
                    b = at[tuple((ix[a][d] - 1 + o[d]) % n[d] + 1 for d in range(3))]
                    if own[b] == rank:
                        continue
                    for br in range(64):
                        bb = (br & 3, (br >> 2) & 3, br >> 4)
                        # B at offset o from A: A at -o from B reads the bricks toward it
                        if all(o[d] == 0 or bb[d] == (0 if o[d] > 0 else 3) for d in range(3)):
                            want.add(64 * b + br)
    return lvl, deep, want


def _worker(rank, world, port, args, rep, q, env=None):
    try:
        os.environ.update(env or {})
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank,
                                world_size=world)
        mine, rep_lvl = _plans(args, rank, world, rep)
        allp = [None] * world
        dist.all_gather_object(allp, mine)
        problems = []
        for (lvl, w, d), (items, per) in mine.items():
            if d != 0:
                continue
            for b in range(world):
                if b == rank:
                    if any(p == rank for p, _ in items):
                        problems.append(f"lvl {lvl} {WHICH[w]}: send to self")
                    continue
                sent = [k for p, k in items if p == b]
                got, per_b = allp[b][(lvl, w, 1)]
                expected = [k for p, k in got if p == rank]
                if sent != expected:
                    problems.append(f"lvl {lvl} {WHICH[w]}: {rank}->{b} sends {len(sent)} keys, "
                                    f"{b} expects {len(expected)}")
                if sent and per != per_b:
                    problems.append(f"lvl {lvl} {WHICH[w]}: item size {per} vs {per_b}")
        halo, rb = _expected_remote(args, rank, world, rep_lvl)
        if rep:
            lo = min(lv for lv, _, _ in mine)
            if rep_lvl < lo:
                problems.append("replication requested but no level replicated")
            # a replicated level has no halo, and no prolongation out of it
            for (lvl, w, d), (items, _) in mine.items():
                if items and ((lvl <= rep_lvl and w in (0, 3)) or (lvl <= rep_lvl + 1 and w == 2)):
                    problems.append(f"lvl {lvl} {WHICH[w]}: {len(items)} items on a replicated level")
            # every rank restricts into every copy of the highest replicated level
            up = rep_lvl + 1
            if world > 1 and (up, 1, 0) in mine:
                peers = {p for p, _ in mine[(up, 1, 0)][0]}
                if peers != set(range(world)) - {rank}:
                    problems.append(f"lvl {up} restrict goes to {sorted(peers)}, not to every peer")
        for lvl in halo:
            got_h = [k for _, k in mine[(lvl, 0, 1)][0]]
            got_r = [k for _, k in mine[(lvl, 3, 1)][0]]
            if sorted(got_h) != sorted(halo[lvl]) or len(set(got_h)) != len(got_h):
                problems.append(f"lvl {lvl}: halo receives {len(got_h)} faces, tree needs {len(halo[lvl])}")
            if sorted(got_r) != sorted(rb[lvl]):
                problems.append(f"lvl {lvl}: rb receives {len(got_r)} faces, tree needs {len(rb[lvl])}")
        if env:
            lvl, deep, want = _expected_deep(args, rank, world)
            got = [k for _, k in mine[(lvl, 5, 1)][0]]
            if bool(got) != deep:
                problems.append(f"lvl {lvl}: deep halo {'on' if got else 'off'}, expected {'on' if deep else 'off'}")
            if deep and (sorted(got) != sorted(want) or len(set(got)) != len(got)):
                problems.append(f"lvl {lvl}: deep halo receives {len(got)} bricks, the columns read {len(want)}")
            if deep and mine[(lvl, 5, 1)][1] != 32:
                problems.append(f"lvl {lvl}: deep item of {mine[(lvl, 5, 1)][1]} doubles")
        n_rb = sum(len(v) for v in rb.values())
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, problems, n_rb))
    except Exception as e:  # noqa: BLE001
        q.put((rank, [f"{type(e).__name__}: {e}"], 0))


def _run(args, world, rep, env=None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, args, rep, q, env)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(60)
    problems = [f"rank {r}: {m}" for r, ms, _ in res for m in ms]
    assert not problems, "\n".join(problems)
    return res


@pytest.mark.parametrize("args,world,rep", CASES)
def test_plans_pair_up_across_ranks(args, world, rep):
    res = _run(args, world, rep)
    if world == 3 and " 2 lb" in args and not rep:
        assert sum(n for _, _, n in res) > 0, "case meant to cross refinement boundaries has none"


# The deep halo of k_gsrb3 / k_gsrb4 on a split level (omg_plan.cpp plan_deep),
# with the pass's level bound lowered to one box (OMG_BLOCK3_MIN_BOXES): the
# brick lists pair up key for key, every rank receives exactly the bricks its
# columns read (from box coordinates, _expected_deep), and a level whose x
# pairs of boxes straddle ranks (128^3 at 3 ranks: 171 boxes on the first)
# is declined on every rank alike.
DEEP = [("16 64 64 64 1 v gsrb lpl 0 per sol 1 lb 0", 2),
        ("16 128 64 64 1 v gsrb lpl 0 per sol 1 lb 0", 4),
        ("16 128 128 128 1 v gsrb lpl 0 per sol 1 lb 0", 3),
        ("16 128 128 128 1 v gsrb helm 1 per sol 1 lb 0", 8)]


@pytest.mark.parametrize("args,world", DEEP)
def test_deep_halo_plans_pair_up(args, world):
    _run(args, world, 0, {"OMG_BLOCK3_MIN_BOXES": "1"})
