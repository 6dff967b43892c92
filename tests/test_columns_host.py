"""The block passes' column records and coarse records (omg_columns.cpp,
omg_plan_columns) on plan-only contexts, every rank's built in turn in this
process (no process group: a plan needs none).

A. Against the parent: the sha256 of both tables, every case, rank and level,
   equals what the commit before omg_columns.cpp built
   (tests/golden/columns_parent.json, profiles/r11/columns_README.md).  Where
   two columns of a rank share a sort key the parent's order was unspecified
   and the multiset of records is compared instead (TIES: no case has any).
B. Against box coordinates: a model that knows only tree.ix, tree.rank and the
   level's id order builds every record from the start / stop rule and the
   coordinates of the boxes around the column.  Which levels have tables at
   all is stated per case (TABLES) and was read off the parent; a case listed
   as declined has none.

Run as a program it records A's file with the library OMG_LIB names:
    OMG_LIB=.../libomg.so python -m tests.test_columns_host OUT.json"""
import functools
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from tests.mgdriver import T, build_tree, omg, parse
from tests.test_plan_distributed import DEEP, _expected_deep

# the record layout (omg_kernels.h), restated
TX, MAXZ = 2, 16
S = 3 * (TX + 2)
REC = (1 + S * (MAXZ + 2) + 15) // 16 * 16
CREC = (1 + 9 * (MAXZ // 2 + 2) + 15) // 16 * 16

MIN1 = {"OMG_BLOCK3_MIN_BOXES": "1"}
SWITCHES = ("OMG_BLOCK3_MIN_BOXES", "OMG_BLOCK3_COLUMN", "OMG_BLOCK3_SMALL_COL", "OMG_NO_BLOCK3_PHYS",
            "OMG_NO_BLOCK3", "OMG_NO_DEEP")
PER64 = "16 64 64 64 1 v gsrb lpl 0 per sol 1 lb 0"
D0_64 = "16 64 64 64 1 v gsrb lpl 0 d0 sol 1 lb 0"
# name: (driver arguments, ranks, switches, {level: columns per rank}, {level: coarse records per rank});
# a level not named has no table
CASES = {
    # level 1: 16 columns of 2 boxes; level 0 (2x2x2 boxes) over the single 16^3 box of level -1
    "per64": (PER64, 1, MIN1, {0: 2, 1: 16}, {0: 2, 1: 16}),
    # a column is the whole z extent: the slots below and above wrap onto the column itself
    "per64_col4": (PER64, 1, dict(MIN1, OMG_BLOCK3_COLUMN="4"), {0: 2, 1: 8}, {0: 2, 1: 8}),
    # x, y, z told apart; 3 boxes in z: a column of 1 box stops at the wrap, so no coarse records
    "per128x64x48": ("16 128 64 48 1 v gsrb lpl 0 per sol 1 lb 0", 1, MIN1, {1: 32}, {}),
    # physical faces: all six flags, slots clamped at faces, edges and corners, columns stopping at z+
    "d0_64": (D0_64, 1, MIN1, {0: 2, 1: 16}, {}),
    "d0_128x64x48": ("16 128 64 48 1 v gsrb lpl 0 d0 sol 1 lb 0", 1, MIN1, {1: 32}, {}),
    # declined
    "d0_64_no_phys": (D0_64, 1, dict(MIN1, OMG_NO_BLOCK3_PHYS="1"), {}, {}),
    "per64_default_min": (PER64, 1, {}, {}, {}),                       # 64 boxes < kB3MinBoxes
    "per32_box8": ("8 32 32 32 1 v gsrb lpl 0 per sol 1 lb 0", 1, MIN1, {}, {}),
    # two levels refine every box of level 1: level 2 is uniform (no refinement-boundary face), both
    # have tables; with three levels, level 3 covers the middle of level 2 and is declined
    "refined2": ("16 32 32 32 1 v gsrb lpl 0 sol sol 2 lb 0", 1, MIN1, {1: 2, 2: 16}, {}),
    "refined3": ("16 32 32 32 1 v gsrb lpl 0 sol sol 3 lb 0", 1, MIN1, {1: 2, 2: 16}, {}),
    # split levels (tests/test_plan_distributed.py's DEEP); 128^3 at 3 ranks is declined on every rank
    "deep64_2": (DEEP[0][0], DEEP[0][1], MIN1, {0: 2, 1: 8}, {1: 8}),
    "deep128x64x64_4": (DEEP[1][0], DEEP[1][1], MIN1, {0: 2, 1: 8}, {1: 8}),
    "deep128_3": (DEEP[2][0], DEEP[2][1], MIN1, {}, {}),
    "deep128_8": (DEEP[3][0], DEEP[3][1], MIN1, {0: 2, 1: 16}, {1: 16}),
}
# cases in which two columns of one rank share a sort key (a rank boundary
# inside a z block): the parent's order of those was unspecified
TIES = ()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "columns_parent.json")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(tree, {(rank, lvl): (column records, coarse records)}) of a case."""
    args, world, env = CASES[name][:3]
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        tree = build_tree(parse(args), T.MGTree(), world, 0)   # (the same tree on every rank)
        arrs = omg.mg._tree_arrays(tree)
        out = {}
        for rank in range(world):
            ctx = omg.device.Context(-2, rank, world)   # OMG_DEVICE_NONE
            ctx.call("tree_setup", tree.n_boxes, *arrs[:6], tree.lowest_lvl, tree.highest_lvl,
                     tree.first_normal_lvl, tree.box_size, arrs[6], arrs[7], arrs[8], arrs[9], 5)
            for lvl in range(tree.lowest_lvl, tree.highest_lvl + 1):
                out[(rank, lvl)] = (ctx.plan_columns(lvl, 0), ctx.plan_columns(lvl, 1))
            ctx.close()
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return tree, out


def _digests(a):
    a = np.ascontiguousarray(a, dtype="<i4")
    rows = sorted(a[i].tobytes() for i in range(a.shape[0]))
    return {"n": int(a.shape[0]), "sha256": hashlib.sha256(a.tobytes()).hexdigest(),
            "sha256_multiset": hashlib.sha256(b"".join(rows)).hexdigest()}


def _record(name):
    _, out = _case(name)
    return {f"{rank}/{lvl}": {"columns": _digests(a), "coarse": _digests(b)} for (rank, lvl), (a, b) in out.items()}


@pytest.mark.parametrize("name", CASES)
def test_tables_equal_the_parents(name):
    want = json.load(open(GOLDEN))[name]
    got = _record(name)
    assert sorted(got) == sorted(want)
    fields = ("n", "sha256_multiset") if name in TIES else ("n", "sha256")
    for k in want:
        for t in ("columns", "coarse"):
            for f in fields:
                assert got[k][t][f] == want[k][t][f], (name, k, t, f)


# ---------------------------------------------------------------------------
# the model

def _spread(v):
    return sum(((v >> q) & 1) << (2 * q) for q in range(20))


def _level(tree, lvl, rank, per, world):
    """The boxes of a level from tree.ix, tree.rank and the id order: 0-based
    coordinates, this rank's boxes in id order (their local indices), the
    proxies (the distinct other-rank boxes in the 26-neighbourhoods of own
    boxes, ascending id) and each box's name in the records."""
    ids = [int(i) for i in tree.lvls[lvl].ids]
    ix = {i: tuple(int(v) - 1 for v in tree.ix[i]) for i in ids}
    n = [max(ix[i][d] for i in ids) + 1 for d in range(3)]
    at = {ix[i]: i for i in ids}
    own = [i for i in ids if int(tree.rank[i]) == rank]

    def box_at(co):
        # periodic: wraps; else across a physical face the box whose face it is
        co = tuple(c % n[d] if per else min(max(c, 0), n[d] - 1) for d, c in enumerate(co))
        return at[co]

    prox = set()
    if world > 1 and len(at) == n[0] * n[1] * n[2]:
        for a in own:
            for dz in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        b = box_at((ix[a][0] + dx, ix[a][1] + dy, ix[a][2] + dz))
                        if int(tree.rank[b]) != rank:
                            prox.add(b)
    prox = sorted(prox)
    name = {b: q for q, b in enumerate(own)}
    name.update({b: len(own) + q for q, b in enumerate(prox)})
    return SimpleNamespace(ix=ix, n=n, own=own, ownset=set(own), prox=prox, name=name, box_at=box_at)


def _expected_columns(L, nzb, per):
    """[(key, (x, y, z, len), record)] in the records' order."""
    cols = []
    for h in L.own:
        x, y, z = L.ix[h]
        # starts: x a multiple of the tile, z a multiple of the column length or above another rank's box
        if x % TX or (z % nzb and L.box_at((x, y, z - 1)) in L.ownset):
            continue
        # stops: at the length, at the z+ face, below another rank's box or the next column's first
        ln = 1
        while ln < nzb and (per or z + ln < L.n[2]):
            up = L.box_at((x, y, z + ln))
            if up not in L.ownset or L.ix[up][2] % nzb == 0:
                break
            ln += 1
        flags = 0
        if not per:
            faces = (x == 0, x + TX == L.n[0], y == 0, y + 1 == L.n[1], z == 0, z + ln == L.n[2])
            flags = sum(1 << f for f in range(6) if faces[f])
        rec = np.zeros(REC, np.int32)
        rec[0] = ln | flags << 8
        for zs in range(ln + 2):
            for ys in range(3):
                for xs in range(TX + 2):
                    rec[1 + S * zs + (TX + 2) * ys + xs] = L.name[L.box_at((x + xs - 1, y + ys - 1, z + zs - 1))]
        key = ((z // nzb) << 40) | _spread(x // TX) | (_spread(y) << 1)
        cols.append((key, (x, y, z, ln), rec))
    return sorted(cols, key=lambda c: c[0])   # (stable)


def _expected_coarse(cols, C):
    out = []
    for _, (x, y, z, ln), _ in cols:
        rec = np.zeros(CREC, np.int32)
        rec[0] = (y % 2) * 8
        for zc in range(ln // 2 + 2):
            for ys in range(3):
                for xs in range(3):
                    rec[1 + 9 * zc + 3 * ys + xs] = C.name[C.box_at((x // 2 + xs - 1, y // 2 + ys - 1, z // 2 + zc - 1))]
        out.append(rec)
    return out


@pytest.mark.parametrize("name", CASES)
def test_tables_against_box_coordinates(name):
    args, world, env, n_cols, n_coarse = CASES[name]
    cfg = parse(args)
    per = cfg["bc"] == "per"
    nzb = int(env.get("OMG_BLOCK3_COLUMN", 2))
    tree, out = _case(name)
    ties = False
    for (rank, lvl), (recs, crecs) in out.items():
        assert recs.shape[1] == REC and crecs.shape[1] == CREC
        assert recs.shape[0] == n_cols.get(lvl, 0), (name, rank, lvl)
        assert crecs.shape[0] == n_coarse.get(lvl, 0), (name, rank, lvl)
        if lvl not in n_cols:
            continue
        L = _level(tree, lvl, rank, per, world)
        want = _expected_columns(L, nzb, per)
        keys = [k for k, _, _ in want]
        ties |= len(set(keys)) != len(keys)
        assert keys == sorted(keys)
        # every own box in exactly one column, at slots zs 1..len, xs 1..kB3TX of the middle row
        seen = []
        for r in recs:
            ln = int(r[0]) & 255
            assert 1 <= ln <= nzb
            grid = r[1:1 + S * (ln + 2)].reshape(ln + 2, 3, TX + 2)
            seen += grid[1:ln + 1, 1, 1:TX + 1].reshape(-1).tolist()
            assert not r[1 + S * (ln + 2):].any()   # nothing past slot len+1
        assert sorted(seen) == list(range(len(L.own)))
        assert len(L.own) == sum(TX * (int(r[0]) & 255) for r in recs) and len(recs) > 0
        # the columns, their lengths and flags, every slot, and the order
        assert len(want) == len(recs)
        if name in TIES:
            by_head = {int(r[1 + S + (TX + 2) + 1]): r for r in recs}
            for _, _, w in want:
                assert np.array_equal(by_head[int(w[1 + S + (TX + 2) + 1])], w)
        else:
            for q, (_, col, w) in enumerate(want):
                assert np.array_equal(recs[q], w), (name, rank, lvl, q, col)
        if not per:   # every flag occurs
            assert {f for r in recs for f in range(6) if int(r[0]) >> (8 + f) & 1} == set(range(6))
        if lvl in n_coarse:
            C = _level(tree, lvl - 1, rank, per, world)
            cw = _expected_coarse(want, C)
            assert len(cw) == len(crecs)
            for q, w in enumerate(cw):
                assert np.array_equal(crecs[q], w), (name, rank, lvl, q)
            # every coarse box is the own box of exactly two columns
            mid = [int(r[1 + 9 * zc + 4]) for r, (_, col, _) in zip(crecs, want) for zc in range(1, col[3] // 2 + 1)]
            assert sorted(mid) == sorted(2 * list(range(len(C.own))))
    assert ties == (name in TIES)


def test_odd_columns_have_no_coarse_records():
    _, out = _case("per128x64x48")
    recs, crecs = out[(0, 1)]
    assert sorted(set((recs[:, 0] & 255).tolist())) == [1, 2] and crecs.shape[0] == 0


def test_whole_extent_column_wraps_onto_itself():
    _, out = _case("per64_col4")
    for r in out[(0, 1)][0]:
        grid = r[1:1 + S * 6].reshape(6, 3, TX + 2)
        assert int(r[0]) == 4 and np.array_equal(grid[0], grid[4]) and np.array_equal(grid[5], grid[1])


@pytest.mark.parametrize("q", range(len(DEEP)))
def test_proxies_are_the_boxes_of_the_deep_halos_bricks(q):
    """The model's proxies are the boxes whose bricks tests/test_plan_distributed.py
    expects this rank to receive, and the records name no other remote box."""
    args, world = DEEP[q]
    name = [k for k, v in CASES.items() if v[0] == args and v[1] == world][0]
    tree, out = _case(name)
    for rank in range(world):
        lvl, deep, want = _expected_deep(args, rank, world)
        L = _level(tree, lvl, rank, True, world)
        recs = out[(rank, lvl)][0]
        assert deep == (recs.shape[0] > 0)
        if not deep:
            continue
        assert set(L.prox) == {k // 64 for k in want}
        named = set()
        for r in recs:
            ln = int(r[0]) & 255
            named |= set(r[1:1 + S * (ln + 2)].tolist())
        assert {s for s in named if s >= len(L.own)} == set(range(len(L.own), len(L.own) + len(L.prox)))


def test_refinement_boundaries_decline_the_level():
    tree, out = _case("refined3")
    ids = tree.lvls[3].ids
    assert (tree.neighbors[ids] == 0).any()   # level 3 has refinement-boundary faces
    assert out[(0, 3)][0].shape[0] == 0 and out[(0, 3)][1].shape[0] == 0
    ids = _case("refined2")[0].lvls[2].ids
    assert not (_case("refined2")[0].neighbors[ids] == 0).any()   # (level 2 of the two-level tree has none)


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump({name: _record(name) for name in CASES}, f, indent=1, sort_keys=True)
        f.write("\n")
