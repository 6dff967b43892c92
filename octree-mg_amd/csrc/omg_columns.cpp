// omg_columns.cpp — the tables the block passes (k_gsrb3 / k_gsrb4) read a
// level through: per workgroup a column record, for the correction form a
// coarse record (layouts: launch_gsrb3 / launch_gsrb4 in omg_kernels.h).
//
// A level of 16^3 boxes is tiled by columns of kB3TX boxes in x and up to
// b3_column() boxes in z, all this rank's.
// - A column starts at a box whose x index is a multiple of kB3TX and whose z
//   index is a multiple of the column length or whose z- neighbour is another
//   rank's.  It stops at that length, at a physical z+ face, below another
//   rank's box and below the next column's first box (where a periodic z
//   extent is no multiple of the length, the last column is shorter).
// - Around every z slot (the box below, the column's boxes, the box above) stand
//   the 3 x (kB3TX+2) boxes of the tile's row and the rows beside it in y, each
//   named by its slot in the arena: a local index, or n + its position among
//   the deep halo's proxies.  A physical face (round 6) is a flag of the column,
//   alike for all its boxes; the slot across it names the box whose face it is.
// - Order: z block, then Morton order in x / y, so that each XCD's run of
//   workgroups (xcd_box) is one compact patch whose halo columns its own L2
//   holds; columns of equal key (a rank boundary inside a z block) keep the
//   order of their first boxes in the level's id list.
// - Declined (no records; the one-substep kernels serve the level): boxes not
//   16^3, a replicated level, fewer than b3_min_boxes boxes, boxes past
//   k_gsrb3's 32-bit byte offsets, a face that is neither this rank's box nor
//   physical, or columns that do not fit (walk_columns' reasons).  A split
//   level that plan_deep (omg_plan.cpp) declared deep, alike on every rank,
//   must fit: there a reason is an error.
#include <algorithm>

#include "omg_host.h"

namespace omg {
namespace host {

// whether k_gsrb3's 32-bit byte offsets reach every box of a variable
// (omg_block.hip b3_ld / b3_st): 95,325 boxes of 16^3 at most
static bool block3_addressable(long long n_boxes, long long stride) {
  return (unsigned long long)n_boxes * (unsigned long long)stride * 8ull <= 0xFFFFFFFFull;
}

// boxes per column in z: 16 on levels of >= 32768 boxes, 4 down to 4096, below
// that (levels that take the passes with OMG_BLOCK3_MIN_BOXES lowered) 2, for
// more workgroups (OMG_BLOCK3_SMALL_COL); OMG_BLOCK3_COLUMN: all levels.
// C3's level 1: 857 / 759 us per pass with 16 against 875 / 772 with 8 (1024
// workgroups, fewer halo planes per box; profiles/r05/s40_block3_z16_ab.txt)
// and 898 / 789 with 4 (s38); on its 4096-box level 8 gained nothing, and
// two-box columns, twice the workgroups, took 110 us a pass against 102
static int b3_column(const omg_ctx* c, int n) {
  if (c->b3_col) return c->b3_col;
  return n / (kB3TX * 8) >= 2048 ? 16 : (n >= kB3MinBoxes ? 4 : c->b3_col_small);
}

namespace {
// The boxes of a level as the tables see them, by global id; face f: 0 x-,
// 1 x+, 2 y-, 3 y+, 4 z-, 5 z+.
struct Boxes {
  Tree T;
  const Level& L;
  bool phys(int id, int f) const { return T.nbr(id, f + 1) < 0; }
  // the neighbour across a face; across a physical face the box itself
  int nbr(int id, int f) const { return phys(id, f) ? id : T.nbr(id, f + 1); }
  bool mine(int id) const { return T.rank(id) == T.c->rank; }
  int ix(int id, int d) const { return T.c->ix[(size_t)(id - 1) * 3 + d] - 1; }
  // where the box stands in L's arena: its local index, n + its position
  // among the proxies, or -1 (another rank's box that is no proxy)
  int slot(int id) const {
    if (mine(id)) return T.c->local_index[id];
    auto it = std::lower_bound(L.prox_ids.begin(), L.prox_ids.end(), id);
    return it != L.prox_ids.end() && *it == id ? L.n + (int)(it - L.prox_ids.begin()) : -1;
  }
  int id(int slot) const { return slot < L.n ? L.ids[slot] : L.prox_ids[slot - L.n]; }
  // (in slots; -1: no box of the level there, or one outside the arena)
  int nbr_slot(int slot, int f) const {
    const int n = slot < 0 ? 0 : T.nbr(id(slot), f + 1);
    return n > 0 ? this->slot(n) : -1;
  }
};
}  // namespace

static unsigned long long spread(unsigned v) {
  unsigned long long r = 0;
  for (int q = 0; q < 20; q++) r |= (unsigned long long)((v >> q) & 1u) << (2 * q);
  return r;
}

// L's column records in their order (h_b3) and whether a column has a
// physical face (b3_phys); returns null, or why the level does not fit.
static const char* walk_columns(omg_ctx* c, Level& L) {
  const Boxes B{Tree{c}, L};
  bool any_phys = false;
  const int nzb = b3_column(c, L.n);
  static_assert(kB3MaxZ >= 16, "column records hold 16 boxes");
  std::vector<std::pair<unsigned long long, std::vector<int>>> cols;
  std::vector<int> covered(L.n, 0);
  for (int h : L.ids) {
    if (B.ix(h, 0) % kB3TX || (B.ix(h, 2) % nzb && B.mine(B.nbr(h, 4)))) continue;
    std::vector<int> zc{h};
    while ((int)zc.size() < nzb && !B.phys(zc.back(), 5)) {
      const int up = B.nbr(zc.back(), 5);
      if (!B.mine(up) || B.ix(up, 2) % nzb == 0) break;   // another rank's, or the next column's first box
      zc.push_back(up);
    }
    const int len = (int)zc.size();
    // the column's physical faces: x-, x+, y-, y+ alike for all its boxes (and
    // none between the tile's boxes), z- of its first box, z+ of its last
    int fl = (B.phys(zc[0], 4) ? 16 : 0) | (B.phys(zc[len - 1], 5) ? 32 : 0);
    for (int z = 0; z < len; z++) {
      int t[kB3TX];
      t[0] = zc[z];
      for (int xs = 1; xs < kB3TX; xs++) {
        if (B.phys(t[xs - 1], 1)) return "a physical face inside a tile";
        t[xs] = B.nbr(t[xs - 1], 1);
      }
      int f = (B.phys(t[0], 0) ? 1 : 0) | (B.phys(t[kB3TX - 1], 1) ? 2 : 0);
      for (int xs = 0; xs < kB3TX; xs++) {
        const int fy = (B.phys(t[xs], 2) ? 4 : 0) | (B.phys(t[xs], 3) ? 8 : 0);
        if (xs && fy != (f & 12)) return "physical faces differ inside a tile";
        f |= fy;
      }
      if (z && f != (fl & 15)) return "physical faces differ along a column";
      fl |= f;
    }
    any_phys |= fl != 0;
    std::vector<int> r(kB3Rec, 0);
    r[0] = len | fl << 8;
    for (int zs = 0; zs <= len + 1; zs++) {
      const int cb = zs == 0 ? B.nbr(zc[0], 4) : (zs == len + 1 ? B.nbr(zc[len - 1], 5) : zc[zs - 1]);
      // the tile's row of boxes along x, then the rows below and above it in
      // y; a grid: the rows' x neighbours agree with the y neighbours' chain
      // (except where a slot stands across a physical face)
      int g[3][kB3TX + 2];
      g[1][0] = B.nbr(cb, 0);
      for (int xs = 1; xs <= kB3TX + 1; xs++) g[1][xs] = xs == 1 ? cb : B.nbr(g[1][xs - 1], 1);
      for (int xs = 0; xs < kB3TX + 2; xs++) {
        g[0][xs] = B.nbr(g[1][xs], 2);
        g[2][xs] = B.nbr(g[1][xs], 3);
      }
      for (int ys = 0; ys < 3; ys += 2)
        for (int xs = (fl & 1) ? 1 : 0; xs + 1 < kB3TX + ((fl & 2) ? 1 : 2); xs++)
          if (B.nbr(g[ys][xs], 1) != g[ys][xs + 1]) return "the rows around a column are no grid";
      for (int ys = 0; ys < 3; ys++)
        for (int xs = 0; xs < kB3TX + 2; xs++) {
          const int s = B.slot(g[ys][xs]);
          if (zs >= 1 && zs <= len && ys == 1 && xs >= 1 && xs <= kB3TX) {
            if (!B.mine(g[ys][xs])) return "a column box on another rank";
            covered[s]++;
          }
          if (s < 0) return "a column reads a box outside the proxies";
          r[1 + kB3S * zs + (kB3TX + 2) * ys + xs] = s;
        }
    }
    const unsigned long long key = ((unsigned long long)(B.ix(h, 2) / nzb) << 40) |
                                   (spread((unsigned)(B.ix(h, 0) / kB3TX)) | (spread((unsigned)B.ix(h, 1)) << 1));
    cols.emplace_back(key, std::move(r));
  }
  for (int b = 0; b < L.n; b++)
    if (covered[b] != 1) return "the columns do not cover the level once";
  std::stable_sort(cols.begin(), cols.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  L.h_b3.reserve(cols.size() * kB3Rec);
  for (auto& cr : cols) L.h_b3.insert(L.h_b3.end(), cr.second.begin(), cr.second.end());
  L.b3_phys = any_phys;
  return nullptr;
}

// L's column records and phi's second buffer, after its face tables.  One GPU:
// a level that does not fit gets none.  A level plan_deep declared deep must fit.
void build_columns(omg_ctx* c, Level& L) {
  if (L.nc != 16 || L.replicated) return;
  if (!L.deep) {
    if (L.n < c->b3_min_boxes || !block3_addressable(L.n, L.stride)) return;
    for (int8_t k : L.h_nbk)
      if (k != NB_LOCAL && !(k == NB_PHYS && !c->no_block3_phys)) return;
  }
  if (const char* why = walk_columns(c, L)) {
    if (L.deep) throw OmgError(std::string("plan_deep: ") + why);
    return;
  }
  L.n_b3 = (int)(L.h_b3.size() / kB3Rec);
  L.d_b3 = to_device(L.h_b3);
  if (L.n_b3) dmalloc(&L.d_phi_buf, sizeof(double) * (size_t)(L.n + L.n_prox) * L.stride, true);
}

// The ghost terms of the block passes' physical faces: bc_to_gc's c0 * b, c1,
// c2 per face (m_ghost_cells.f90:665-766; k_gsrb_tile's phys_ghost, the same
// expressions), for constant boundary values only; false when the level's
// are tabulated (a boundary callback) or stored with phi.
static bool b3_phys_args(omg_ctx* c, int lvl, const Level& L, B3Phys& P) {
  if (c->phi_bc_data_stored) return false;
  auto it = c->d_face_off_lvl[0].find(lvl);
  if (it != c->d_face_off_lvl[0].end() && it->second) return false;
  for (int nb = 1; nb <= 6; nb++) {
    const int type = c->bc[0].type[nb - 1];
    const double bv = c->bc[0].value[nb - 1];
    double c0, c1, c2;
    if (type == OMG_BC_DIRICHLET) {
      c0 = 2; c1 = -1; c2 = 0;
    } else if (type == OMG_BC_NEUMANN) {
      c0 = L.dr[(nb - 1) >> 1] * ((nb & 1) ? -1.0 : 1.0); c1 = 1; c2 = 0;
    } else {
      c0 = 0; c1 = 2; c2 = -1;
    }
    P.k[nb - 1] = c0 * bv;
    P.c1[nb - 1] = c1;
    P.c2[nb - 1] = c2;
  }
  return true;
}

// whether a block pass (k_gsrb3 / k_gsrb4) may smooth the level now: records,
// consistent ghosts, an operator it has; ph: its physical faces' terms (null:
// none), P their storage
bool b3_usable(omg_ctx* c, int lvl, B3Phys& P, const B3Phys*& ph) {
  const Level* L = level_ptr(c, lvl);
  ph = nullptr;
  if (!L || !L->d_b3 || !(L->phi_gc_ok || (L->gc_deferred && !L->b3_phys)) || !gsrb3_op_ok(c->op) ||
      c->no_block3)
    return false;
  if (L->b3_phys) {
    if (!b3_phys_args(c, lvl, *L, P)) return false;
    ph = &P;
  }
  return true;
}

// k_gsrb3's correct_children form (launch_gsrb3's ccols) for the columns of F:
// every column of an even number of boxes starts at a coarse box's corner in x
// and z, its fine boxes are the children of its coarse boxes, and every coarse
// box is the own box of exactly two columns (its two halves in y), on a
// coarse level of 16^3 boxes whose faces are all same-GPU boxes; on a split
// level (deep halo on both levels) a box on another rank stands for its proxy
// in C's arena (deep_res fills its res).  (After the grid transfers of F.)
void build_coarse_columns(omg_ctx* c, Level& F, const Level& C) {
  if (F.h_b3.empty() || C.nc != 16 || C.replicated || C.n == 0 || F.n != 8 * C.n || F.deep != C.deep) return;
  if (!block3_addressable(C.n + C.n_prox, C.stride)) return;
  if (!F.deep)
    for (int8_t k : C.h_nbk)
      if (k != NB_LOCAL) return;
  for (int b = 0; b < F.n; b++)
    if (F.parent_local[b] < 0) return;
  const Boxes B{Tree{c}, C};
  auto dix = [&](int b, int q) { return (F.dix_packed[b] >> (10 * q)) & 1023; };
  std::vector<int> out((size_t)F.n_b3 * kB3CRec, 0);
  std::vector<int> own(C.n, 0);
  for (int q = 0; q < F.n_b3; q++) {
    const int* r = &F.h_b3[(size_t)q * kB3Rec];
    if (r[0] > kB3LenMask) return;   // (physical faces: the plain passes only)
    const int len = r[0], lenc = len / 2;
    if (len % 2) return;
    auto fine = [&](int zs, int xs) { return r[1 + kB3S * zs + (kB3TX + 2) + xs]; };
    const int b0 = fine(1, 1);
    if (dix(b0, 0) != 0 || dix(b0, 2) != 0) return;
    int* o = &out[(size_t)q * kB3CRec];
    o[0] = dix(b0, 1);
    int zc[kB3MaxZ / 2 + 2];
    zc[1] = F.parent_local[b0];
    for (int z = 2; z <= lenc; z++) {
      zc[z] = B.nbr_slot(zc[z - 1], 5);
      if (zc[z] < 0 || zc[z] >= C.n) return;   // (a column's coarse boxes are this rank's)
    }
    zc[0] = B.nbr_slot(zc[1], 4);
    zc[lenc + 1] = B.nbr_slot(zc[lenc], 5);
    for (int z = 0; z <= lenc + 1; z++) {
      int* row = o + 1 + 9 * z;
      row[4] = zc[z];
      row[3] = B.nbr_slot(zc[z], 0);
      row[5] = B.nbr_slot(zc[z], 1);
      for (int xs = 0; xs < 3; xs++) {
        row[xs] = B.nbr_slot(row[3 + xs], 2);
        row[6 + xs] = B.nbr_slot(row[3 + xs], 3);
      }
      for (int q2 = 0; q2 < 9; q2++)
        if (row[q2] < 0) return;
      for (int ys = 0; ys < 3; ys += 2)
        for (int xs = 0; xs < 2; xs++)
          if (B.nbr_slot(row[3 * ys + xs], 1) != row[3 * ys + xs + 1]) return;
      if (z >= 1 && z <= lenc) own[zc[z]]++;
    }
    for (int zs = 1; zs <= len; zs++)
      for (int xs = 1; xs <= kB3TX; xs++) {
        const int fb = fine(zs, xs);
        if (F.parent_local[fb] != zc[(zs + 1) / 2] || dix(fb, 0) != (xs - 1) * 8 || dix(fb, 1) != o[0] ||
            dix(fb, 2) != ((zs - 1) & 1) * 8)
          return;
      }
  }
  for (int b = 0; b < C.n; b++)
    if (own[b] != 2) return;
  F.d_b3c = to_device(out);
  F.h_b3c = std::move(out);
}

// k_gsrb3 / k_gsrb4's correction form on split levels: which path the
// up-smoothing takes decides collective rounds (the deep halo of both levels,
// deep_res), and whether the coarse records could be built depends on each
// rank's boxes, so the ranks agree: every rank holding boxes of the level must
// have them, else none uses them (a plan-only context keeps what it built)
void agree_columns(omg_ctx* c) {
  if (c->n_ranks > 1 && !c->host_only)
    for (int l = c->lowest + 1; l <= c->highest; l++) {
      Level& F = c->levels[l];
      if (!F.deep) continue;
      const bool fail = F.n > 0 && F.h_b3c.empty();
      if (allreduce(c, fail ? 1.0 : 0.0, true) > 0.5) {
        dfree(F.d_b3c);
        F.h_b3c.clear();
      }
    }
}

const std::vector<int>& columns_host(const Level& L, int which, int* rec_ints) {
  *rec_ints = which ? kB3CRec : kB3Rec;
  return which ? L.h_b3c : L.h_b3;
}

}  // namespace host
}  // namespace omg
