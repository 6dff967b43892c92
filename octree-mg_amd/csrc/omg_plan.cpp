// omg_plan.cpp — what omg_tree_setup builds on one rank from the tree: the
// levels' arenas and face tables, the communication plans of every exchange
// and the deep halo of split levels (the block kernels' tables: omg_columns.cpp).
#include <algorithm>

#include "omg_host.h"

namespace omg {
namespace host {

// Level::d_topo, the per-box face words the tiled kernels load once
// (FaceTopo, omg_face.h), from the host tables; rebuilt when they change
// (phi_bc_store rewrites the physical faces' codes)
void pack_topo(Level& L) {
  if (!L.n) return;
  std::vector<int> w((size_t)L.n * 8, 0);
  auto put = [](int kind, long long arg) {
    if (arg < 0 || arg >= (1ll << 29)) throw OmgError("pack_topo: face argument out of range");
    return (int)(((unsigned)kind << 29) | (unsigned)arg);
  };
  for (int b = 0; b < L.n; b++) {
    unsigned nonlocal = 0;
    for (int f = 0; f < 6; f++) {
      const size_t i = (size_t)b * 6 + f;
      const int kind = L.h_nbk[i];
      long long arg = 0;
      if (kind == NB_LOCAL) {
        arg = L.h_nba[i];
      } else if (kind == NB_PHYS) {
        arg = -(long long)L.h_nba[i];
      } else if (kind == NB_REMOTE) {
        arg = L.h_sendpos[i];
      } else if (kind == NB_RB) {
        const RBRec& r = L.h_rb[L.h_nba[i]];
        if (r.coarse_idx < 0 || r.coarse_idx >= (1 << 25)) throw OmgError("pack_topo: coarse index out of range");
        arg = r.coarse_idx;
        for (int d = 0; d < 3; d++) {
          if (r.dix[d] != 0 && r.dix[d] != L.nc / 2) throw OmgError("pack_topo: child offset not 0 or nc/2");
          arg |= (long long)(r.dix[d] != 0) << (25 + d);
        }
      }
      if (kind != NB_LOCAL) nonlocal |= 1u << f;
      w[(size_t)b * 8 + f] = put(kind, arg);
    }
    w[(size_t)b * 8 + 6] = (int)nonlocal;
  }
  dfree(L.d_topo);
  L.d_topo = to_device(w);
}

// Build a Transfer's device arrays from its per-peer lists.
void finalize_transfer(Transfer& T) {
  std::vector<int> s, r;
  int off = 0;
  for (auto& p : T.send) {
    p.offset = off;
    off += (int)p.items.size() / T.send_ints;
    s.insert(s.end(), p.items.begin(), p.items.end());
  }
  T.n_send = off;
  off = 0;
  for (auto& p : T.recv) {
    p.offset = off;
    off += (int)p.items.size() / T.recv_ints;
    r.insert(r.end(), p.items.begin(), p.items.end());
  }
  T.n_recv = off;
  T.d_send_items = to_device(s);
  T.d_recv_items = to_device(r);
}

std::vector<PeerList> group(std::vector<Rec>& recs, int ints_per_item) {
  std::sort(recs.begin(), recs.end(), [](const Rec& x, const Rec& y) {
    return x.peer != y.peer ? x.peer < y.peer : x.key < y.key;
  });
  std::vector<PeerList> out;
  for (auto& r : recs) {
    if (out.empty() || out.back().peer != r.peer) {
      out.push_back(PeerList());
      out.back().peer = r.peer;
    }
    out.back().keys.push_back(r.key);
    out.back().items.push_back(r.a);
    if (ints_per_item >= 2) out.back().items.push_back(r.b);
    if (ints_per_item >= 3) out.back().items.push_back(r.c);
  }
  return out;
}

static void rbh_free(Level& L) {
  for (auto& kv : L.rbh) {
    RbHostFaces& R = kv.second;
    dfree(R.d_items);
    dfree(R.d_slot);
    dfree(R.d_cgc);
    dfree(R.d_cc);
    if (R.h_cgc) (void)hipHostFree(R.h_cgc);
    if (R.h_cc) (void)hipHostFree(R.h_cc);
  }
  L.rbh.clear();
}

// the records of every level with refinement boundaries, for the variables
// and faces that have a host callback
void rbh_build(omg_ctx* c) {
  c->rbh_any = false;
  for (int iv = 0; iv < kMaxVars; iv++)
    for (int nb = 0; nb < 6; nb++) c->rbh_any |= c->rb_fn[iv][nb] != nullptr;
  for (auto& kv : c->levels) {
    Level& L = kv.second;
    rbh_free(L);
    if (!c->rbh_any || !L.has_rb || !L.n || c->host_only) continue;
    // receive slot of every NB_RBREM face (its position in the rb exchange)
    std::map<int, int> rslot;
    {
      int pos = 0;
      for (auto& p : L.rbx.recv)
        for (int f : p.items) rslot[f] = pos++;
    }
    for (int iv = 1; iv <= c->n_vars; iv++) {
      RbHostFaces R;
      for (int nb = 1; nb <= 6; nb++) {
        if (!c->rb_fn[iv - 1][nb - 1]) continue;
        for (int b = 0; b < L.n; b++) {
          const int f = b * 6 + nb - 1, kind = L.h_nbk[f];
          if (kind != NB_RB && kind != NB_RBREM) continue;
          R.items.push_back(f);
          R.slot.push_back(kind == NB_RBREM ? rslot.at(f) : -1);
          R.ids.push_back(L.ids[b]);
          R.nbs.push_back(nb);
        }
      }
      R.n = (int)R.items.size();
      if (!R.n) continue;
      const size_t nc2 = (size_t)L.nc * L.nc, per = (size_t)(L.nc + 2) * (L.nc + 2) * (L.nc + 2);
      R.d_items = to_device(R.items);
      R.d_slot = to_device(R.slot);
      dmalloc(&R.d_cgc, sizeof(double) * R.n * nc2);
      dmalloc(&R.d_cc, sizeof(double) * R.n * per);
      HIPCHK(hipHostMalloc(&R.h_cgc, sizeof(double) * R.n * nc2));
      HIPCHK(hipHostMalloc(&R.h_cc, sizeof(double) * R.n * per));
      L.rbh[iv] = std::move(R);
    }
  }
}

// ring-order rhs buffers for the levels the register-ring lexicographic
// kernel serves (allocated outside any graph capture: tree setup, smoother
// choice): 16^3 levels large enough that the sweep is bandwidth-bound; on
// smaller levels the per-cycle copies cost more than they save (rings on
// levels of >= 512 or >= 64 boxes: 0.2-2 % slower, profiles/r03/s16,
// r04/s10_gs_ring_min_ab.txt)
constexpr int kGsRingMinBoxes = 2048;
// Called whenever the smoother or the operator changes (never inside a
// capture): the buffers exist exactly on the levels the current methods use
// them on, and are freed otherwise (a 512^3 level's are ~1.1 GiB).
void ensure_rhs_lex(omg_ctx* c) {
  if (c->host_only) return;
  const bool want = c->smoother != OMG_SMOOTHER_GSRB && !c->no_gs_plane;
  for (auto& kv : c->levels) {
    Level& L = kv.second;
    if (!want || L.n < kGsRingMinBoxes || !gs_lex_ring_ok(L.nc, c->op)) {
      if (L.d_rhs_lex || L.d_xlay) HIPCHK(hipStreamSynchronize(c->stream));   // (in use by queued sweeps)
      dfree(L.d_rhs_lex);
      dfree(L.d_xlay);
      dfree(L.d_galt);
      L.rhs_lex_ok = false;
      continue;
    }
    if (L.d_rhs_lex) continue;
    dmalloc(&L.d_rhs_lex, sizeof(double) * L.n * L.nc * L.nc * L.nc);
    dmalloc(&L.d_xlay, sizeof(double) * L.n * 2 * L.nc * L.nc);
    // the two-ghost-set chains skip the fills between sweeps, so only where
    // those fills exchange nothing: no remote or refinement-boundary faces,
    // and no coarse faces owed to another rank's refinement boundaries
    // (rbx.n_send: their fill_gc_lvl calls finish_rb after every sweep)
    if (!L.has_remote && !L.has_rb && L.rbx.n_send == 0 && L.rbx.n_recv == 0)
      dmalloc(&L.d_galt, sizeof(double) * L.n * 6 * (size_t)stored_face(L.nc));
    L.rhs_lex_ok = false;
  }
}

// ---------------------------------------------------------------------------
// Plan builder (device side of mg_allocate_storage, m_allocate_storage.f90:51-99,
// and of the three buffer dry runs m_ghost_cells.f90:17-62, m_restrict.f90:
// 16-69, m_prolong.f90:16-48).
void free_levels(omg_ctx* c) {
  free_state_destroy(c);   // the FFT level belongs to the old tree
  for (auto& P : c->box_plans) P.buf.release();   // (the lists name boxes of the old tree)
  c->box_plans.clear();
  for (auto& kv : c->levels) {
    Level& L = kv.second;
    dfree(L.d_data); L.d_phi = nullptr; dfree(L.d_nbk); dfree(L.d_nba); dfree(L.d_sendpos); dfree(L.d_rb);
    dfree(L.d_topo);
    rbh_free(L);
    dfree(L.d_parents); dfree(L.d_leaves); dfree(L.d_parent_local); dfree(L.d_dix); dfree(L.d_parmask);
    dfree(L.d_rbgv);
    dfree(L.d_pairs); dfree(L.d_sendbuf); dfree(L.d_recvbuf); dfree(L.d_scratch); dfree(L.d_scratch_rhs);
    dfree(L.d_rhs_lex);
    dfree(L.d_xlay);
    dfree(L.d_galt);
    dfree(L.d_phi_buf); dfree(L.d_b3); dfree(L.d_b3c); L.n_b3 = 0; L.h_b3.clear(); L.h_b3c.clear();
    dfree(L.d_physbox);
    for (auto& P : L.dense) P.buf.release();
    L.dense.clear();
    dfree(L.d_rbsend); dfree(L.d_rbrecv); dfree(L.d_bnd); dfree(L.d_int); dfree(L.d_push0); dfree(L.d_bndface);
    for (Transfer* T : {&L.halo, &L.restr, &L.prol, &L.rbx, &L.repl, &L.deep_phi, &L.deep_rhs}) {
      dfree(T->d_send_items);
      dfree(T->d_recv_items);
    }
  }
  c->levels.clear();
  for (int iv = 0; iv < kMaxVars; iv++) {
    for (auto& kv : c->d_face_off_lvl[iv]) dfree(kv.second);
    for (auto& kv : c->d_face_type_lvl[iv]) dfree(kv.second);
    c->d_face_off_lvl[iv].clear();
    c->d_face_type_lvl[iv].clear();
    c->h_face_off_lvl[iv].clear();
    c->h_face_type_lvl[iv].clear();
    dfree(c->d_face_data[iv]);
  }
}

// ---------------------------------------------------------------------------
// Deep halo: k_gsrb3 / k_gsrb4 on a level split over GPUs.
// The reference fills the ghost layer after every substep
// (m_multigrid.f90:404-424, mg_fill_ghost_cells_lvl, m_ghost_cells.f90:131-175,
// whose remote part is one sort_and_transfer_buffers round,
// m_communication.f90:37-66).  A multi-substep pass instead reads the
// neighbours' cells up to 4 deep, so on a split level the remote boxes its
// columns read become proxy boxes of this rank (after its own boxes, in every
// variable), filled once per pass: phi of the colour the pass reads, rhs when
// it changed.  The pass then runs exactly as on one GPU; its store wave's
// pushes into proxies are dropped, and the remote faces' ghosts of this rank's
// boxes arrive by the level's halo plan after it.
//
// What travels: a proxy B is read by the columns of this rank's boxes A in
// its 26-neighbourhood; per dimension, B lies below A (its top 4 layers are
// read), above (its bottom 4) or level with A (all 16): a product of ranges,
// whose union over those A is sent as 4^3-cell bricks (launch_deep_copy).  Every rank derives the same regions from the global
// tree, so the brick lists pair up key for key (key 64*id + brick).
//
// Where: 16^3 levels, every face a box of the level (uniform, periodic or
// interior), x pairs of boxes (even ix and its x+ neighbour) on one rank, at
// least b3_min_boxes boxes on every rank holding some, and byte offsets of
// every rank's boxes + proxies under 4 GiB; decided alike on every rank.  On
// a level of leaves rhs changes only by the periodic mean, which the proxies
// follow; a level with parents gets its rhs from update_coarse every cycle,
// so its proxies' rhs travels once per cycle.  Such a level (C3's level 0 at
// N > 1) also stores res for the correction form above it (the RES pass), and
// its proxies get that res too (deep_res).  (The columns: omg_columns.cpp.)
// the box at offset o (components -1..1) from id, walking x, y, z in turn
// (zyx: the reverse order); 0 when the walk leaves the level's boxes
static int deep_walk(const Tree& T, int id, const int o[3], bool zyx = false) {
  for (int s = 0; s < 3; s++) {
    const int d = zyx ? 2 - s : s;
    if (!o[d]) continue;
    id = T.nbr(id, 2 * d + (o[d] > 0 ? 2 : 1));
    if (id <= 0) return 0;
  }
  return id;
}

template <typename F>
static void deep_offsets(F&& f) {
  for (int z = -1; z <= 1; z++)
    for (int y = -1; y <= 1; y++)
      for (int x = -1; x <= 1; x++)
        if (x || y || z) {
          const int o[3] = {x, y, z};
          f(o);
        }
}

// the bricks box B shows a box A at offset o from B (A reads B's 4 layers
// toward it, all 16 across): bit bx + 4 by + 16 bz
static unsigned long long deep_bricks(const int o[3]) {
  unsigned long long m = 0;
  for (int bz = 0; bz < 4; bz++)
    for (int by = 0; by < 4; by++)
      for (int bx = 0; bx < 4; bx++) {
        const int b[3] = {bx, by, bz};
        bool in = true;
        for (int d = 0; d < 3; d++) in &= o[d] == 0 || b[d] == (o[d] > 0 ? 3 : 0);
        if (in) m |= 1ull << (bx + 4 * by + 16 * bz);
      }
  return m;
}

// (before the level's arena is allocated: sets n_prox, which sizes it)
static void plan_deep(omg_ctx* c, Level& L) {
  const int l = L.lvl, me = c->rank;
  L.deep = false;
  L.n_prox = 0;
  L.prox_ids.clear();
  if (c->n_ranks == 1 || L.replicated || L.nc != 16 || c->no_block3 || c->no_deep) return;
  Tree T{c};
  const auto& ids = c->ids[l];
  if (ids.empty()) return;
  std::map<int, std::vector<int>> by_rank;
  bool split = false;
  for (int id : ids) {
    by_rank[T.rank(id)].push_back(id);
    for (int nb = 1; nb <= 6; nb++) {
      const int nid = T.nbr(id, nb);
      if (nid <= 0 || T.lvl(nid) != l) return;   // physical or refinement-boundary face
      split |= T.rank(nid) != T.rank(id);
    }
  }
  if (!split) return;
  auto ixd = [&](int id, int d) { return c->ix[(size_t)(id - 1) * 3 + d] - 1; };
  for (int id : ids) {
    const int odd = ixd(id, 0) & 1, pr = T.nbr(id, odd ? 1 : 2);
    if (T.rank(pr) != T.rank(id) || T.nbr(pr, odd ? 2 : 1) != id || (ixd(pr, 0) & 1) == odd) return;
    bool grid = true;
    deep_offsets([&](const int* o) { grid &= deep_walk(T, id, o) == deep_walk(T, id, o, true); });
    if (!grid) return;
  }
  // every rank: enough boxes, and its boxes + proxies addressable by k_gsrb3's
  // 32-bit byte offsets
  std::vector<int> stamp((size_t)c->n_boxes + 1, -1);
  const unsigned long long box_bytes = 8ull * (unsigned long long)(((stored_cells(16) + 63) / 64) * 64);
  for (auto& kv : by_rank) {
    if ((int)kv.second.size() < c->b3_min_boxes) return;
    long long np = 0;
    for (int id : kv.second)
      deep_offsets([&](const int* o) {
        const int b = deep_walk(T, id, o);
        if (T.rank(b) != kv.first && stamp[b] != kv.first) {
          stamp[b] = kv.first;
          np++;
        }
      });
    if ((unsigned long long)(kv.second.size() + np) * box_bytes > 0xFFFFFFFFull) return;
  }
  L.deep = true;
  // proxies (this rank reads them) and what the peers read of this rank's boxes
  // (box B at offset o from my box A: A reads B's bricks at -o from B; and
  // the peer's box B reads my A's bricks at o from A)
  std::map<int, unsigned long long> need;
  std::map<std::pair<int, int>, unsigned long long> give;
  for (int id : L.ids) {
    if (T.rank(id) != me) continue;
    deep_offsets([&](const int* o) {
      const int b = deep_walk(T, id, o), q = T.rank(b);
      if (q == me) return;
      const int mo[3] = {-o[0], -o[1], -o[2]};
      need[b] |= deep_bricks(mo);
      give[{q, id}] |= deep_bricks(o);
    });
  }
  std::vector<Rec> rs, rr;
  for (auto& kv : need) {   // (ascending ids: a proxy's slot is n + its place in prox_ids)
    for (int br = 0; br < 64; br++)
      if ((kv.second >> br) & 1) rr.push_back({T.rank(kv.first), 64LL * kv.first + br, L.n + (int)L.prox_ids.size(), br});
    L.prox_ids.push_back(kv.first);
  }
  L.n_prox = (int)L.prox_ids.size();
  for (auto& kv : give)
    for (int br = 0; br < 64; br++)
      if ((kv.second >> br) & 1)
        rs.push_back({kv.first.first, 64LL * kv.first.second + br, c->local_index[kv.first.second], br});
  for (Transfer* X : {&L.deep_phi, &L.deep_rhs}) {
    X->send = group(rs, 2);
    X->recv = group(rr, 2);
    X->send_ints = X->recv_ints = 2;
    X->item_doubles = X == &L.deep_phi ? 32 : 64;
    finalize_transfer(*X);
  }
  L.prox_rhs_ok = false;
}

namespace {

// build_plan's stages, in the order it runs them.  They share the tree, this
// rank and which boxes live here: its own and every box of a replicated level.
struct Planner {
  omg_ctx* c;
  Tree T;
  int me;
  bool owns(int id) const { return T.lvl(id) <= c->rep_lvl || T.rank(id) == me; }
  void owned_levels();
  std::vector<int> faces(int l, Level& L);
  void boundary_lists(Level& L);
  void parents_leaves(int l, Level& L);
  void grid_transfers();
  void buffers();
};

// which levels are replicated, the boxes of every level that live here
void Planner::owned_levels() {
  c->local_index.assign(c->n_boxes + 1, -1);
  // Replicated coarse levels: the lowest levels, while they hold at most
  // rep_cells cells and neither leaves nor refinement boundaries, live on every
  // rank.  Their exchanges (latency-bound at a few boxes per GPU) disappear:
  // the restriction into the highest replicated level goes to every rank, and
  // the prolongation out of it is local everywhere.  Bits do not change: each
  // box's arithmetic is the same wherever it runs, and get_sum reads leaves only.
  c->rep_lvl = INT_MIN;
  if (c->rep_cells > 0 && c->n_ranks > 1)
    for (int l = c->lowest; l < c->highest; l++) {
      const long long nc = c->bsl[l];
      if ((long long)c->ids[l].size() * nc * nc * nc > c->rep_cells || !c->leaves[l].empty() ||
          !c->ref_bnds[l].empty())
        break;
      c->rep_lvl = l;
    }
  for (int l = c->lowest; l <= c->highest; l++) {
    Level& L = c->levels[l];
    L.lvl = l;
    L.nc = c->bsl[l];
    L.replicated = l <= c->rep_lvl;
    for (int d = 0; d < 3; d++) L.dr[d] = c->drl[l][d];
    for (int id : c->ids[l])
      if (owns(id)) {
        c->local_index[id] = (int)L.ids.size();
        if (T.rank(id) == me) L.host_local.push_back((int)L.ids.size());
        L.ids.push_back(id);
      }
    L.n = (int)L.ids.size();
    L.stride = ((stored_cells(L.nc) + 63) / 64) * 64;   // 512-B aligned boxes
    if (L.replicated) {
      // the host's boxes of this level go to every peer (upload_level)
      std::vector<Rec> rs, rr;
      for (int b = 0; b < L.n; b++) {
        const int id = L.ids[b];
        if (T.rank(id) == me) {
          for (int r = 0; r < c->n_ranks; r++)
            if (r != me) rs.push_back({r, (long long)id, b, 0});
        } else {
          rr.push_back({T.rank(id), (long long)id, b, 0});
        }
      }
      L.repl.send = group(rs, 1);
      L.repl.recv = group(rr, 1);
      L.repl.item_doubles = (int)L.stride;
      finalize_transfer(L.repl);
    }
  }
}

// returns the send slot of every face (Level::h_sendpos)
std::vector<int> Planner::faces(int l, Level& L) {
  const int nc = L.nc;
  // neighbour table + halo receive plan
  L.h_nbk.assign((size_t)L.n * 6, NB_LOCAL);
  L.h_nba.assign((size_t)L.n * 6, 0);
  std::vector<Rec> hrecv, hsend, rbrecv, rbsend;
  for (int b = 0; b < L.n; b++) {
    const int id = L.ids[b];
    for (int nb = 1; nb <= 6; nb++) {
      const int nid = T.nbr(id, nb);
      const size_t f = (size_t)b * 6 + nb - 1;
      if (nid > 0) {
        if (owns(nid)) {
          L.h_nbk[f] = NB_LOCAL;
          L.h_nba[f] = c->local_index[nid];
        } else {
          L.h_nbk[f] = NB_REMOTE;
          hrecv.push_back({T.rank(nid), (long long)id * 6 + nb, (int)f, 0});
          // the neighbour sends the face of its own box toward us; we send ours
          hsend.push_back({T.rank(nid), (long long)nid * 6 + kNeighbRev[nb - 1], (int)f, 0});
        }
      } else if (nid == 0) {
        // refinement boundary: parent's neighbour at lvl-1 (fill_refinement_bnd :287-328)
        const int p_id = T.parent(id);
        const int p_nb = p_id > 0 ? T.nbr(p_id, nb) : 0;
        if (p_nb <= 0) throw OmgError("refinement boundary without coarse neighbour");
        if (!owns(p_nb)) {
          L.h_nbk[f] = NB_RBREM;
          rbrecv.push_back({T.rank(p_nb), (long long)id * 6 + nb, (int)f, 0});
          continue;
        }
        RBRec r;
        r.coarse_idx = c->local_index[p_nb];
        T.child_offset(id, r.dix);
        L.h_nbk[f] = NB_RB;
        L.h_nba[f] = (int)L.h_rb.size();
        L.h_rb.push_back(r);
      } else {
        L.h_nbk[f] = NB_PHYS;
        L.h_nba[f] = nid;
      }
    }
  }
  // coarse side of the refinement boundaries toward other ranks: my
  // ref_bnds at lvl-1 next to a refined box with children elsewhere
  // (buffer_refinement_boundaries, m_ghost_cells.f90:200-229)
  // (a replicated coarse level is on every rank: nothing to send)
  if (l > c->lowest && l - 1 > c->rep_lvl)
    for (int cid : c->ref_bnds[l - 1]) {
      if (T.rank(cid) != me) continue;
      for (int nb = 1; nb <= 6; nb++) {
        const int nid = T.nbr(cid, nb);
        if (nid <= 0 || T.child(nid, 1) <= 0) continue;
        const int rev = kNeighbRev[nb - 1];
        for (int s = 1; s <= 8; s++) {
          const int ch = T.child(nid, s);
          // children of nid on the face toward cid: child offset along the
          // normal matches the low/high side rev points to
          const int d = (nb + 1) >> 1, bit = ((s - 1) >> (d - 1)) & 1;
          if (bit != ((rev & 1) ? 0 : 1)) continue;
          if (ch <= 0 || T.rank(ch) == me) continue;
          int dd[3];
          T.child_offset(ch, dd);
          rbsend.push_back({T.rank(ch), (long long)ch * 6 + rev, c->local_index[cid], nb, pack_dix(dd)});
        }
      }
    }
  L.rbx.recv = group(rbrecv, 1);
  L.rbx.send = group(rbsend, 3);
  L.rbx.send_ints = 3;
  L.rbx.recv_ints = 1;
  L.rbx.item_doubles = nc * nc;
  finalize_transfer(L.rbx);
  L.halo.recv = group(hrecv, 1);
  L.halo.send = group(hsend, 1);
  L.halo.send_ints = L.halo.recv_ints = 1;
  L.halo.item_doubles = nc * nc;
  // receive slot of every remote face = its position in the receive buffer;
  // send slot = its position in the send buffer (wire order of each peer)
  std::vector<int> sendpos((size_t)L.n * 6, -1);
  {
    int pos = 0;
    for (auto& p : L.halo.recv)
      for (int f : p.items) L.h_nba[f] = pos++;
    pos = 0;
    for (auto& p : L.halo.send)
      for (int f : p.items) sendpos[f] = pos++;
  }
  finalize_transfer(L.halo);
  L.has_rb = !L.h_rb.empty() || L.rbx.n_recv > 0;
  L.has_remote = L.halo.n_send || L.halo.n_recv;
  L.has_phys = std::any_of(L.h_nbk.begin(), L.h_nbk.end(), [](int8_t k) { return k == NB_PHYS; });
  // (tiled box sizes: the red-black smoother's coarse-part buffer, for the
  // faces whose coarse box is on this GPU)
  if (!L.h_rb.empty() && !c->host_only && !c->no_rbgv &&
      (L.nc == 16 || L.nc == 8 || L.nc == 4 || L.nc == 2))
    dmalloc(&L.d_rbgv, sizeof(double) * L.n * 6 * L.nc * L.nc);
  L.rbgv_ok = false;
  {
    std::vector<int> pb;
    for (int b = 0; b < L.n; b++)
      for (int nb = 0; nb < 6; nb++)
        if (L.h_nbk[(size_t)b * 6 + nb] == NB_PHYS) {
          pb.push_back(b);
          break;
        }
    L.n_physbox = (int)pb.size();
    L.d_physbox = to_device(pb);
  }
  L.any_rb = L.any_phys = L.any_rbx = false;
  for (int id : c->ids[l])
    for (int nb = 1; nb <= 6; nb++) {
      const int nid = T.nbr(id, nb);
      L.any_rb |= nid == 0;
      L.any_phys |= nid < 0;
      if (nid == 0) {   // the coarse box across: the parent's neighbour
        const int p_id = c->parent[id - 1];
        const int p_nb = p_id > 0 ? T.nbr(p_id, nb) : 0;
        L.any_rbx |= p_nb > 0 && !(l - 1 <= c->rep_lvl) && c->rank_of[p_nb - 1] != c->rank_of[id - 1];
      }
    }
  return sendpos;
}

void Planner::boundary_lists(Level& L) {
  // boxes with a face toward another GPU (halo overlap in smooth_boxes)
  std::vector<int> bnd, in;
  for (int b = 0; b < L.n; b++) {
    bool r = false;
    for (int nb = 0; nb < 6; nb++) r |= L.h_nbk[(size_t)b * 6 + nb] == NB_REMOTE;
    (r ? bnd : in).push_back(b);
  }
  if (!bnd.empty()) {
    L.n_bnd = (int)bnd.size();
    L.n_int = (int)in.size();
    L.d_bnd = to_device(bnd);
    L.d_int = to_device(in);
    std::vector<uint8_t> isb(L.n, 0), push0(L.n, 0);
    for (int b : bnd) isb[b] = 1;
    for (int b : in)
      for (int nb = 0; nb < 6; nb++)
        if (L.h_nbk[(size_t)b * 6 + nb] == NB_LOCAL && isb[L.h_nba[(size_t)b * 6 + nb]]) push0[b] |= 1u << nb;
    L.d_push0 = to_device(push0);
    std::vector<int> bf;
    for (int b : bnd)
      for (int nb = 0; nb < 6; nb++)
        if (L.h_nbk[(size_t)b * 6 + nb] == NB_PHYS || L.h_nbk[(size_t)b * 6 + nb] == NB_RB) {
          bf.push_back(b);
          break;
        }
    L.n_bndface = (int)bf.size();
    L.d_bndface = to_device(bf);
  }
}

void Planner::parents_leaves(int l, Level& L) {
  // parents / leaves (my_parents, my_leaves) as local indices
  for (int id : c->parents[l])
    if (owns(id)) L.parents.push_back(c->local_index[id]);
  for (int id : c->leaves[l])
    if (owns(id)) L.leaves.push_back(c->local_index[id]);
  L.d_parents = to_device(L.parents);
  L.d_leaves = to_device(L.leaves);
  {
    std::vector<uint8_t> pm(L.n, 0);
    for (int b : L.parents) pm[b] = 1;
    L.d_parmask = to_device(pm);
  }
  dmalloc(&L.d_scratch, sizeof(double) * L.leaves.size());
  dmalloc(&L.d_scratch_rhs, sizeof(double) * L.leaves.size());
  L.all_parents = L.n > 0 && (int)L.parents.size() == L.n;
}

void Planner::grid_transfers() {
  // grid transfers between lvl-1 (coarse) and lvl (fine)
  for (int l = c->lowest + 1; l <= c->highest; l++) {
    Level& F = c->levels[l];
    Level& C = c->levels[l - 1];
    const int nc = F.nc, hnc = nc / 2;
    F.parent_local.assign(F.n, -1);
    F.dix_packed.assign(F.n, 0);
    std::vector<int> pairs;
    std::vector<Rec> rsend, rrecv, psend, precv;
    for (int b = 0; b < F.n; b++) {
      const int id = F.ids[b], p = T.parent(id);
      int d[3];
      T.child_offset(id, d);
      F.dix_packed[b] = pack_dix(d);
      int slot = 0;
      for (int s = 1; s <= 8; s++)
        if (T.child(p, s) == id) slot = s;
      if (owns(p)) {
        F.parent_local[b] = c->local_index[p];
        pairs.push_back(b);
        // a replicated parent of a distributed child: every peer restricts
        // into its own copy of the parent
        if (C.replicated && !F.replicated)
          for (int r = 0; r < c->n_ranks; r++)
            if (r != me) rsend.push_back({r, (long long)p * 8 + slot, b, 0});
      } else {
        rsend.push_back({T.rank(p), (long long)p * 8 + slot, b, 0});   // restrict_set_buffer
        precv.push_back({T.rank(p), (long long)id, b, 0});             // prolong_onto remote
      }
    }
    for (int pb = 0; pb < C.n; pb++) {
      const int p = C.ids[pb];
      for (int s = 1; s <= 8; s++) {
        const int ch = T.child(p, s);
        if (ch <= 0 || owns(ch)) continue;
        int d[3];
        T.child_offset(ch, d);
        rrecv.push_back({T.rank(ch), (long long)p * 8 + s, pb, pack_dix(d)});   // restrict_onto
        // (the child's owner holds a replicated parent itself)
        if (!C.replicated) psend.push_back({T.rank(ch), (long long)ch, pb, pack_dix(d)});   // prolong_set_buffer
      }
    }
    F.restr.send = group(rsend, 1);
    F.restr.recv = group(rrecv, 2);
    F.restr.send_ints = 1;
    F.restr.recv_ints = 2;
    F.restr.item_doubles = hnc * hnc * hnc;
    finalize_transfer(F.restr);
    F.prol.send = group(psend, 2);
    F.prol.recv = group(precv, 1);
    F.prol.send_ints = 2;
    F.prol.recv_ints = 1;
    F.prol.item_doubles = nc * nc * nc;
    finalize_transfer(F.prol);
    F.n_pairs = (int)pairs.size();
    F.d_pairs = to_device(pairs);
    F.d_parent_local = to_device(F.parent_local);
    F.d_dix = to_device(F.dix_packed);
    // k_prolong_smooth needs, for every same-GPU fine face whose neighbour has
    // another parent, that parent on this GPU as the coarse neighbour (boxes
    // with a face on another GPU are not fused)
    F.prolong_smooth_ok = F.n > 0 && F.n_pairs == F.n;
    const bool one_child = C.nc * 2 == F.nc;
    for (int b = 0; b < F.n && F.prolong_smooth_ok; b++) {
      bool remote = false;
      for (int nb = 0; nb < 6; nb++) remote |= F.h_nbk[(size_t)b * 6 + nb] == NB_REMOTE;
      if (remote) continue;   // takes correct + fill + the substep (prolong_smooth())
      int d[3];
      T.child_offset(F.ids[b], d);
      for (int nb = 1; nb <= 6; nb++) {
        const int kind = F.h_nbk[(size_t)b * 6 + nb - 1];
        if (kind == NB_PHYS || kind == NB_RB) continue;   // (formed from the box's own cells)
        if (kind != NB_LOCAL) { F.prolong_smooth_ok = false; break; }
        const bool low = nb & 1;
        const bool sib = !one_child && (low ? d[(nb - 1) >> 1] == F.nc / 2 : d[(nb - 1) >> 1] == 0);
        if (!sib && C.h_nbk[(size_t)F.parent_local[b] * 6 + nb - 1] != NB_LOCAL) {
          F.prolong_smooth_ok = false;
          break;
        }
      }
    }
    build_coarse_columns(c, F, C);
  }
}

void Planner::buffers() {
  // communication buffers, sized for the largest transfer touching each level
  if (c->n_ranks > 1) {
    std::map<int, size_t> sendn, recvn;
    for (int l = c->lowest; l <= c->highest; l++) {
      Level& L = c->levels[l];
      auto upd = [](std::map<int, size_t>& m, int k, size_t v) { m[k] = std::max(m[k], v); };
      upd(sendn, l, (size_t)L.halo.n_send * L.halo.item_doubles);
      upd(recvn, l, (size_t)L.halo.n_recv * L.halo.item_doubles);
      upd(sendn, l, (size_t)L.repl.n_send * L.repl.item_doubles);
      upd(recvn, l, (size_t)L.repl.n_recv * L.repl.item_doubles);
      upd(sendn, l, (size_t)L.deep_rhs.n_send * L.deep_rhs.item_doubles);
      upd(recvn, l, (size_t)L.deep_rhs.n_recv * L.deep_rhs.item_doubles);
      if (l > c->lowest) {
        upd(sendn, l, (size_t)L.restr.n_send * L.restr.item_doubles);      // fine side packs
        upd(recvn, l - 1, (size_t)L.restr.n_recv * L.restr.item_doubles);  // coarse side receives
        upd(sendn, l - 1, (size_t)L.prol.n_send * L.prol.item_doubles);    // coarse side packs
        upd(recvn, l, (size_t)L.prol.n_recv * L.prol.item_doubles);        // fine side receives
      }
    }
    for (int l = c->lowest; l <= c->highest; l++) {
      Level& L = c->levels[l];
      L.sendbuf_doubles = sendn[l];
      L.recvbuf_doubles = recvn[l];
      dmalloc(&L.d_sendbuf, sizeof(double) * sendn[l]);
      dmalloc(&L.d_recvbuf, sizeof(double) * recvn[l]);
      dmalloc(&L.d_rbsend, sizeof(double) * (size_t)L.rbx.n_send * L.rbx.item_doubles);
      dmalloc(&L.d_rbrecv, sizeof(double) * (size_t)L.rbx.n_recv * L.rbx.item_doubles);
    }
  }
}

}  // namespace

void build_plan(omg_ctx* c) {
  Planner P{c, Tree{c}, c->rank};
  P.owned_levels();
  for (int l = c->lowest; l <= c->highest; l++) {
    Level& L = c->levels[l];
    // deep halo on a split level (k_gsrb3 / k_gsrb4 there): the proxies
    // extend every variable of the arena
    plan_deep(c, L);
    // arena
    if (L.n) {
      const size_t bytes = sizeof(double) * (size_t)c->n_vars * (L.n + L.n_prox) * L.stride;
      dmalloc(&L.d_data, bytes, true);
      L.d_phi = L.d_data;
      if (c->debug && !g_host_only) {   // (L.view() needs only the arena fields here)
        launch_poison_ghosts(L.view(), c->n_vars, snan_value(), nullptr);
        HIPCHK(hipDeviceSynchronize());
      }
    }
    const std::vector<int> sendpos = P.faces(l, L);
    P.boundary_lists(L);
    L.d_phi = L.d_data;
    build_columns(c, L);
    L.d_sendpos = to_device(sendpos);
    L.d_nbk = to_device(L.h_nbk);
    L.d_nba = to_device(L.h_nba);
    L.d_rb = to_device(L.h_rb);
    L.h_sendpos = sendpos;
    pack_topo(L);
    P.parents_leaves(l, L);
  }
  P.grid_transfers();
  P.buffers();
  agree_columns(c);
  ensure_rhs_lex(c);
  rbh_build(c);
}

}  // namespace host
}  // namespace omg
