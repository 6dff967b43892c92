// omg_cycle.cpp — the per-level steps (ghost fills, deep-halo rounds,
// smoothing, residual, restriction, prolongation, correction), the coarse
// tail, and the FAS V-cycle / FMG / captured-graph driver built from them.
//
// The control flow of every routine follows the reference routine named in
// its comment (FermiQ/octree-mg, src/m_multigrid.f90 etc.); each per-box loop
// of the reference is one level-wide kernel launch here, and every MPI
// exchange of the reference (m_communication.f90:37-66) is one grouped RCCL
// send/recv round over xGMI carrying device-packed buffers.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "omg_host.h"

namespace omg {
namespace host {

// ---------------------------------------------------------------------------
// Per-level steps
static GcBC bc_for(omg_ctx* c, int lvl, int iv) {
  GcBC g;
  for (int nb = 0; nb < 6; nb++) {
    g.type[nb] = c->bc[iv - 1].type[nb];
    g.value[nb] = c->bc[iv - 1].value[nb];
  }
  auto it = c->d_face_off_lvl[iv - 1].find(lvl);
  g.face_off = it == c->d_face_off_lvl[iv - 1].end() ? nullptr : it->second;
  auto jt = c->d_face_type_lvl[iv - 1].find(lvl);
  g.face_type = jt == c->d_face_type_lvl[iv - 1].end() ? nullptr : jt->second;
  g.face_data = c->d_face_data[iv - 1];
  g.phi_stored = c->phi_bc_data_stored;
  return g;
}

// Refinement-boundary faces whose ghosts a host callback sets instead of
// sides_rb (mg%bc(nb,iv)%refinement_bnd, fill_refinement_bnd,
// m_ghost_cells.f90:321-325): after a fill of the level has run on the device
// (sides_rb included), the coarse faces and the boxes go to the host, the
// callback sets the ghosts of face nb, and they come back.  Called once per
// fill, as the reference calls it once per fill.
static void rb_host_fixup(omg_ctx* c, Level* L, int iv) {
  if (!c->rbh_any) return;
  auto it = L->rbh.find(iv);
  if (it == L->rbh.end() || it->second.n == 0) return;
  if (c->capturing) throw OmgError("refinement_bnd host callback inside a captured cycle");
  RbHostFaces& R = it->second;
  const int nc = L->nc, nc2 = nc * nc;
  const size_t per = (size_t)(nc + 2) * (nc + 2) * (nc + 2);
  launch_rbh_gather(L->view(), view_of(c, L->lvl - 1), iv, L->d_rb, R.d_items, R.d_slot, R.n, L->d_rbrecv, R.d_cgc,
                    R.d_cc, c->stream);
  HIPCHK(hipMemcpyAsync(R.h_cgc, R.d_cgc, sizeof(double) * R.n * nc2, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(R.h_cc, R.d_cc, sizeof(double) * R.n * per, hipMemcpyDeviceToHost, c->stream));
  host_sync(c, c->stream);
  for (int q0 = 0; q0 < R.n;) {   // one call per face direction (records sorted by face)
    int q1 = q0;
    while (q1 < R.n && R.nbs[q1] == R.nbs[q0]) q1++;
    const int nb = R.nbs[q0];
    auto fn = (omg_rb_fn)c->rb_fn[iv - 1][nb - 1];
    fn(c->rb_user[iv - 1][nb - 1], L->lvl, iv, q1 - q0, R.ids.data() + q0, R.nbs.data() + q0, nc,
       R.h_cgc + (size_t)q0 * nc2, R.h_cc + (size_t)q0 * per);
    q0 = q1;
  }
  HIPCHK(hipMemcpyAsync(R.d_cc, R.h_cc, sizeof(double) * R.n * per, hipMemcpyHostToDevice, c->stream));
  launch_rbh_scatter(L->view(), iv, R.d_items, R.n, R.d_cc, c->stream);
  host_sync(c, c->stream);   // (the pinned buffer is reused by the next fill)
}

// halo exchange of the faces packed by the last fill/substep kernel, then
// fill_buffered_nb (m_ghost_cells.f90:163-174, 424-454); rb_hook: the fill is
// complete here (no full fill follows), so host refinement-boundary callbacks run
static void finish_rb(omg_ctx* c, Level* L, int iv);
static void finish_halo(omg_ctx* c, Level* L, int iv, bool rb_hook = true) {
  if (c->n_ranks > 1) {
    if (L->halo.n_send || L->halo.n_recv) {
      exchange(c, L->halo, L->d_sendbuf, L->d_recvbuf, nullptr, L->lvl);
      launch_unpack_faces(L->view(), iv, L->halo.d_recv_items, L->halo.n_recv, L->d_recvbuf, c->stream);
    }
    finish_rb(c, L, iv);
  }
  if (rb_hook) rb_host_fixup(c, L, iv);
}

// refinement boundaries across ranks (buffer_refinement_boundaries,
// m_ghost_cells.f90:157-162, 200-229): coarse faces go out interpolated,
// the fine side applies sides_rb once they arrive
static void finish_rb(omg_ctx* c, Level* L, int iv) {
  if (c->n_ranks == 1) return;
  if (L->rbx.n_send || L->rbx.n_recv) {
    launch_rb_pack(view_of(c, L->lvl - 1), iv, L->rbx.d_send_items, L->rbx.n_send, L->nc, L->d_rbsend,
                   c->stream);
    exchange(c, L->rbx, L->d_rbsend, L->d_rbrecv, nullptr, L->lvl);
    launch_rb_unpack(L->view(), iv, L->rbx.d_recv_items, L->rbx.n_recv, L->d_rbrecv, c->stream);
  }
}

// mg_fill_ghost_cells_lvl (m_ghost_cells.f90:131-175): same-GPU faces are
// pushed by their owner, physical / refinement-boundary ghosts recomputed,
// remote faces packed, exchanged over RCCL and unpacked.
void fill_gc_lvl(omg_ctx* c, int lvl, int iv) {
  if (lvl < c->lowest) throw OmgError("fill_ghost_cells_lvl: lvl < lowest_lvl");
  if (lvl > c->highest) throw OmgError("fill_ghost_cells_lvl: lvl > highest_lvl");
  Level* L = level_ptr(c, lvl);
  if (!L) return;
  if (iv == 1) {   // (the ghosts it sets are read by lvl+1's interpolation)
    ready(c, lvl, kWrite);
    wrote(c, lvl, kGcAll);
  }
  if (iv == 2) rhs_ghosts_written(c, lvl);
  if (L->n) {
    Prof p(c, "fill_gc", (double)L->n * 6 * L->nc * L->nc, lvl);
    if (iv != 1 || L->has_rb || c->no_fill_tile ||
        !launch_fill_tile(L->sweep_view(), bc_for(c, lvl, iv), L->d_sendbuf, c->stream))
      launch_fill_gc(L->view(), iv, 3, view_of(c, lvl - 1), L->d_rb, bc_for(c, lvl, iv), L->d_sendbuf,
                     c->stream);
  }
  finish_halo(c, L, iv);
}

// Deep halo of a split level (plan_deep) around a k_gsrb3 / k_gsrb4 pass:
// before it, the proxies get phi of the colour the pass reads (as stored: a
// pending mean shift is subtracted by the pass from proxies and own boxes
// alike) and, when the level's rhs changed since the last fill, rhs; after
// it, the ghosts of this rank's faces toward other GPUs (nobody pushed them)
// by the level's halo plan.  Both rounds are collective: the rhs refill is
// decided by flags every rank changes alike (every rhs writer is a
// collective call, include/omg.h), checked under OMG_CHECK_COLLECTIVE.
// one round of the deep halo's bricks: variable iv (colour: phi's), w doubles each
static void deep_round(omg_ctx* c, Level* L, const Transfer& T, int iv, int colour, int w) {
  const LevelView V = L->view();
  launch_deep_copy(V, iv, colour, w, T.d_send_items, T.n_send, L->d_sendbuf, false, c->stream);
  exchange(c, T, L->d_sendbuf, L->d_recvbuf, nullptr, L->lvl);
  launch_deep_copy(V, iv, colour, w, T.d_recv_items, T.n_recv, L->d_recvbuf, true, c->stream);
}
// the ghosts of this rank's faces toward other GPUs, by the level's halo plan
static void face_round(omg_ctx* c, Level* L, int iv, hipStream_t st) {
  launch_face_pack(L->view(), iv, L->halo.d_send_items, L->halo.n_send, L->d_sendbuf, st);
  exchange(c, L->halo, L->d_sendbuf, L->d_recvbuf, st, L->lvl);
  launch_unpack_faces(L->view(), iv, L->halo.d_recv_items, L->halo.n_recv, L->d_recvbuf, st);
}
static void deep_before(omg_ctx* c, Level* L, int colour) {
  if (!L->deep) return;
  ready(c, L->lvl, kRhs);   // (its rhs round copies rhs as stored; a split level never has shifts pending)
  if (c->check_collective && (allreduce(c, L->prox_rhs_ok ? 1.0 : 0.0, true) > 0.5) != L->prox_rhs_ok)
    throw OmgError("deep halo: the rhs refill decision differs across ranks (an rhs write was not collective)");
  if (!L->prox_rhs_ok) {
    Prof p(c, "deep_rhs", (double)L->deep_rhs.n_recv * 64, L->lvl);
    deep_round(c, L, L->deep_rhs, 2, 0, 64);
    L->prox_rhs_ok = true;
  }
  Prof p(c, "deep_phi", (double)L->deep_phi.n_recv * 32, L->lvl);
  deep_round(c, L, L->deep_phi, 1, colour, 32);
}
// defer: on the comm stream, joined by the caller (faces_pending: only the
// boxes with a face on another GPU wait for it, update_coarse's residual)
static void deep_after(omg_ctx* c, Level* L, bool defer = false) {
  if (!L->deep) return;
  hipStream_t st = c->stream;
  if (defer && L->n_bnd && L->n_int) {
    HIPCHK(hipEventRecord(c->ev_bnd, c->stream));
    HIPCHK(hipStreamWaitEvent(c->stream_comm, c->ev_bnd, 0));
    st = c->stream_comm;
    L->faces_pending = true;
  }
  Prof p(c, "deep_faces", (double)L->halo.n_recv * L->nc * L->nc, L->lvl, st);
  face_round(c, L, 1, st);
  if (L->faces_pending) HIPCHK(hipEventRecord(c->ev_comm, c->stream_comm));
}
// after a deep level's RES pass (res = phi - old, stored for the correction
// form above): the proxies get res where the level above's columns read it
// (the bricks of the deep halo, both colours), and this rank's faces toward
// other GPUs get their res ghosts (the halo plan), as the pass gave the
// same-GPU ones
static void deep_res(omg_ctx* c, Level* L) {
  if (!L->deep) return;
  Prof p(c, "deep_res", (double)L->deep_rhs.n_recv * 64, L->lvl);
  deep_round(c, L, L->deep_rhs, 4, 0, 64);
  face_round(c, L, 4, c->stream);
}

// the deferred faces of deep_after have arrived (the main stream waits)
static void faces_join(omg_ctx* c, Level* L) {
  if (!L || !L->faces_pending) return;
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_comm, 0));
  L->faces_pending = false;
}

// A pass over a split level with its halo under way: the boxes with faces on
// other GPUs first (bnd), whose halo travels on the comm stream while the
// others run (rest: it reads only its own boxes' ghost faces, and none of
// those is remote; the unpack writes remote faces only, the halves `colours`).
// rest is queued before the exchange is issued: the exchange may wait on the
// host (the loopback transport waits for its peer's message), and rest needs
// nothing from it.
template <class Bnd, class Rest>
static void split_overlap(omg_ctx* c, Level* L, int colours, Bnd bnd, Rest rest) {
  bnd();
  HIPCHK(hipEventRecord(c->ev_bnd, c->stream));
  rest();
  HIPCHK(hipStreamWaitEvent(c->stream_comm, c->ev_bnd, 0));
  exchange(c, L->halo, L->d_sendbuf, L->d_recvbuf, c->stream_comm, L->lvl);
  launch_unpack_faces(L->view(), 1, L->halo.d_recv_items, L->halo.n_recv, L->d_recvbuf, c->stream_comm, colours);
  HIPCHK(hipEventRecord(c->ev_comm, c->stream_comm));
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_comm, 0));
}

// smooth_boxes (m_multigrid.f90:404-424)
// want_res: the level above takes k_gsrb3's correct_children form next, which
// reads this level's res = phi - old: the last three substeps run as one
// k_gsrb3 pass that also stores it (the plain substeps first); returns whether
// that pass ran.
// block4: runs of four substeps as one k_gsrb4 pass (the down-smoothing when
// the residual + restriction run unfused after it, OMG_BLOCK4); the one that
// ends the smoothing leaves its remote faces' exchange in flight on the comm
// stream (deep_after), for update_coarse
bool smooth_boxes(omg_ctx* c, int lvl, int n_cycle, int first_substep, int skip_last, bool want_res, bool block4) {
  Level* L = level_ptr(c, lvl);
  const int n_sub = n_cycle * c->n_substeps - skip_last;
  bool res_done = false;
  if (!L) return false;
  // a pending phi shift is subtracted by the first tiled substep while it
  // loads (the values it reads are dead afterwards); otherwise applied now
  // (not next to refinement boundaries: their ghosts read the coarse level;
  // nor before a block pass with physical faces, whose ghosts take no shift)
  const bool absorb = L->shift_pending && c->smoother == OMG_SMOOTHER_GSRB && n_sub >= 1 &&
                      (L->phi_gc_ok || L->gc_deferred) && !L->has_rb && tiled_nc(L->nc) && !(L->d_b3 && L->b3_phys);
  if (!absorb) ready(c, lvl, kPhi);
  if (c->smoother != OMG_SMOOTHER_GSRB) {
    ready(c, lvl, kGhosts | kRhs | (n_sub >= 1 ? kWrite : 0));
    // the register-ring kernel reads rhs from its ring-order copy, rebuilt
    // here when a write since the last build dropped it (update_coarse for
    // the levels below the top, every entry point that may change rhs)
    const bool ring = n_sub >= 1 && L->d_rhs_lex && gs_lex_ring_ok(L->nc, c->op);
    if (ring && !L->rhs_lex_ok) {
      Prof p(c, "rhs_lex", (double)L->n * L->nc * L->nc * L->nc, lvl);
      launch_rhs_lex(L->view(), L->d_rhs_lex, c->stream);
      L->rhs_lex_ok = true;
    }
    // the register ring also writes the boxes' new x boundary layers, so the
    // fill after each sweep stages 12 KB per box instead of 32 (no
    // refinement boundaries on the level; OMG_NO_FILL_XL: the plain fill)
    const bool xlf = ring && L->d_xlay && !L->has_rb && !c->no_fill_tile && !c->no_fill_xl;
    // Round 4: an even number of ring sweeps on a level whose faces are
    // same-GPU or physical runs with no fill in between: sweep n reads the
    // ghost set sweep n-1 pushed into (the box storage's own faces for odd
    // n, d_galt for even n; every sweep after the first forms the physical
    // ghosts at load, since only the same-GPU faces are pushed), so the last
    // sweep lands in the box storage and only its physical ghosts are left to
    // form (k_phys_gc).  The reference fills after every sweep
    // (m_multigrid.f90:412-423): the same values reach the same ghosts
    // before every read.  OMG_NO_GS_DBL: the fill after every sweep.
    // (d_galt exists only where no fill of this level exchanges anything:
    // no remote faces, no refinement-boundary faces, and no coarse faces
    // this rank owes another rank's refinement boundaries, ensure_rhs_lex.)
    if (xlf && L->d_galt && n_sub % 2 == 0 && L->n && !c->no_gs_dbl) {
      const GcBC bc = bc_for(c, lvl, 1);
      double* prim = L->d_phi + 2 * (long long)L->view().hv;
      for (int n = 1; n <= n_sub; n++) {
        const bool odd = n & 1;
        GhostSets gs;
        gs.in = odd ? prim : L->d_galt;
        gs.in_stride = odd ? L->stride : 6 * (long long)stored_face(L->nc);
        gs.out = odd ? L->d_galt : prim;
        gs.out_stride = odd ? 6 * (long long)stored_face(L->nc) : L->stride;
        gs.phys_load = n > 1;
        Prof p(c, "smoother_gs", (double)L->n * L->nc * L->nc * L->nc, lvl);
        launch_gs_lex(L->view(), c->op, c->lambda, c->stream, L->d_rhs_lex, nullptr, &gs, &bc);
      }
      if (L->n_physbox) {
        Prof p(c, "fill_gc", (double)L->n_physbox * 6 * L->nc * L->nc, lvl);
        launch_phys_gc(L->view(), bc, L->d_physbox, L->n_physbox, c->stream);
      }
      wrote(c, lvl, kGcAll);
      return false;
    }
    for (int n = 1; n <= n_sub; n++) {
      if (L->n) {
        Prof p(c, "smoother_gs", (double)L->n * L->nc * L->nc * L->nc, lvl);
        launch_gs_lex(L->view(), c->op, c->lambda, c->stream, ring ? L->d_rhs_lex : nullptr,
                      xlf ? L->d_xlay : nullptr);
      }
      if (xlf) {
        wrote(c, lvl, kGcAll);
        if (L->n) {
          Prof p(c, "fill_gc", (double)L->n * 6 * L->nc * L->nc, lvl);
          launch_fill_tile_xl(L->sweep_view(), bc_for(c, lvl, 1), L->d_sendbuf, L->d_xlay, c->stream);
        }
        finish_halo(c, L, 1);
      } else {
        fill_gc_lvl(c, lvl, 1);
      }
    }
    return false;
  }
  for (int n = first_substep; n <= n_sub; n++) {
    // substep n updates the cells with i+j+k+n even, i.e. colour e = n mod 2,
    // and ends with the ghost fill; same-GPU neighbours only need colour e
    // when their ghost faces were consistent before the substep.
    // For odd box sizes the box-local colouring is not global (a ghost has the
    // colour of the cell it is read by), so nothing is pushed during the
    // substep and a full fill follows it.
    const int e = n & 1;
    const bool odd = L->nc & 1;
    const unsigned phi = n == 1 && absorb ? kPhiAbsorb : kPhi;
    const double* shift = n == 1 && absorb ? red_mean(c, 0) : nullptr;
    // substeps n, n+1, n+2 in one pass (k_gsrb3) into phi's other buffer: it
    // reads the neighbours' cells in their boxes, which equal its ghosts only
    // when they are consistent (phi_gc_ok), and writes every ghost face
    // (ph: the ghosts across physical faces, formed in the pass)
    B3Phys P3;
    const B3Phys* ph = nullptr;
    const bool b3 = b3_usable(c, lvl, P3, ph);
    if (block4 && (n_sub - n + 1) % 4 == 0 && b3 && (!ph || c->block4_phys)) {
      ready(c, lvl, phi | (ph ? kRhs : 0) | kWriteOther);   // (the form with physical faces takes no list)
      deep_before(c, L, 1 - e);
      {
        Prof p(c, "smoother_gsrb4", 2.0 * L->n * L->nc * L->nc * L->nc, lvl);
        launch_gsrb4(L->view(), other_phi(L), L->d_b3, L->n_b3, c->op, c->lambda, e, shift, c->stream, nullptr,
                     nullptr, ph, true, rhs_shifts(c, L));
      }
      wrote(c, lvl, kWriteOther | kGcAll);
      deep_after(c, L, n + 3 == n_sub);
      n += 3;
      continue;
    }
    if (n + 2 <= n_sub && b3 && !(want_res && (n_sub - n + 1) % 3 != 0)) {
      // the down-smoothing's last pass before k_smooth_resid (skip_last: it
      // runs the next substep, colour 0, and forms colour 0's ghosts itself
      // from colour 1, reading colour 1's only): push colour e = 1 alone
      // (a split level: both colours, its remote faces' ghosts arrive whole)
      const bool push1 = L->deep || !(skip_last == 1 && n + 2 == n_sub && e == 1);
      const bool res = want_res && n + 2 == n_sub && push1;
      ready(c, lvl, phi | kRhs | kWriteOther);
      deep_before(c, L, 1 - e);
      {
        Prof p(c, res ? "smoother_gsrb3r" : "smoother_gsrb3", 1.5 * L->n * L->nc * L->nc * L->nc, lvl);
        launch_gsrb3(L->view(), other_phi(L), L->d_b3, L->n_b3, c->op, c->lambda, e, shift, c->stream, push1, nullptr,
                     nullptr, 1, res, ph);
      }
      res_done = res;
      // (its ghost faces: every one, colour e's only without push1, whose
      // colour-(1-e) halves k_smooth_resid forms itself)
      wrote(c, lvl, kWriteOther | kGcAll);
      deep_after(c, L);
      if (res) deep_res(c, L);
      n += 2;
      continue;
    }
    ready(c, lvl, phi | kGhosts | kRhs | kWrite);
    if (L->n_bnd && L->n_int && !odd && tiled_nc(L->nc)) {
      const int gvm = L->d_rbgv ? (L->rbgv_ok ? 2 : 1) : 0;
      if (gvm) L->rbgv_ok = true;
      auto substep = [&](const int* boxes, int n_boxes) {
        Prof p(c, "smoother_gsrb", 0.5 * n_boxes * L->nc * L->nc * L->nc, lvl);
        launch_gs_substep(L->sweep_view(), c->op, c->lambda, e, 1 << e, view_of(c, lvl - 1), L->d_rb, L->has_rb,
                          bc_for(c, lvl, 1), L->d_sendbuf, shift, c->stream, boxes, n_boxes, L->d_rbgv, gvm);
      };
      split_overlap(c, L, 3, [&] { substep(L->d_bnd, L->n_bnd); }, [&] { substep(L->d_int, L->n_int); });
      finish_rb(c, L, 1);
      if (!L->phi_gc_ok) fill_gc_lvl(c, lvl, 1);
      else rb_host_fixup(c, L, 1);
      continue;
    }
    if (L->n) {
      Prof p(c, "smoother_gsrb", 0.5 * L->n * L->nc * L->nc * L->nc, lvl);
      // refinement-boundary coarse parts: the first substep after the level
      // below changed computes and stores them, the others read them
      const int gvm = L->d_rbgv ? (L->rbgv_ok ? 2 : 1) : 0;
      if (gvm) L->rbgv_ok = true;
      launch_gs_substep(L->sweep_view(), c->op, c->lambda, e, odd ? 0 : 1 << e, view_of(c, lvl - 1), L->d_rb,
                        L->has_rb, bc_for(c, lvl, 1), L->d_sendbuf, shift, c->stream, nullptr, 0, L->d_rbgv, gvm);
    }
    const bool full_fill = odd || !L->phi_gc_ok;
    finish_halo(c, L, 1, !full_fill);
    if (full_fill) fill_gc_lvl(c, lvl, 1);
  }
  return res_done;
}

void residual_lvl(omg_ctx* c, int lvl, unsigned long long* maxbits) {
  Level* L = level_ptr(c, lvl);
  if (!L || L->n == 0) return;
  ready(c, lvl, kPhi | kGhosts | (tiled_nc(L->nc) ? 0 : kRhs) | kResWrite);
  Prof p(c, "residual", (double)L->n * L->nc * L->nc * L->nc, lvl);
  if (tiled_nc(L->nc))
    launch_resid_restrict(L->sweep_view(), empty_view(), c->op, c->lambda, maxbits, 0, nullptr, nullptr, c->stream,
                          nullptr, 0, rhs_shifts(c, L));
  else
    launch_residual(L->view(), c->op, c->lambda, maxbits, c->stream);
}

// max over levels lo..hi of max_residual_lvl (m_multigrid.f90:296-311), this
// rank only: the levels' maxima fold into one word on the device, read back
// with one synchronisation
static double max_residual_levels(omg_ctx* c, int lo, int hi) {
  unsigned long long* d = (unsigned long long*)c->d_scalar;
  for (int l = lo; l <= hi; l++) {
    residual_lvl(c, l, c->d_maxslots);
    launch_max_fold(c->d_maxslots, d, l > lo, c->stream);
  }
  HIPCHK(hipMemcpyAsync(c->h_scalar, d, 8, hipMemcpyDeviceToHost, c->stream));
  if (c->capturing) {   // run_cycle reads it once the graph has run
    if (c->max_deferred) throw OmgError("internal: two max-residual readbacks in one captured cycle");
    c->max_deferred = true;
    return 0.0;
  }
  host_sync(c, c->stream);
  return c->h_scalar[0];
}

double max_residual_lvl(omg_ctx* c, int lvl) { return max_residual_levels(c, lvl, lvl); }

// the remote part of mg_restrict_lvl: children whose parent lives on another
// rank are restricted into a buffer, exchanged and unpacked (m_restrict.f90:
// 94-108, 196-211)
static void restrict_remote(omg_ctx* c, int iv, int lvl) {
  Level* F = level_ptr(c, lvl);
  Level* C = level_ptr(c, lvl - 1);
  if (c->n_ranks > 1 && F && C && (F->restr.n_send || F->restr.n_recv)) {
    launch_restrict_pack(F->view(), iv, F->restr.d_send_items, F->restr.n_send, F->d_sendbuf, c->stream);
    exchange(c, F->restr, F->d_sendbuf, C->d_recvbuf, nullptr, lvl);
    launch_restrict_unpack(C->view(), iv, F->restr.d_recv_items, F->restr.n_recv, F->nc / 2, C->d_recvbuf,
                           c->stream);
  }
}

// mg_restrict_lvl (m_restrict.f90:83-114)
void restrict_lvl(omg_ctx* c, int iv, int lvl) {
  if (lvl <= c->lowest) throw OmgError("cannot restrict lvl <= lowest_lvl");
  if (iv == 1) ready(c, lvl - 1, kWrite), wrote(c, lvl - 1, kGcStale);
  Level* F = level_ptr(c, lvl);
  restrict_remote(c, iv, lvl);
  if (F && F->n_pairs) {
    Prof p(c, "restrict", (double)F->n_pairs * F->nc * F->nc * F->nc, lvl);
    launch_restrict(F->view(), view_of(c, lvl - 1), iv, F->d_pairs, F->n_pairs, F->d_parent_local, F->d_dix,
                    c->stream);
  }
}

// mg_prolong (m_prolong.f90:51-85), lvl -> lvl+1
void prolong(omg_ctx* c, int lvl, int iv, int iv_to, int add) {
  if (lvl == c->highest) throw OmgError("cannot prolong highest level");
  if (lvl < c->lowest) throw OmgError("cannot prolong below lowest level");
  if (iv_to == 1) ready(c, lvl + 1, kWrite), wrote(c, lvl + 1, kGcStale);
  Level* F = level_ptr(c, lvl + 1);
  Level* C = level_ptr(c, lvl);
  const LevelView FV = view_of(c, lvl + 1), CV = view_of(c, lvl);
  if (c->n_ranks > 1 && F && C && (F->prol.n_send || F->prol.n_recv)) {
    launch_prolong_pack(CV, FV, iv, F->prol.d_send_items, F->prol.n_send, C->d_sendbuf, c->stream);
    exchange(c, F->prol, C->d_sendbuf, F->d_recvbuf, nullptr, lvl + 1);
    launch_prolong_unpack(FV, iv_to, add, F->prol.d_recv_items, F->prol.n_recv, F->d_recvbuf,
                          c->stream);
  }
  if (F && F->n_pairs) {
    Prof p(c, "prolong", (double)F->n_pairs * F->nc * F->nc * F->nc, lvl + 1);
    launch_prolong(CV, FV, iv, iv_to, add, F->d_pairs, F->n_pairs, F->d_parent_local, F->d_dix,
                   c->stream);
  }
}

// Whether the down-smoothing of level lvl can end in k_smooth_resid (its last
// substep, colour 0, fused with update_coarse's residual + restriction):
// red-black (two substeps per cycle, so the last one is colour 0),
// Laplacian / Helmholtz, 16^3 or 8^3 boxes.  Same-GPU faces: the recomputed
// ghosts read the neighbour box directly; physical and refinement-boundary
// faces (round 4; OMG_NO_FUSE_DOWN_BC: not fused): from the box's own cells.
// On a level with faces on other GPUs only the boxes without such a face fuse
// (n_int > 0); the others take the unfused substep + residual.
static bool smooth_resid_ok(omg_ctx* c, int lvl) {
  const Level* F = level_ptr(c, lvl);
  const Level* C = level_ptr(c, lvl - 1);
  // (a host refinement_bnd callback sets phi's ghosts on some faces: the
  // kernel's sides_rb would stand in for it)
  if (F) {
    const auto rbh = F->rbh.find(1);
    if (rbh != F->rbh.end() && rbh->second.n) return false;
  }
  return !c->no_fuse_down && F && C && F->n && c->smoother == OMG_SMOOTHER_GSRB && c->n_substeps == 2 &&
         c->n_cycle_down >= 1 &&
         (c->op == OP_LPL || c->op == OP_HELM) && (F->nc == 16 || F->nc == 8) &&
         !(c->no_fuse_down_bc && (F->has_rb || F->has_phys)) && (!F->has_remote || F->n_int) &&
         // Refinement-boundary faces whose coarse box is on another rank
         // exchange coarse faces after every substep (finish_rb); the fused
         // kernel forms those ghosts from the coarse box itself.  Decided
         // alike on every rank (any_rbx: the global tree).  Physical and
         // same-GPU refinement-boundary faces fuse on split levels too
         // (update_coarse: the boundary boxes' substep leaves the colour-1
         // halves of those ghosts for the fused boxes' edge taps).
         !F->any_rbx;
}

// update_coarse (m_multigrid.f90:347-384); fused: the level's last down
// substep is still to do (smooth_resid_ok), k_smooth_resid runs it
// with tail_crhs the coarse tail forms lvl-1's ghosts and coarse rhs itself
// (its top level, TailArgs::top_crhs): only the residual and the restriction here
void update_coarse(omg_ctx* c, int lvl, bool fused, bool tail_crhs, bool res_may_pend) {
  Level* F = level_ptr(c, lvl);
  // (every branch below writes res of every box of lvl, or leaves it pending
  // anew; k_resid_restrict takes the level's pending rhs shifts)
  if (F) ready(c, lvl, kPhi | kGhosts | (fused || !tiled_nc(F->nc) ? kRhs : 0) | kResWrite);
  // the coarse level's rhs and res are rewritten below; restriction overwrites
  // every box of an all-parents level (interior), and the fill below every
  // ghost face.  (Its phi is written once F's stored coarse parts were read.)
  if (Level* Cl = level_ptr(c, lvl - 1)) {
    ready(c, lvl - 1, (Cl->all_parents ? kPhiDead : kPhi) | kRhsWrite);
    wrote(c, lvl - 1, kRhsWrite);
  }
  if (F && F->n && tiled_nc(F->nc)) {
    // The stored refinement-boundary coarse parts of lvl (d_rbgv) were formed
    // from lvl-1 as it stands until the restriction below writes it, which is
    // what the fused down-substep's ghosts need; read the flag before the
    // write of lvl-1 drops it.  (The coarse boxes across those faces are
    // leaves: the restriction never writes them.)
    const bool rbgv = F->rbgv_ok;
    // residual + restriction of phi and res in one pass (omg_tiles.hip)
    ready(c, lvl - 1, kWrite), wrote(c, lvl - 1, kGcStale);
    if (fused && F->has_remote) {
      // multi-GPU: boxes with a face on another GPU take the unfused pair (the
      // substep, its halo on the comm stream, then the residual); the others
      // run fused meanwhile.  Those read their neighbours' colour-1 ghosts at
      // face edges, and some of those faces are remote: the unpack therefore
      // writes the colour-0 halves only (the colour this substep changed;
      // colour 1 is consistent since the previous substep's exchange).
      // Physical and refinement-boundary ghosts: a fused box's edge tap reads
      // its neighbour's colour-1 ghost on the neighbour's side face as it
      // stood before this substep, so the boundary boxes' substep writes only
      // the colour-0 halves of those ghosts (colours bit 2), and k_face_gc
      // forms them whole once the fused launch is done, before the boundary
      // boxes' residual reads them.
      const bool faces = F->any_phys || F->any_rb;
      split_overlap(c, F, 1, [&] {
        Prof p(c, "smoother_gsrb", 0.5 * F->n_bnd * F->nc * F->nc * F->nc, lvl);
        launch_gs_substep(F->view(), c->op, c->lambda, 0, faces ? 1 | 4 : 1, view_of(c, lvl - 1), F->d_rb,
                          F->has_rb, bc_for(c, lvl, 1), F->d_sendbuf, nullptr, c->stream, F->d_bnd, F->n_bnd,
                          rbgv ? F->d_rbgv : nullptr, rbgv ? 2 : 0);
      }, [&] {
        Prof p(c, "smooth_resid", (double)F->n_int * F->nc * F->nc * F->nc, lvl);
        if (!launch_smooth_resid(F->sweep_view(), view_of(c, lvl - 1), c->op, c->lambda, 1, F->d_parent_local,
                                 F->d_dix, c->stream, F->d_int, F->n_int, bc_for(c, lvl, 1), F->has_rb, F->has_phys,
                                 rbgv ? F->d_rbgv : nullptr))
          throw OmgError("smooth_resid: not available for this level");
      });
      if (faces && F->n_bndface) {
        Prof p(c, "face_gc", (double)F->n_bndface * 6 * F->nc * F->nc, lvl);
        launch_face_gc(F->view(), view_of(c, lvl - 1), bc_for(c, lvl, 1), F->d_bndface, F->n_bndface, c->stream);
      }
      {
        Prof p(c, "resid_restrict", (double)F->n_bnd * F->nc * F->nc * F->nc, lvl);
        launch_resid_restrict(F->sweep_view(), view_of(c, lvl - 1), c->op, c->lambda, nullptr, 1, F->d_parent_local,
                              F->d_dix, c->stream, F->d_bnd, F->n_bnd, rhs_shifts(c, F));
      }
    } else if (fused) {
      Prof p(c, "smooth_resid", (double)F->n * F->nc * F->nc * F->nc, lvl);
      if (!launch_smooth_resid(F->sweep_view(), view_of(c, lvl - 1), c->op, c->lambda, 1, F->d_parent_local,
                               F->d_dix, c->stream, nullptr, 0, bc_for(c, lvl, 1), F->has_rb, F->has_phys,
                               rbgv ? F->d_rbgv : nullptr))
        throw OmgError("smooth_resid: not available for this level");
    } else if (F->faces_pending) {
      // a split level's k_gsrb4 pass left its remote faces' ghosts in flight
      // (deep_after): the boxes without such a face first
      {
        Prof p(c, "resid_restrict", (double)F->n_int * F->nc * F->nc * F->nc, lvl);
        launch_resid_restrict(F->sweep_view(), view_of(c, lvl - 1), c->op, c->lambda, nullptr, 1, F->d_parent_local,
                              F->d_dix, c->stream, F->d_int, F->n_int, rhs_shifts(c, F));
      }
      faces_join(c, F);
      {
        Prof p(c, "resid_restrict", (double)F->n_bnd * F->nc * F->nc * F->nc, lvl);
        launch_resid_restrict(F->sweep_view(), view_of(c, lvl - 1), c->op, c->lambda, nullptr, 1, F->d_parent_local,
                              F->d_dix, c->stream, F->d_bnd, F->n_bnd, rhs_shifts(c, F));
      }
    } else {
      // (a stand-alone cycle's top level: res stays unstored, materialize_res)
      const bool pend = res_may_pend && res_pend_ok(c, F);
      Prof p(c, "resid_restrict", (double)F->n * F->nc * F->nc * F->nc, lvl);
      launch_resid_restrict(F->sweep_view(), view_of(c, lvl - 1), c->op, c->lambda, nullptr, 1, F->d_parent_local,
                            F->d_dix, c->stream, nullptr, 0, rhs_shifts(c, F), !pend);
      F->res_pend = pend;
      F->res_src = pend ? F->d_phi : nullptr;
    }
    restrict_remote(c, 1, lvl);
    restrict_remote(c, 4, lvl);
    // the fused step leaves the colour-1 halves of physical / refinement-
    // boundary ghosts as they were before the substep (k_smooth_resid); the
    // up-step's correction forms them again before anything reads them
    if (fused && (F->any_phys || F->any_rb)) F->phi_gc_ok = false;
  } else {
    residual_lvl(c, lvl, nullptr);
    restrict_lvl(c, 1, lvl);
    restrict_lvl(c, 4, lvl);
  }
  if (tail_crhs) return;
  Level* C = level_ptr(c, lvl - 1);
  // the fill of lvl-1 and its parents' coarse rhs in one pass when its faces
  // are same-GPU or physical (k_fill_crhs: a parent box reads its
  // neighbours' boundary cells itself instead of waiting for their pushes)
  if (C && C->n && !C->parents.empty() && !C->has_rb && !C->has_remote && !c->no_fill_tile && !c->no_fill_crhs &&
      (C->nc == 16 || C->nc == 8 || C->nc == 4)) {
    ready(c, lvl - 1, kWrite), wrote(c, lvl - 1, kGcAll);
    {
      Prof p(c, "fill_crhs", (double)C->n * C->nc * C->nc * C->nc, lvl - 1);
      launch_fill_crhs(C->sweep_view(), c->op, c->lambda, bc_for(c, lvl - 1, 1), C->d_parmask, c->stream);
    }
    finish_halo(c, C, 1);
    return;
  }
  fill_gc_lvl(c, lvl - 1, 1);
  if (C && !C->parents.empty()) {
    Prof p(c, "coarse_rhs", (double)C->parents.size() * C->nc * C->nc * C->nc, lvl - 1);
    if (!launch_coarse_rhs_tile(C->sweep_view(), c->op, c->lambda, C->d_parents, (int)C->parents.size(), c->stream))
      launch_coarse_rhs(C->view(), c->op, c->lambda, C->d_parents, (int)C->parents.size(), c->stream);
  }
}

// correct_children (m_multigrid.f90:387-402)
void correct_children(omg_ctx* c, int lvl) {
  Level* C = level_ptr(c, lvl);
  if (C && !C->parents.empty()) {
    Prof p(c, "sub_parents", (double)C->parents.size() * C->nc * C->nc * C->nc, lvl);
    launch_sub_parents(C->view(), C->d_parents, (int)C->parents.size(), c->stream);
  }
  prolong(c, lvl, 4, 1, 1);
}

// correct_children(lvl) + fill of lvl+1 + its first up-smoothing substep in
// one pass (k_prolong_smooth), when the level allows; returns whether it ran
// (the caller then starts smooth_boxes at substep 2).
static bool prolong_smooth(omg_ctx* c, int lvl) {
  Level* F = level_ptr(c, lvl + 1);
  Level* C = level_ptr(c, lvl);
  // refinement-boundary faces: their coarse boxes on this GPU (decided alike
  // on every rank: any_rbx), formed on the device (no host refinement_bnd
  // for phi), 16^3 / 8^3 boxes
  const bool rb_ok = F && !c->no_rb_fill_fuse && !F->any_rbx && (F->nc == 16 || F->nc == 8) &&
                     !(F->rbh.count(1) && F->rbh.at(1).n);
  if (c->no_fuse_up || !F || !C || !F->prolong_smooth_ok || c->smoother != OMG_SMOOTHER_GSRB ||
      (c->op != OP_LPL && c->op != OP_HELM) ||
      c->n_cycle_up < 1 || (F->has_rb && !rb_ok) || (F->has_remote && !F->n_int) || !tiled_nc(F->nc) ||
      !((size_t)F->n == 8 * C->parents.size() || C->nc * 2 == F->nc) ||
      (c->n_ranks > 1 && (F->prol.n_send || F->prol.n_recv)))
    return false;
  ready(c, lvl + 1, kPhi | kGhosts | kRhs | kWrite);
  const bool split = F->has_remote;
  {
    const int n = split ? F->n_int : F->n;
    Prof p(c, "prolong_smooth", (double)n * F->nc * F->nc * F->nc, lvl + 1);
    launch_prolong_smooth(C->view(), F->sweep_view(), c->op, c->lambda, F->d_parent_local, F->d_dix,
                          bc_for(c, lvl + 1, 1), C->nc * 2 == F->nc, split ? F->d_int : nullptr, n,
                          split ? F->d_push0 : nullptr, c->stream, F->has_rb, F->has_rb ? F->d_rbgv : nullptr);
    if (F->has_rb && F->d_rbgv) F->rbgv_ok = true;   // (its substep stored the coarse parts)
  }
  if (split) {
    // multi-GPU: boxes with a face on another GPU take the unfused pair,
    // correct + fill (their faces travel), then the colour-1 substep; their
    // same-GPU neighbours above pushed them the corrected colour 0 (push0)
    {
      Prof p(c, "prolong_fill", (double)F->n_bnd * F->nc * F->nc * F->nc, lvl + 1);
      launch_prolong_fill(C->view(), F->sweep_view(), 4, F->d_parent_local, F->d_dix, bc_for(c, lvl + 1, 1),
                          F->d_sendbuf, true, !c->no_skip1, c->stream, F->d_bnd, F->n_bnd, false,
                          F->h_rb.empty() ? nullptr : F->d_rb);
    }
    finish_halo(c, F, 1);
    {
      // (the boundary boxes' refinement-boundary coarse parts are stored here,
      // the interior boxes' by k_prolong_smooth: the level's whole buffer is
      // current after this)
      Prof p(c, "smoother_gsrb", 0.5 * F->n_bnd * F->nc * F->nc * F->nc, lvl + 1);
      launch_gs_substep(F->view(), c->op, c->lambda, 1, 1 << 1, view_of(c, lvl), F->d_rb, F->has_rb,
                        bc_for(c, lvl + 1, 1), F->d_sendbuf, nullptr, c->stream, F->d_bnd, F->n_bnd,
                        F->has_rb ? F->d_rbgv : nullptr, F->has_rb && F->d_rbgv ? 1 : 0);
    }
    finish_halo(c, F, 1);
  }
  // colour-0 ghost halves hold pre-correction values, but the next substep
  // reads only colour 1 and pushes colour 0 itself
  wrote(c, lvl + 1, kGcAll);
  return true;
}

// correct_children(l-1) + fill of l + up-smoothing substeps 1-3 of l in one
// k_gsrb3 pass (its correct_children form); returns whether it ran (the caller
// then starts smooth_boxes at substep 4).  Levels with k_gsrb3's coarse
// records (build_coarse_columns, omg_columns.cpp), whose coarse level has consistent ghosts (the
// reference's correction reads the parents' ghost cells; the pass reads the
// neighbour parents' cells).
static bool block3c_ok(omg_ctx* c, const Level* F) {
  return F && F->d_b3c && !c->no_block3 && !c->no_block3p && c->smoother == OMG_SMOOTHER_GSRB &&
         gsrb3_op_ok(c->op) && c->n_cycle_up * c->n_substeps >= 3;
}
// res_ready: the coarse level's last up pass stored its res = phi - old
// (smooth_boxes' want_res), which the pass then reads instead of phi and old;
// then, where the up-smoothing has four substeps or more, the pass is
// k_gsrb4's correction form, substeps 1-4 (round 6: level 1 of C3 815 + 308
// us for k_gsrb3's form + the one-substep launch before; OMG_NO_BLOCK4P: those)
// Returns the substeps run (0: none, the caller corrects otherwise).
static int correct_block3(omg_ctx* c, int l, bool res_ready, bool defer_gc = false) {
  Level* F = level_ptr(c, l);
  Level* C = level_ptr(c, l - 1);
  if (!block3c_ok(c, F) || !C || !C->phi_gc_ok || C->shift_pending) return 0;
  // (a split level: only from the coarse res, whose proxies deep_res filled)
  if (F->deep && !res_ready) return 0;
  const bool four = res_ready && c->block4 && !c->no_block4p && c->n_cycle_up * c->n_substeps >= 4;
  ready(c, l, kPhi | (four ? 0 : kRhs) | kWriteOther);   // (k_gsrb4 takes the rhs shifts)
  double* other = other_phi(F);
  const LevelView cv = C->view();
  int done = 3;
  deep_before(c, F, 0);   // (the pass reads colour 0, before the correction)
  // defer_gc: nothing reads the level's ghosts before its next pass, which
  // reads none (the stand-alone V-cycle's last pass on its top level, see
  // fas_vcycle): the pass writes the interior only (12 of the 44 KB it
  // writes per box are ghost faces), and the ghosts are filled if anything
  // else comes first (Level::gc_deferred)
  bool deferred = false;
  if (four) {
    // (one rank: every rank decides its fills alike, see fas_vcycle)
    deferred = defer_gc && c->n_ranks == 1 && c->n_cycle_up * c->n_substeps == 4 && !F->deep && !F->b3_phys &&
               !c->no_defer_gc;
    Prof p(c, "smoother_gsrb4p", 2.0 * F->n * F->nc * F->nc * F->nc, l);
    launch_gsrb4(F->view(), other, F->d_b3, F->n_b3, c->op, c->lambda, 1, nullptr, c->stream, &cv, F->d_b3c,
                 nullptr, !deferred, rhs_shifts(c, F));
    done = 4;
  } else {
    Prof p(c, "smoother_gsrb3p", 1.5 * F->n * F->nc * F->nc * F->nc, l);
    launch_gsrb3(F->view(), other, F->d_b3, F->n_b3, c->op, c->lambda, 1, nullptr, c->stream, true, &cv, F->d_b3c,
                 res_ready ? 2 : 1);
  }
  wrote(c, l, kWriteOther | (deferred ? kGcNone : kGcAll));
  deep_after(c, F);
  return done;
}

// correct_children(lvl) followed by mg_fill_ghost_cells_lvl(lvl+1, phi), as the
// V-cycle and FMG run them (m_multigrid.f90:127-136, 216-219); fused when every
// box of lvl+1 has its parent on this GPU (refinement-boundary ghosts are
// interpolated in the same kernel from lvl, which is final by then).
// then_gsrb: the caller smooths lvl+1 with red-black substeps right after
// (colour 1 first), so colour 1's correction is dead where no face needs it.
// save_old (FMG, fused path only, see correct_fill_fused): old = phi of lvl+1
// before the correction, the interior written by the fused kernel.
static bool correct_fill_fused(omg_ctx* c, int lvl) {
  Level* F = level_ptr(c, lvl + 1);
  Level* C = level_ptr(c, lvl);
  return F && C && F->n && F->n_pairs == F->n && tiled_nc(F->nc) && !(F->has_rb && c->no_rb_fill_fuse) &&
         !(c->n_ranks > 1 && (F->prol.n_send || F->prol.n_recv));
}

static void correct_and_fill(omg_ctx* c, int lvl, bool then_gsrb = false, bool save_old = false) {
  Level* F = level_ptr(c, lvl + 1);
  Level* C = level_ptr(c, lvl);
  if (save_old && (then_gsrb || !correct_fill_fused(c, lvl)))
    throw OmgError("internal: old = phi fused into an unfused correction");
  ready(c, lvl + 1, kPhi | kGhosts | kWrite);
  if (correct_fill_fused(c, lvl)) {
    // every parent here has all its children on this GPU (no prolongation
    // traffic, every fine box has a local parent): the children form res
    const bool sub = (size_t)F->n == 8 * C->parents.size() || C->nc * 2 == F->nc;
    if (!sub && !C->parents.empty()) {
      Prof p(c, "sub_parents", (double)C->parents.size() * C->nc * C->nc * C->nc, lvl);
      launch_sub_parents(C->view(), C->d_parents, (int)C->parents.size(), c->stream);
    }
    {
      Prof p(c, "prolong_fill", (double)F->n * F->nc * F->nc * F->nc, lvl + 1);
      launch_prolong_fill(C->view(), F->sweep_view(), 4, F->d_parent_local, F->d_dix, bc_for(c, lvl + 1, 1),
                          F->d_sendbuf, sub, then_gsrb && !c->no_skip1, c->stream, nullptr, 0, save_old,
                          F->h_rb.empty() ? nullptr : F->d_rb);
    }
    finish_halo(c, F, 1);
    wrote(c, lvl + 1, kGcAll);
    return;
  }
  correct_children(c, lvl);
  fill_gc_lvl(c, lvl + 1, 1);
}

// The highest level `top` such that every level lowest..top can run inside
// the single-workgroup coarse program (launch_coarse_tail): a few boxes, all
// on this GPU, LDS-tiled box size, no refinement boundary, and every parent
// with all its children here.  INT_MIN when not even the lowest level can.
static int tail_top(omg_ctx* c, int max_lvl) {
  // (the variable-coefficient operators measured faster level by level:
  // their single-workgroup program spills heavily)
  if (c->op != OP_LPL && c->op != OP_HELM) return INT_MIN;
  if (max_lvl - c->lowest + 1 > kTailMaxLevels) max_lvl = c->lowest + kTailMaxLevels - 1;
  int top = INT_MIN;
  for (int l = c->lowest; l <= max_lvl; l++) {
    Level* L = level_ptr(c, l);
    if (!L || L->n < 1 || L->n > kTailMaxBoxes || L->n != (int)c->ids[l].size() || L->has_rb ||
        !tiled_nc(L->nc))
      break;
    if (l > c->lowest) {
      Level* C = level_ptr(c, l - 1);
      if (L->n_pairs != L->n || !((size_t)L->n == 8 * C->parents.size() || C->nc * 2 == L->nc)) break;
    }
    top = l;
  }
  return top;
}

// Levels lowest..top of the V-cycle (down-smoothing of top .. up-smoothing of
// top) in one launch, bit-identical to the level-by-level path.
// the LDS-resident part of the tail (omg_tiles.hip): one box per level whose
// faces are physical or the box itself, the lowest levels up to 8^3 cells
// (at most three: 2^3, 4^3, 8^3, 5,120 doubles for their four variables),
// and a 16^3 top level right above them
static void tail_lds_plan(omg_ctx* c, int top, int* lds_levels, int* lds_top) {
  const int n_lvls = top - c->lowest + 1;
  auto lds_box_ok = [&](int l, int max_nc) {
    Level* L = level_ptr(c, l);
    if (!L || L->n != 1 || L->nc > max_nc) return false;
    for (int nb = 0; nb < 6; nb++) {
      const int k = L->h_nbk[nb];
      if (!(k == NB_PHYS || (k == NB_LOCAL && L->h_nba[nb] == 0))) return false;
    }
    return true;
  };
  int n = 0;
  while (n < std::min(n_lvls, kTailLdsMaxLevels) && lds_box_ok(c->lowest + n, 8)) n++;
  *lds_levels = n;
  *lds_top = n > 0 && n == n_lvls - 1 && level_ptr(c, top)->nc == 16 && lds_box_ok(top, 16);
}

// whether the tail can take over update_coarse's fill and coarse rhs of its
// top level: a single parent box on this GPU whose faces are physical or same-
// GPU (kTailMaxBoxes), after a level-by-level down-step of top+1
static bool tail_crhs_ok(omg_ctx* c, int top) {
  const Level* T = level_ptr(c, top);
  return !c->no_tail_crhs && T && T->n == 1 && !T->parents.empty() && !T->has_rb && !T->has_remote &&
         level_ptr(c, top + 1) != nullptr;
}

static void run_tail(omg_ctx* c, int top, bool top_crhs) {
  TailArgs A;
  std::memset(&A, 0, sizeof(A));   // padding too: compared bytewise below
  A.n_lvls = top - c->lowest + 1;
  for (int l = c->lowest; l <= top; l++) {
    Level* L = level_ptr(c, l);
    // (phi of an all-parents level below the top is overwritten by the
    // restriction; the tail reads rhs as stored and writes that of the levels
    // below its top)
    ready(c, l, (L->all_parents && l < top ? kPhiDead : kPhi) | kRhs | kWrite);
    wrote(c, l, kRhsWrite);
    TailLevel& T = A.lv[l - c->lowest];
    T.L = L->view();
    T.bc = bc_for(c, l, 1);
    T.parents = L->d_parents;
    T.n_par = (int)L->parents.size();
    T.parent_local = L->d_parent_local;
    T.dixp = L->d_dix;
    // the first box's bc table entries inline (the LDS setup reads them
    // without a dependent load)
    auto fo = c->h_face_off_lvl[0].find(l);
    auto ft = c->h_face_type_lvl[0].find(l);
    for (int nb = 0; nb < 6; nb++) {
      const bool tab = fo != c->h_face_off_lvl[0].end() && fo->second.size() >= 6;
      const long long o = tab ? fo->second[nb] : -1;
      T.foff[nb] = o > INT_MAX ? -2 : (int)o;
      T.ftype[nb] = (signed char)(tab && ft != c->h_face_type_lvl[0].end() && ft->second.size() >= 6 ? ft->second[nb] : 0);
    }
  }
  A.lambda = c->lambda;
  A.n_down = c->n_cycle_down;
  A.n_up = c->n_cycle_up;
  A.max_coarse = c->max_coarse_cycles;
  A.res_abs = c->res_abs;
  A.res_rel = c->res_rel;
  A.maxbits = (unsigned long long*)c->d_scalar;
  A.coarse_its = (int*)(c->d_scalar + 1);
  A.gs_lex = c->smoother != OMG_SMOOTHER_GSRB;
  A.top_crhs = top_crhs;
  tail_lds_plan(c, top, &A.lds_levels, &A.lds_top);
  const bool tail_timing = c->tail_timing;
  if (tail_timing) {
    if (!c->d_tail_stamps) HIPCHK(hipMalloc(&c->d_tail_stamps, 8 * 64));   // (never captured: graph_ok)
    A.stamps = c->d_tail_stamps;
    HIPCHK(hipMemsetAsync(c->d_tail_stamps, 0, 8 * 64, c->stream));   // (unwritten stamps stay 0)
  }
  if (std::memcmp(&A, c->h_tail, sizeof(TailArgs)) != 0) {
    *c->h_tail = A;   // what d_tail holds once the stream gets here
    launch_store_tail(A, c->d_tail, c->stream);
  }
  {
    Prof p(c, "coarse_tail", 0.0, top);
    launch_coarse_tail(c->d_tail, A.gs_lex, c->op, c->stream);
  }
  if (tail_timing) {   // diagnostics: phase times of the tail (100 MHz wall clock)
    long long h[64];
    HIPCHK(hipMemcpyAsync(h, c->d_tail_stamps, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    host_sync(c, c->stream);
    std::fprintf(stderr, "tail us:");
    for (int i = 1; i < 64 && h[i]; i++) std::fprintf(stderr, " %.1f", (h[i] - h[i - 1]) * 0.01);
    std::fprintf(stderr, "\n");
  }
  for (int l = c->lowest; l <= top; l++) wrote(c, l, kGcAll);
}

// Failure detection: the device max residual is an exact max of
// |res| over IEEE bits, so one NaN or Inf cell makes it non-finite.  The
// reference's Fortran max() drops NaN operands (m_multigrid.f90:226-234,
// 296-311) and reports a finite or zero residual for a diverged field; here
// it is an error instead, the caller's output argument holding the bits.
void check_finite_res(double r, const char* where) {
  if (!std::isfinite(r))
    throw OmgError(std::string(where) + ": non-finite residual (" + (std::isnan(r) ? "NaN" : "Inf") +
                   "): phi or rhs holds NaN/Inf");
}

// mg_fas_vcycle (m_multigrid.f90:150-243)
double fas_vcycle(omg_ctx* c, int highest_lvl, bool want_max_res, bool standalone) {
  const bool has_highest = highest_lvl >= c->lowest;
  const int min_lvl = c->lowest, max_lvl = has_highest ? highest_lvl : c->highest;
  const bool full = standalone && !has_highest;   // a stand-alone cycle over the whole tree
  // (nothing below changes which levels the coarse tail can hold)
  const int top = tail_top(c, max_lvl);
  const bool tail = top >= min_lvl && !c->no_tail;
  const bool tail_crhs = tail && max_lvl > top && tail_crhs_ok(c, top);
  // A res left pending by the previous stand-alone cycle (Level::res_pend) is
  // dead when this cycle's update_coarse runs on that level, which writes
  // every box of it (or leaves it pending anew); decided here, before this
  // cycle's rhs mean joins the list and its first pass writes the buffer.
  // Any other cycle (partial, inside FMG, or one whose coarse tail holds the
  // level) leaves that res as the reference does: it is stored first.
  const bool top_updates = full && max_lvl > min_lvl && !(tail && max_lvl <= top);
  materialize_res_all(c, top_updates ? max_lvl : INT_MIN);
  // a pending phi shift (previous stand-alone cycle) is absorbed by the first
  // substep on max_lvl or dropped where restriction overwrites a level
  if (c->phi_shift_pending) {
    if (!full) {
      materialize_phi(c);
    } else {
      for (auto& kv : c->levels)
        if (kv.first != max_lvl && !kv.second.all_parents) ready(c, kv.first, kPhi);
    }
  }
  // rhs shifts a stand-alone cycle left pending stay so through the next one
  // (subtract_mean adds this cycle's); any other cycle writes them out first
  if (!full) materialize_rhs_all(c);
  struct FullCycle {   // materialize_rhs notes the readers that ran without the list
    omg_ctx* c;
    ~FullCycle() { c->in_full_cycle = false; }
  } full_cycle{c};
  c->in_full_cycle = full;
  if (c->subtract_mean && !has_highest) subtract_mean(c, 2, 0, full ? kInCycle : kPlain);
  if (standalone) {
    // the fill is idempotent: skip it when the ghosts already equal its result.
    // Fills exchange halos, so every rank must decide alike; the decision is
    // rank-invariant without communication: phi_gc_ok changes only in calls
    // every rank makes (fills, cycles, restriction / prolongation, collective
    // uploads of phi, see omg.h), and any_rb is a property of the global
    // tree.  (Agreeing over the transport instead, as round 3 did, cost a
    // host synchronisation per cycle.)  OMG_CHECK_COLLECTIVE checks it.
    // A level with refinement boundaries is consistent as long as the level
    // below was not written since its last fill (rb_stale_above).  With a
    // subtracted mean those writes depend on per-rank state (pending mean
    // shifts, materialised where a rank has boxes), so with more than one
    // rank such a level is then always refilled.
    Level* L = level_ptr(c, max_lvl);
    bool need = !(L && L->phi_gc_ok && (!L->any_rb || c->n_ranks == 1 || !c->subtract_mean));
    // (ghosts deferred by the last cycle: its first pass reads none, k_gsrb4 /
    // k_gsrb3, and writes them all; smooth_boxes fills first otherwise).
    // Only when this cycle smooths on the way down: the counts may have
    // changed since the deferral was made, and with n_cycle_down = 0 (a
    // zero-trip loop in the reference, m_multigrid.f90:407) smooth_boxes
    // launches nothing and update_coarse's residual reads the ghosts next
    if (L && L->gc_deferred && c->smoother == OMG_SMOOTHER_GSRB && top < max_lvl &&
        c->n_cycle_down * c->n_substeps >= 1)
      need = false;
    if (c->n_ranks > 1 && c->check_collective && (allreduce(c, need ? 1.0 : 0.0, true) > 0.5) != need)
      throw OmgError("mg_fas_vcycle: the stand-alone fill decision differs across ranks "
                     "(an upload of phi was not made on every rank)");
    if (need) {
      ready(c, max_lvl, kPhi);
      fill_gc_lvl(c, max_lvl, 1);
    }
  }
  for (int l = max_lvl; l >= min_lvl + 1; l--) {
    if (tail && l <= top) break;
    // four substeps per pass, then the unfused residual (k_resid_restrict):
    // C3 4.06 -> 3.97 ms against k_gsrb3 + k_smooth_resid (level 1 775 + 592
    // us; level 0 even, profiles/r05/s50_block4_ab.txt); OMG_NO_BLOCK4: the latter
    // (a level with physical faces: k_gsrb3 + k_smooth_resid, whose k_gsrb4
    // takes a workgroup per CU, 114 VGPRs; OMG_BLOCK4_PHYS: k_gsrb4 there too)
    B3Phys P3;
    const B3Phys* ph = nullptr;
    const bool four = c->block4 && c->smoother == OMG_SMOOTHER_GSRB && b3_usable(c, l, P3, ph) &&
                      (!ph || c->block4_phys) && (c->n_cycle_down * c->n_substeps) % 4 == 0;
    const bool fused = !four && smooth_resid_ok(c, l);
    // (the down pass writes its ghosts, which the residual reads: leaving them
    // to a residual that gathers the neighbours' boundary cells instead took
    // C3's down pass 837 -> 713 us and the residual 590 -> 750 us, the x faces'
    // cells 64 B apart in the neighbours' boxes; profiles/r06/s19_defer_down_ab.txt)
    smooth_boxes(c, l, c->n_cycle_down, 1, fused ? 1 : 0, false, four);
    update_coarse(c, l, fused, tail_crhs && l == top + 1, full && l == max_lvl);
    faces_join(c, level_ptr(c, l));   // (update_coarse joined them; defensive)
  }
  if (tail) {
    run_tail(c, top, tail_crhs);
  } else {
    // coarse grid: all its boxes live on one rank (error stop otherwise, :197-200)
    const auto& ids = c->ids[min_lvl];
    for (int id : ids)
      if (min_lvl > c->rep_lvl && c->rank_of[id - 1] != c->rank_of[ids[0] - 1])
        throw OmgError("Multiple CPUs for coarse grid (not implemented yet)");
    // a rank without the coarse boxes has nothing to do here: they all live on
    // one rank, so their smoothing exchanges nothing (the reference's other
    // ranks run empty loops until the owner's residual test, which they never
    // see either, m_multigrid.f90:202-208); skipping it saves them a host wait
    // per coarse sweep
    const Level* Lmin = level_ptr(c, min_lvl);
    const bool own_coarse = Lmin && Lmin->n > 0;
    double init_res = own_coarse ? max_residual_lvl(c, min_lvl) : 0.0;
    for (int i = 1; own_coarse && i <= c->max_coarse_cycles; i++) {
      smooth_boxes(c, min_lvl, c->n_cycle_up + c->n_cycle_down);
      double res = max_residual_lvl(c, min_lvl);
      if (res < c->res_rel * init_res || res < c->res_abs) break;
    }
  }
  // res_ready: level l-1's last up pass stored its res (correct_children's
  // phi - old) for level l's correct_children form.  A level whose level
  // above takes that form (want_res) ends its up-smoothing with that pass, so
  // it starts with k_prolong_smooth rather than the form itself (which leaves
  // a plain last substep).
  bool res_ready = false;
  for (int l = (tail ? top : min_lvl) + 1; l <= max_lvl; l++) {
    const bool want_res = l < max_lvl && block3c_ok(c, level_ptr(c, l + 1)) && !c->no_block3r;
    bool done = false;
    int pro = 0;
    if (!want_res && (pro = correct_block3(c, l, res_ready, full && l == max_lvl && !want_max_res)) > 0) {
      done = smooth_boxes(c, l, c->n_cycle_up, pro + 1);
    } else if (prolong_smooth(c, l - 1)) {
      done = smooth_boxes(c, l, c->n_cycle_up, 2, 0, want_res);
    } else {
      correct_and_fill(c, l - 1, c->smoother == OMG_SMOOTHER_GSRB && c->n_cycle_up >= 1);
      done = smooth_boxes(c, l, c->n_cycle_up, 1, 0, want_res);
    }
    res_ready = done;
  }
  double max_res = 0.0;
  if (want_max_res) {
    double m = 0.0;
    if (min_lvl <= max_lvl) m = max_residual_levels(c, min_lvl, max_lvl);
    max_res = allreduce(c, m, true);
  }
  materialize_phi(c);   // nothing left pending after a cycle (defensive: all consumed)
  if (c->subtract_mean) subtract_mean(c, 1, 1, full ? kInCycle : kPlain);
  return max_res;
}

// mg_fas_fmg (m_multigrid.f90:84-147)
double fas_fmg(omg_ctx* c, bool have_guess, bool want_max_res) {
  materialize_res_all(c);   // (FMG's own update_coarse loop stores; a pending res is written out as it stands)
  materialize_rhs_all(c);
  if (have_guess) {
    materialize_phi(c);
  } else {
    for (auto& kv : c->levels) kv.second.shift_pending = false;   // phi = 0 below
    c->phi_shift_pending = false;
  }
  if (!have_guess) phi_dirty_all(c);
  if (!have_guess)
    for (int l = c->highest; l >= c->lowest; l--) {
      Level* L = level_ptr(c, l);
      if (L && L->n) launch_copy_var(L->view(), 0, 1, c->stream);
    }
  fill_gc_lvl(c, c->highest, 1);
  for (int l = c->highest; l >= c->lowest + 1; l--) update_coarse(c, l);
  if (c->subtract_mean) subtract_mean(c, 2, 0);
  double max_res = 0.0;
  for (int l = c->lowest; l <= c->highest; l++) {
    Level* L = level_ptr(c, l);
    // old = phi (:127-129).  Below the highest level, where every box is a
    // parent, update_coarse's parent loop above left old equal to phi, ghost
    // faces included, and nothing has written that level since (unless the
    // cycles below subtract phi's mean, which covers every level)
    // Elsewhere the copy's interior half rides on the fused correction, which
    // loads the pre-correction interior anyway: only the ghost faces are copied
    const bool old_is_phi = l < c->highest && L && L->all_parents && !c->subtract_mean;
    const bool save_old = L && L->n && !old_is_phi && l > c->lowest && correct_fill_fused(c, l - 1);
    if (save_old) {
      launch_copy_ghosts(L->view(), c->stream);
    } else if (L && L->n && !old_is_phi) {
      launch_copy_var(L->view(), 1, 3, c->stream);
    }
    if (l > c->lowest) correct_and_fill(c, l - 1, false, save_old);
    if (l == c->highest)
      max_res = fas_vcycle(c, l, want_max_res, false);
    else
      fas_vcycle(c, l, false, false);
  }
  return max_res;
}

// A whole cycle (V-cycle or FMG) as one HIP graph: the host logic runs as
// usual while the stream is captured, so every kernel argument and every
// host-side state change is exactly that of the direct launches; the graph of
// the previous call with the same key is updated in place (same topology) or
// re-instantiated, then launched.  A graph issues a dependent kernel in ~1.8
// us of host time against ~3.2 us direct (tools/graph_probe.hip), but the
// cycles measured no faster (C1 0.252 -> 0.260 ms, C4 0.553 -> 0.568, 512^3
// FMG 11.65 -> 11.49): their small-level kernels are bound by their own
// 3-5 us on the GPU, not by the host, and capturing costs what it saves.
// Opt-in (OMG_GRAPH=1).  Only where the cycle never waits for the host:
// one GPU, no subtract_mean (its side-stream chain spans calls), every
// V-cycle ends in the coarse tail (the level-by-level coarse solve reads its
// residual back per sweep), no profiling.
static bool graph_ok(omg_ctx* c) {
  return !c->no_graph && !c->capturing && c->n_ranks == 1 && !c->subtract_mean && !c->profiling && !c->rbh_any &&
         !c->tail_timing && !c->no_tail && c->n_boxes > 0 && tail_top(c, c->highest) >= c->lowest;
}

// The host state the captured body changed assumes the graph ran.  When the
// capture, instantiation or launch fails, that is rolled back to "unknown":
// the tail arguments are re-uploaded by the next call (h_tail no longer
// matches anything), the graph of this key is dropped, and every level's phi
// ghost faces count as stale (the next cycle fills them).  (The graph path
// runs without subtract_mean, so no mean / shift state is involved.)
static void graph_rollback(omg_ctx* c, int key, const std::map<int, double*>& phi_at_start) {
  c->capturing = false;
  // the multi-substep passes swap a level's phi buffer on the host as they are
  // recorded: a graph that never ran leaves phi where it was
  for (auto& kv : phi_at_start) c->levels[kv.first].d_phi = kv.second;
  c->max_deferred = false;
  std::memset(c->h_tail, 0xff, sizeof(TailArgs));
  auto it = c->graphs.find(key);
  if (it != c->graphs.end()) {
    if (it->second) (void)hipGraphExecDestroy(it->second);
    c->graphs.erase(it);
  }
  phi_dirty_all(c);
  // the captured body may have recorded the ring-order rhs copy (and marked
  // it built) without the graph ever running
  drop_rhs_lex(c);
  (void)hipGetLastError();
}

double run_cycle(omg_ctx* c, int key, const std::function<double()>& body) {
  if (!graph_ok(c)) return body();
  // a captured cycle leaves no res pending (res_pend_ok) and finds none: what
  // a direct cycle left is stored before the capture begins, so a rollback
  // has no such state to restore
  materialize_res_all(c);
  std::map<int, double*> phi_at_start;
  for (auto& kv : c->levels) phi_at_start[kv.first] = kv.second.d_phi;
  c->capturing = true;
  c->max_deferred = false;
  HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  hipGraph_t g = nullptr;
  try {
    if (c->graph_fail_at == 1) {   // one-shot test injection
      c->graph_fail_at = 0;
      throw OmgError("injected failure during capture (OMG_GRAPH_FAIL=1)");
    }
    body();
  } catch (...) {
    (void)hipStreamEndCapture(c->stream, &g);
    if (g) (void)hipGraphDestroy(g);
    graph_rollback(c, key, phi_at_start);
    throw;
  }
  c->capturing = false;
  try {
    HIPCHK(hipStreamEndCapture(c->stream, &g));
    size_t n_nodes = 0;
    HIPCHK(hipGraphGetNodes(g, nullptr, &n_nodes));
    if (c->graph_fail_at == 2) {   // one-shot: the body ran (host state changed), the graph does not
      c->graph_fail_at = 0;
      throw OmgError("injected failure before the launch (OMG_GRAPH_FAIL=2)");
    }
    if (n_nodes) {
      hipGraphExec_t& ex = c->graphs[key];
      if (ex) {
        hipGraphNode_t err_node = nullptr;
        hipGraphExecUpdateResult res;
        if (hipGraphExecUpdate(ex, g, &err_node, &res) != hipSuccess || res != hipGraphExecUpdateSuccess) {
          (void)hipGetLastError();
          HIPCHK(hipGraphExecDestroy(ex));
          ex = nullptr;
        }
      }
      if (!ex) HIPCHK(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
      HIPCHK(hipGraphLaunch(ex, c->stream));
    }
  } catch (...) {
    if (g) (void)hipGraphDestroy(g);
    graph_rollback(c, key, phi_at_start);
    throw;
  }
  HIPCHK(hipGraphDestroy(g));
  if (!c->max_deferred) return 0.0;
  c->max_deferred = false;
  host_sync(c, c->stream);
  return c->h_scalar[0];
}

// mg_set_methods' operator part + *_set_lambda (m_multigrid.f90:27-60,
// m_helmholtz.f90:39-46, m_vhelmholtz.f90:51-58, m_ahelmholtz.f90:59-66)
void set_operator(omg_ctx* c, int op, double lambda) {
  if (op < OMG_LAPLACIAN || op > OMG_AHELMHOLTZ) throw OmgError("mg_set_methods: unknown operator");
  if (lambda < 0) throw OmgError("helmholtz_set_lambda: lambda < 0 not allowed");
  if (op == OMG_AHELMHOLTZ && c->n_vars < 7 && c->n_boxes > 0)
    throw OmgError("ahelmholtz_set_methods: needs 3 extra variables");
  if ((op == OMG_VLAPLACIAN || op == OMG_VHELMHOLTZ) && c->n_vars < 5 && c->n_boxes > 0)
    throw OmgError("vlaplacian/vhelmholtz_set_methods: mg%n_extra_vars == 0");
  if (op == OMG_VLAPLACIAN) lambda = 0.0;
  const bool changed = c->op != op;
  // (a pending res is that of the operator and lambda it was skipped under)
  if ((changed || lambda != c->lambda) && !c->host_only) materialize_res_all(c);
  if (changed) rhs_pend_retry(c);
  c->op = op;
  c->lambda = lambda;
  if (changed && !c->capturing) ensure_rhs_lex(c);
}

// mg_apply_op (m_multigrid.f90:439-456): box_op on every box of every level
void apply_op(omg_ctx* c, int i_out) {
  enter(c);
  if (i_out == 1) phi_dirty_all(c);
  for (int l = c->lowest; l <= c->highest; l++) {
    Level* L = level_ptr(c, l);
    if (L && L->n) launch_box_op(L->view(), c->op, c->lambda, i_out, c->stream);
  }
}

// m_diffusion's set_rhs (m_diffusion.f90:144-159): rhs = f1*phi + f2*rhs on
// the interior of this rank's leaves of levels 1..highest
void set_rhs(omg_ctx* c, double f1, double f2) {
  enter(c);
  for (int l = 1; l <= c->highest; l++) {
    Level* L = level_ptr(c, l);
    if (!L || L->leaves.empty()) continue;
    launch_set_rhs(L->view(), L->d_leaves, (int)L->leaves.size(), f1, f2, c->stream);
  }
}

// diffusion_solve / diffusion_solve_vcoeff / diffusion_solve_acoeff
// (m_diffusion.f90:19-57, :63-101, :108-142): one implicit time step of
// order 1 (backward Euler) or 2 (Crank-Nicolson) as a Helmholtz problem,
// FMG first, then up to 10 V-cycles until max_res.  The three differ only in
// the operator and in lambda = 1/(dt*D) vs 1/dt (D = 1 for the v/a forms).
constexpr int kDiffusionMaxIts = 10;   // m_diffusion.f90:25
void diffusion_solve(omg_ctx* c, int op, double dt, double coeff, int order, double max_res, int* n_vcycles,
                     double* res_out) {
  if (op != OMG_HELMHOLTZ && op != OMG_VHELMHOLTZ && op != OMG_AHELMHOLTZ)
    throw OmgError("diffusion_solve: operator must be helmholtz, vhelmholtz or ahelmholtz");
  if (order != 1 && order != 2) throw OmgError("diffusion_solve: order should be 1 or 2");
  const double dtc = op == OMG_HELMHOLTZ ? dt * coeff : dt;
  // helmholtz_set_methods / vhelmholtz_set_methods clear subtract_mean;
  // ahelmholtz_set_methods leaves it as it was
  set_operator(c, op, 0.0);
  if (op != OMG_AHELMHOLTZ) c->subtract_mean = 0;
  if (order == 1) {
    set_operator(c, op, 1 / dtc);
    set_rhs(c, -1 / dtc, 0.0);
  } else {
    apply_op(c, 2);   // lambda = 0: rhs = L(phi) on every level
    set_operator(c, op, 2 / dtc);
    set_rhs(c, -2 / dtc, -1.0);
  }
  double res = run_cycle(c, 2 + 2 + 4, [&] { return fas_fmg(c, true, true); });
  int n = 1;
  for (; n <= kDiffusionMaxIts; n++) {
    if (!std::isfinite(res)) {   // the outputs hold the state at the error (omg.h)
      if (n_vcycles) *n_vcycles = n - 1;
      if (res_out) *res_out = res;
      check_finite_res(res, "diffusion_solve");
    }
    if (res <= max_res) break;
    res = run_cycle(c, 1 + 2 + 4 + 8 * (c->lowest - 1 + 64),
                    [&] { return fas_vcycle(c, c->lowest - 1, true, true); });
  }
  if (n_vcycles) *n_vcycles = n - 1;
  if (res_out) *res_out = res;
  if (n == kDiffusionMaxIts + 1) throw OmgError("diffusion_solve: no convergence");
}

// ---------------------------------------------------------------------------
// mg_phi_bc_store (m_ghost_cells.f90:66-117): the bc values of phi go into
// the rhs ghost cells and the bc type into the neighbour slot.
void phi_bc_store(omg_ctx* c) {
  phi_dirty_all(c);
  for (auto& kv : c->levels) {
    Level& L = kv.second;
    if (!L.n) continue;
    GcBC g = bc_for(c, kv.first, 1);
    g.phi_stored = 0;
    launch_phi_bc_store(L.view(), g, L.d_nba, c->stream);
    HIPCHK(hipMemcpyAsync(L.h_nba.data(), L.d_nba, sizeof(int) * L.h_nba.size(), hipMemcpyDeviceToHost,
                          c->stream));
    host_sync(c, c->stream);
    for (int b = 0; b < L.n; b++)
      for (int nb = 1; nb <= 6; nb++)
        if (L.h_nbk[(size_t)b * 6 + nb - 1] == NB_PHYS)
          c->neighbors[(size_t)(L.ids[b] - 1) * 6 + nb - 1] = L.h_nba[(size_t)b * 6 + nb - 1];
    pack_topo(L);
  }
  c->phi_bc_data_stored = 1;
}

}  // namespace host
}  // namespace omg
