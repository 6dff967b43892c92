// omg_lazy.cpp — the per-level state that is left unwritten until somebody
// needs it (the five mechanisms described above Level's lazy fields in
// omg_internal.h), and the one place that decides what "needs it" means:
// ready() before a pass, from what the pass reads and writes (Pass flags,
// omg_host.h), wrote() after it; enter() and the whole-context forms for the
// entry points and the cycle starts.
#include "omg_host.h"

namespace omg {
namespace host {

// The refinement-boundary ghosts of level lvl+1 are interpolated from level
// lvl (its interior and tangential ghosts, box_gc_for_fine_neighbor,
// m_ghost_cells.f90:500-577): every write of phi on lvl makes them stale.
void rb_stale_above(omg_ctx* c, int lvl) {
  if (Level* U = level_ptr(c, lvl + 1)) {
    if (U->any_rb) U->phi_gc_ok = false;
    U->rbgv_ok = false;   // (its refinement-boundary coarse parts read lvl)
  }
}
// phi was written on a level: its ghost faces may no longer match a fill
void phi_dirty(omg_ctx* c, int lvl) {
  if (Level* L = level_ptr(c, lvl)) L->phi_gc_ok = L->gc_deferred = false;
  rb_stale_above(c, lvl);
}
void phi_dirty_all(omg_ctx* c) {
  for (auto& kv : c->levels) kv.second.phi_gc_ok = kv.second.rbgv_ok = kv.second.gc_deferred = false;
}
// After mg_phi_bc_store phi's boundary values live in rhs's ghost slots, and
// phi's ghosts across physical faces are formed from them (GcBC::phi_stored):
// a write of those slots (an upload or a put of rhs with its ghosts, a fill of
// rhs, subtract_mean with the ghosts) makes phi's ghosts stale, as a fill
// after it would change them.
void rhs_ghosts_written(omg_ctx* c, int lvl) {
  if (c->phi_bc_data_stored) phi_dirty(c, lvl);
}
void rhs_ghosts_written_all(omg_ctx* c) {
  if (c->phi_bc_data_stored) phi_dirty_all(c);
}

// --- the unstored res (Level::res_pend)
static void materialize_res(omg_ctx* c, Level* L) {
  if (!L->res_pend) return;
  L->res_pend = false;
  if (!L->n) return;
  LevelView V = L->sweep_view();
  V.phi = L->res_src;
  Prof p(c, "residual", (double)L->n * L->nc * L->nc * L->nc, L->lvl);
  launch_resid_restrict(V, empty_view(), c->op, c->lambda, nullptr, 0, nullptr, nullptr, c->stream, nullptr, 0,
                        rhs_shifts(c, L));
}
void materialize_res_all(omg_ctx* c, int dead_lvl) {
  for (auto& kv : c->levels) {
    if (kv.first == dead_lvl) kv.second.res_pend = false;
    else materialize_res(c, &kv.second);
  }
}
// before a write of the level's phi buffer buf (interior or ghost faces)
static void res_before_write(omg_ctx* c, Level* L, const double* buf) {
  if (!L->res_pend || L->res_src != buf) return;
  // inside a stand-alone cycle: these counts make the level's own passes write
  // the buffer, every cycle would pay the second launch
  if (c->in_full_cycle) L->res_pend_off = true;
  materialize_res(c, L);
}
// whether update_coarse's residual on a stand-alone cycle's top level may
// leave its res unstored
bool res_pend_ok(omg_ctx* c, const Level* L) {
  return c->n_ranks == 1 && !c->capturing && !c->no_res_pend && L->n && tiled_nc(L->nc) && !L->res_pend_off;
}

// --- the pending phi mean (Level::shift_pending): applied before anything
// that takes no shift reads phi
// The phi mean of a stand-alone cycle's subtract_mean is finished on the side
// stream (its chain overlaps the next cycle's rhs work); consumers wait here.
void phi_mean_ready(omg_ctx* c) {
  if (!c->phi_mean_on_side) return;
  c->phi_mean_on_side = false;
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_phi, 0));
  if (c->n_ranks > 1) mean_device(c, kChPhi, red_mean(c, kChPhi));
}
static void materialize_level(omg_ctx* c, Level* L) {
  if (!L->shift_pending) return;
  res_before_write(c, L, L->d_phi);
  phi_mean_ready(c);
  L->shift_pending = false;
  rb_stale_above(c, L->lvl);
  if (L->n) {
    Prof p(c, "subtract", (double)L->n * L->nc * L->nc * L->nc, L->lvl);
    launch_subtract(L->view(), 1, red_mean(c, kChPhi), 1, c->stream);
  }
}
void materialize_phi(omg_ctx* c) {
  if (!c->phi_shift_pending) return;
  for (auto& kv : c->levels) materialize_level(c, &kv.second);
  c->phi_shift_pending = false;
}

// --- the pending rhs shifts (Level::rhs_pend)
RhsShifts rhs_shifts(omg_ctx* c, const Level* L) {
  RhsShifts r;
  r.s = c->d_rhs_pend + (c->rhs_n - L->rhs_pend);
  r.n = L->rhs_pend;
  return r;
}
// The stored values catch up with the list; the box sums in the level's
// scratch and the chained sum are those of the same values and stay valid.
static void materialize_rhs(omg_ctx* c, Level* L) {
  if (!L->rhs_pend) return;
  // inside a stand-alone cycle: a reader that takes no list ran on this level
  if (c->in_full_cycle) L->rhs_pend_off = true;
  {
    Prof p(c, "subtract_rhs", (double)L->n * L->nc * L->nc * L->nc, L->lvl);
    launch_subtract_sums(L->sweep_view(), 2, L->d_leaves, L->n, rhs_shifts(c, L), nullptr, c->stream);
  }
  L->rhs_pend = 0;
  L->rhs_lex_ok = L->prox_rhs_ok = false;
}
void materialize_rhs_all(omg_ctx* c) {
  for (auto& kv : c->levels) materialize_rhs(c, &kv.second);
}
void rhs_pend_retry(omg_ctx* c) {
  for (auto& kv : c->levels) kv.second.rhs_pend_off = kv.second.res_pend_off = false;
}
// whether a cycle may leave the level's rhs - mean pending: its passes are
// the block passes that take the list
bool rhs_pend_ok(omg_ctx* c, const Level* L) {
  return c->n_ranks == 1 && c->smoother == OMG_SMOOTHER_GSRB && !c->no_rhs_pend && L->d_b3 && !L->b3_phys &&
         !L->rhs_pend_off;
}

// --- the caches of rhs: every write of a level's rhs drops its copies
void drop_rhs_lex(omg_ctx* c) {
  for (auto& kv : c->levels) kv.second.rhs_lex_ok = kv.second.prox_rhs_ok = false;
}
void drop_rhs_cache(omg_ctx* c) {
  c->rhs_cache_valid = false;
  drop_rhs_lex(c);
}

// --- one guard before each pass, one note after it
double* other_phi(const Level* L) { return L->d_phi == L->d_data ? L->d_phi_buf : L->d_data; }

void ready(omg_ctx* c, int lvl, unsigned pass) {
  Level* L = level_ptr(c, lvl);
  const bool writes = pass & (kWrite | kWriteOther);
  if (L) {
    // 1. a pending res is formed from its source buffer and rhs as they stand
    if (pass & kRhsWrite) materialize_res(c, L);
    else if (writes) res_before_write(c, L, pass & kWriteOther ? other_phi(L) : L->d_phi);
    if (pass & kResWrite) L->res_pend = false;
    // 2. the pending mean: taken by the pass, dead, or applied
    if (L->shift_pending) {
      if (pass & kPhiAbsorb) phi_mean_ready(c), L->shift_pending = false;
      else if (pass & kPhiDead) L->shift_pending = false;
      else if (pass & kPhi) materialize_level(c, L);
    }
    // 3. (under a pass that absorbs the mean the ghosts are formed from
    // unshifted values and shifted at its loads, like the interior)
    if ((pass & kGhosts) && L->gc_deferred) fill_gc_lvl(c, lvl, 1);
    // 4. the stored rhs catches up with its shifts
    if (pass & (kRhs | kRhsWrite)) materialize_rhs(c, L);
  }
  // 5. (also where this rank has no box of the level)
  if (writes) rb_stale_above(c, lvl);
}

void wrote(omg_ctx* c, int lvl, unsigned pass) {
  Level* L = level_ptr(c, lvl);
  if (!L) return;
  if (pass & kWriteOther) L->d_phi = other_phi(L);
  if (pass & (kGcAll | kGcNone | kGcStale)) {
    L->phi_gc_ok = pass & kGcAll;
    L->gc_deferred = pass & kGcNone;
  }
  if (pass & kRhsWrite) L->rhs_lex_ok = L->prox_rhs_ok = false;
}

// entry points other than the cycles: apply pending phi work first; `writes`
// = the call may change rhs (the cached rhs sum is dropped)
void enter(omg_ctx* c, bool writes) {
  // (a pending res first: it is formed from phi and rhs as they stand, the
  // shifts below subtract in place)
  materialize_res_all(c);
  materialize_rhs_all(c);
  materialize_phi(c);
  for (auto& kv : c->levels) ready(c, kv.first, kGhosts);
  if (writes) drop_rhs_cache(c);
}

}  // namespace host
}  // namespace omg
