// omg_mean.cpp — get_sum / subtract_mean for periodic problems: the leaf
// sums and the mean on the device.  What a stand-alone cycle's subtract_mean
// leaves pending (the phi shift, the rhs shifts) is kept by omg_lazy.cpp.
#include <algorithm>

#include "omg_host.h"

namespace omg {
namespace host {

// ---------------------------------------------------------------------------
// get_sum / subtract_mean on the device.  d_red slots: kAcc (this rank's sum,
// per channel phi / rhs), kMean (the mean), kAll (the gathered per-rank sums).
static double* red_acc(omg_ctx* c, int ch) { return c->d_red + ch; }
double* red_mean(omg_ctx* c, int ch) { return c->d_red + 2 + ch; }
static double* red_all(omg_ctx* c, int ch) { return c->d_red + 8 + (size_t)ch * c->n_ranks; }

// get_sum's loop (m_multigrid.f90:278-294) for this rank, in two parts: the
// per-leaf sums of every level (into the channel's scratch), then acc = 0 and
// the sequential chains level by level.  Scratch and acc of a channel may be
// in use by a chain on the side stream: writers wait for it first.
static double* leaf_scratch(Level* L, int ch) { return ch == kChRhs ? L->d_scratch_rhs : L->d_scratch; }

static void side_done(omg_ctx* c) {
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_side, 0));
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_phi, 0));
}

static void leaf_box_sums(omg_ctx* c, int iv, int ch, hipStream_t st) {
  for (int l = 1; l <= c->highest; l++) {
    Level* L = level_ptr(c, l);
    if (!L || L->leaves.empty()) continue;
    Prof p(c, "box_sums", (double)L->leaves.size() * L->nc * L->nc * L->nc, l, st);
    // (rhs: the sums of the values its pending shifts leave)
    launch_box_sums(L->sweep_view(), iv, L->d_leaves, (int)L->leaves.size(), leaf_scratch(L, ch), st,
                    iv == 2 ? rhs_shifts(c, L) : RhsShifts());
  }
}

static void leaf_chain(omg_ctx* c, int ch, hipStream_t st) {
  double* acc = red_acc(c, ch);
  bool first = true;   // get_sum = 0 (:283): the first chain starts from +0.0 itself
  for (int l = 1; l <= c->highest; l++) {
    Level* L = level_ptr(c, l);
    if (!L || L->leaves.empty()) continue;
    Prof p(c, "seq_sum", (double)L->leaves.size(), l, st);   // (timed on the stream it runs on)
    launch_seq_sum(leaf_scratch(L, ch), (int)L->leaves.size(), L->dr[0] * L->dr[1] * L->dr[2], acc, first, st);
    first = false;
  }
  if (first) HIPCHK(hipMemsetAsync(acc, 0, 8, st));
}

static void leaf_sum_device(omg_ctx* c, int iv, int ch) {
  side_done(c);
  leaf_box_sums(c, iv, ch, c->stream);
  leaf_chain(c, ch, c->stream);
}

static double subtract_volume(omg_ctx* c) {
  const int nc = c->box_size;
  const auto& d1 = c->drl[1];
  return (double)(nc * nc * nc) * (d1[0] * d1[1] * d1[2]) * (double)c->ids[1].size();
}

// MPI_Allreduce(acc) / volume into red_mean(ch), without leaving the stream
// (RCCL all-gather + k_mean); the loopback transport gathers on the host.
void mean_device(omg_ctx* c, int ch, double* mean) {
  const int n = c->n_ranks;
  if (n > 64) throw OmgError("subtract_mean: more than 64 ranks");
  double* all = red_all(c, ch);
  if (n == 1) {
    all = red_acc(c, ch);
  } else if (c->loop || c->host_xport) {
    HIPCHK(hipMemcpyAsync(c->h_scalar + 4, red_acc(c, ch), 8, hipMemcpyDeviceToHost, c->stream));
    host_sync(c, c->stream);
    std::vector<double> v = c->loop ? loop_allgather(c, c->h_scalar[4]) : host_allgather(c, c->h_scalar[4]);
    for (int r = 0; r < n; r++) c->h_scalar[8 + r] = v[r];
    HIPCHK(hipMemcpyAsync(all, c->h_scalar + 8, 8 * n, hipMemcpyHostToDevice, c->stream));
  } else {
    NCCLCHK(ncclAllGather(red_acc(c, ch), all, 1, ncclDouble, (ncclComm_t)c->nccl, c->stream));
  }
  launch_mean(all, n, subtract_volume(c), mean, c->stream);
}

// get_sum + MPI_Allreduce(sum) as one value on the host (omg_get_sum)
double get_sum(omg_ctx* c, int iv) {
  leaf_sum_device(c, iv, kChPhi);
  HIPCHK(hipMemcpyAsync(c->h_scalar + 2, red_acc(c, kChPhi), 8, hipMemcpyDeviceToHost, c->stream));
  host_sync(c, c->stream);
  return allreduce(c, c->h_scalar[2], false);
}

// subtract_mean (m_multigrid.f90:245-276), mean computed on the device.
// mode kInCycle: the standalone V-cycle's calls, where the next reads are
// known: rhs of levels whose boxes are all parents is overwritten by
// update_coarse before it is read (skipped), and phi -= mean is left pending:
// the first red-black substep of the next cycle subtracts it while loading
// (bit-identical), levels that restriction overwrites drop it, anything else
// applies it first (materialize_phi).
void subtract_mean(omg_ctx* c, int iv, int ghosts, int mode) {
  // (a stand-alone cycle resolves a pending res at its start, before its rhs
  // mean joins the list, and its phi pass only reads)
  if (mode != kInCycle) materialize_res_all(c);
  // subtracting from interior and ghosts keeps same-GPU / remote face ghosts
  // equal to a fill; physical and refinement-boundary ghosts are not.
  if (iv == 1) {
    materialize_phi(c);
    for (auto& kv : c->levels)
      if (!ghosts || kv.second.any_phys || kv.second.any_rb) kv.second.phi_gc_ok = false;
  }
  if (iv == 2 && (ghosts || mode != kInCycle)) materialize_rhs_all(c);
  if (iv == 2 && !ghosts) {
    // rhs: the sums may already be running on the side stream (see below)
    if (c->rhs_cache_valid) {
      HIPCHK(hipStreamWaitEvent(c->stream, c->ev_side, 0));
    } else {
      leaf_sum_device(c, 2, kChRhs);
    }
    c->rhs_cache_valid = false;
    // (split levels: proxies whose rhs was the owners' take the same
    // subtraction, bit for bit the owners' rhs - mean, and stay valid)
    std::vector<int> prox_kept;
    for (auto& kv : c->levels)
      if (kv.second.prox_rhs_ok) prox_kept.push_back(kv.first);
    drop_rhs_lex(c);
    // the mean goes to the end of the list of pending shifts (empty again
    // once no level has any pending); a full list is written out by this
    // cycle, its own mean included
    bool any_pend = false;
    for (auto& kv : c->levels) any_pend = any_pend || kv.second.rhs_pend > 0;
    if (!any_pend) c->rhs_n = 0;
    const bool list_full = c->rhs_n >= kRhsPendMax;
    double* mean = c->d_rhs_pend + c->rhs_n;
    mean_device(c, kChRhs, mean);
    bool all_fused = true;
    for (int l = c->lowest; l <= c->highest; l++) {
      Level* L = level_ptr(c, l);
      if (!L || !L->n) continue;
      if (mode == kInCycle && L->all_parents) continue;
      if (L->n_prox && std::count(prox_kept.begin(), prox_kept.end(), l)) {
        LevelView P = L->view();   // the proxies as boxes 0 .. n_prox-1
        P.data += (long long)L->n * L->stride;
        P.phi += (long long)L->n * L->stride;
        P.n = L->n_prox;
        launch_subtract(P, 2, mean, 0, c->stream);
        L->prox_rhs_ok = true;
      }
      const double cells = (double)L->n * L->nc * L->nc * L->nc;
      if (l >= 1 && (int)L->leaves.size() == L->n && subtract_sums_nc(L->nc)) {
        // the level's pending shifts and the new mean; either form leaves the
        // box sums of the shifted values for the next get_sum
        RhsShifts rs = rhs_shifts(c, L);
        rs.n++;
        if (mode == kInCycle && !list_full && rhs_pend_ok(c, L)) {
          Prof p(c, "box_sums", cells, l);
          launch_box_sums(L->sweep_view(), 2, L->d_leaves, L->n, L->d_scratch_rhs, c->stream, rs);
          L->rhs_pend++;
        } else {
          Prof p(c, "subtract_rhs", cells, l);
          launch_subtract_sums(L->sweep_view(), 2, L->d_leaves, L->n, rs, L->d_scratch_rhs, c->stream);
          L->rhs_pend = 0;
        }
      } else {
        ready(c, l, kRhs);   // (never pending here: such a level's cycles subtract at once)
        Prof p(c, "subtract_rhs", cells, l);
        launch_subtract(L->view(), 2, mean, 0, c->stream);
        if (l >= 1 && !L->leaves.empty()) all_fused = false;
      }
    }
    c->rhs_n = list_full ? 0 : c->rhs_n + 1;
    if (all_fused) {
      // the next get_sum(rhs): its leaf sums were produced by the fused
      // kernels; its sequential chain runs now on the side stream
      HIPCHK(hipEventRecord(c->ev_main, c->stream));
      HIPCHK(hipStreamWaitEvent(c->stream2, c->ev_main, 0));
      leaf_chain(c, kChRhs, c->stream2);
      HIPCHK(hipEventRecord(c->ev_side, c->stream2));
      c->rhs_cache_valid = true;
    }
    return;
  }
  if (iv == 2) drop_rhs_cache(c);
  const int ch = iv == 2 ? kChRhs : kChPhi;
  if (iv == 1 && ghosts && mode == kInCycle) {
    // leaf sums now, chain (+ mean on one rank) on the side stream; the next
    // cycle's rhs work overlaps it and phi_mean_ready() joins before use
    side_done(c);
    leaf_box_sums(c, 1, kChPhi, c->stream);
    HIPCHK(hipEventRecord(c->ev_main, c->stream));
    HIPCHK(hipStreamWaitEvent(c->stream2, c->ev_main, 0));
    leaf_chain(c, kChPhi, c->stream2);
    if (c->n_ranks == 1) launch_mean(red_acc(c, kChPhi), 1, subtract_volume(c), red_mean(c, kChPhi), c->stream2);
    HIPCHK(hipEventRecord(c->ev_phi, c->stream2));
    c->phi_mean_on_side = true;
    for (auto& kv : c->levels) kv.second.shift_pending = kv.second.n > 0;
    c->phi_shift_pending = true;
    return;
  }
  leaf_sum_device(c, iv, ch);
  mean_device(c, ch, red_mean(c, ch));
  for (int l = c->lowest; l <= c->highest; l++) {
    Level* L = level_ptr(c, l);
    // (phi of every level changes: the refinement-boundary coarse parts the
    // level above stored, Level::rbgv_ok, are those of the old phi)
    if (L && iv == 1) L->rbgv_ok = false;
    if (L && iv == 2 && ghosts) rhs_ghosts_written(c, l);
    if (L && L->n) {
      Prof p(c, "subtract", (double)L->n * L->nc * L->nc * L->nc, l);
      launch_subtract(L->view(), iv, red_mean(c, ch), ghosts, c->stream);
    }
  }
}

}  // namespace host
}  // namespace omg
