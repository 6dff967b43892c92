// omg_api.cpp — the C-ABI (include/omg.h): context lifetime, tree setup,
// upload / download, and one guarded entry point per routine of the other
// host units (omg_host.h lists them).
#include <algorithm>

#include "omg_host.h"

using namespace omg;
using namespace omg::host;

thread_local bool omg::host::g_host_only = false;

namespace {

thread_local std::string g_last_error;

template <typename F>
int guarded(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return 1;
  }
}

void resolve_stats(omg_ctx* c) {
  if (c->pending.empty()) return;
  for (auto& p : c->pending) {
    float ms = 0;
    HIPCHK(hipEventSynchronize(p.e1));
    HIPCHK(hipEventElapsedTime(&ms, p.e0, p.e1));
    for (int pass = 0; pass < (p.lvl == NO_LVL ? 1 : 2); pass++) {
      auto& s = c->stats[pass ? std::string(p.name) + "@" + std::to_string(p.lvl) : std::string(p.name)];
      s.launches++;
      s.ms += ms;
      s.cells += p.cells;
    }
    (void)hipEventDestroy(p.e0);
    (void)hipEventDestroy(p.e1);
  }
  c->pending.clear();
}

// staging buffer in the reference's box layout
double* stage(omg_ctx* c, size_t n) {
  if (n > c->stage_n) {
    dfree(c->d_stage);
    HIPCHK(hipMalloc(&c->d_stage, sizeof(double) * n));
    c->stage_n = n;
  }
  return c->d_stage;
}

}  // namespace

// ===========================================================================
// C-ABI
extern "C" {

const char* omg_last_error(void) { return g_last_error.c_str(); }

int omg_get_unique_id(void* out) {
  return guarded([&] {
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    std::memcpy(out, &id, sizeof(id));
  });
}

int omg_loopback_unique_id(long long tag, void* out) {
  return guarded([&] {
    loopback_unique_id(tag, out);
  });
}

int omg_host_unique_id(void* out) {
  return guarded([&] {
    host_unique_id(out);
  });
}

int omg_set_host_transport(omg_ctx* c, omg_host_exchange_fn exchange, omg_host_allgather_fn allgather, void* user) {
  return guarded([&] {
    if (!c->host_xport) throw OmgError("omg_set_host_transport: the context was not created with omg_host_unique_id");
    c->hx_exchange = exchange;
    c->hx_allgather = allgather;
    c->hx_user = user;
  });
}

int omg_device_count(int* n) {
  return guarded([&] { HIPCHK(hipGetDeviceCount(n)); });
}

int omg_ctx_create(omg_ctx** out, int device, int rank, int n_ranks, const void* unique_id) {
  return guarded([&] {
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) throw OmgError("bad rank / n_ranks");
    if (n_ranks > 1 && !unique_id && device != OMG_DEVICE_NONE)
      throw OmgError("unique_id required for n_ranks > 1");
    // the switches the communication plan depends on (read by plan-only
    // contexts too, whose plans the CPU tests pair up)
    auto plan_switches = [](omg_ctx* c) {
      c->no_block3 = env_flag("OMG_NO_BLOCK3");
      c->no_block3_phys = env_flag("OMG_NO_BLOCK3_PHYS");
      c->no_deep = env_flag("OMG_NO_DEEP");
      // (tests: the smallest level k_gsrb3 serves; OMG_BLOCK3_MIN_BOXES)
      if (const char* v = getenv("OMG_BLOCK3_MIN_BOXES")) c->b3_min_boxes = std::max(1, atoi(v));
      // (tests: the column length, 2 .. 16 boxes, even; OMG_BLOCK3_COLUMN)
      if (const char* v = getenv("OMG_BLOCK3_COLUMN")) c->b3_col = std::min(std::max(2, atoi(v) & ~1), kB3MaxZ);
      if (const char* v = getenv("OMG_BLOCK3_SMALL_COL")) c->b3_col_small = std::min(std::max(2, atoi(v) & ~1), kB3MaxZ);
    };
    if (device == OMG_DEVICE_NONE) {   // plan-only context: no HIP, no RCCL
      omg_ctx* c = new omg_ctx();
      c->device = device;
      c->rank = rank;
      c->n_ranks = n_ranks;
      c->host_only = true;
      plan_switches(c);
      *out = c;
      return;
    }
    if (device < 0) {   // one rank per GPU: rank modulo the visible devices
      int n_dev = 0;
      HIPCHK(hipGetDeviceCount(&n_dev));
      if (n_dev < 1) throw OmgError("no HIP device visible");
      device = rank % n_dev;
    }
    omg_ctx* c = new omg_ctx();
    c->device = device;
    c->rank = rank;
    c->n_ranks = n_ranks;
    c->no_tail = env_flag("OMG_NO_TAIL");
    c->no_fuse_up = env_flag("OMG_NO_FUSE_UP");
    c->no_skip1 = env_flag("OMG_NO_SKIP1");
    c->tail_timing = env_flag("OMG_TAIL_TIMING");
    c->no_fill_tile = env_flag("OMG_NO_FILL_TILE");
    c->no_fill_crhs = env_flag("OMG_NO_FILL_CRHS");
    c->no_tail_crhs = env_flag("OMG_NO_TAIL_CRHS");
    c->no_rbgv = env_flag("OMG_NO_RBGV");
    c->no_graph = !env_flag("OMG_GRAPH");
    c->no_fuse_down = env_flag("OMG_NO_FUSE_DOWN");
    c->no_rb_fill_fuse = env_flag("OMG_NO_RB_FUSE");
    c->no_gs_plane = env_flag("OMG_NO_GS_PLANE");
    c->no_fill_xl = env_flag("OMG_NO_FILL_XL");
    c->no_gs_dbl = env_flag("OMG_NO_GS_DBL");
    plan_switches(c);
    c->no_block3p = env_flag("OMG_NO_BLOCK3P");
    c->no_block3r = env_flag("OMG_NO_BLOCK3R");
    c->block4 = !env_flag("OMG_NO_BLOCK4");
    c->no_block4p = env_flag("OMG_NO_BLOCK4P");
    c->block4_phys = env_flag("OMG_BLOCK4_PHYS");
    c->no_defer_gc = env_flag("OMG_NO_DEFER_GC");
    c->no_rhs_pend = env_flag("OMG_NO_RHS_PEND");
    c->no_res_pend = env_flag("OMG_NO_RES_PEND");
    c->no_fuse_down_bc = env_flag("OMG_NO_FUSE_DOWN_BC");
    c->roctx = env_flag("OMG_ROCTX");
    c->debug = env_flag("OMG_DEBUG");
    // (on under OMG_DEBUG too: a rank that uploads phi alone would otherwise
    // make halo exchanges the others skip, a hang or mispaired messages)
    c->check_collective = env_flag("OMG_CHECK_COLLECTIVE") || c->debug;
    if (const char* v = getenv("OMG_GRAPH_FAIL")) c->graph_fail_at = std::atoi(v);   // tests only
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipMalloc(&c->d_scalar, sizeof(double) * (64 + 2 * (size_t)n_ranks)));
    HIPCHK(hipMalloc(&c->d_red, sizeof(double) * (8 + 2 * (size_t)n_ranks)));
    HIPCHK(hipMemset(c->d_red, 0, sizeof(double) * (8 + 2 * (size_t)n_ranks)));
    HIPCHK(hipMalloc(&c->d_rhs_pend, sizeof(double) * (omg::kRhsPendMax + 1)));
    HIPCHK(hipMemset(c->d_rhs_pend, 0, sizeof(double) * (omg::kRhsPendMax + 1)));
    HIPCHK(hipMalloc(&c->d_maxslots, sizeof(unsigned long long) * omg::kMaxSlots * omg::kMaxSlotStride));
    // (allocated here: no allocation may happen while a cycle is captured)
    HIPCHK(hipMalloc(&c->d_tail, sizeof(TailArgs)));
    c->h_tail = new TailArgs;
    std::memset(c->h_tail, 0xff, sizeof(TailArgs));
    HIPCHK(hipMemset(c->d_maxslots, 0, sizeof(unsigned long long) * omg::kMaxSlots * omg::kMaxSlotStride));
    HIPCHK(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
    {
      // the halo stream at the highest priority: its RCCL kernels are queued
      // behind the boundary boxes while an interior substep of thousands of
      // workgroups fills every CU; priority lets the dispatcher place them first
      int least = 0, greatest = 0;
      HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
      HIPCHK(hipStreamCreateWithPriority(&c->stream_comm, hipStreamNonBlocking, greatest));
      c->comm_priority = greatest;
    }
    HIPCHK(hipEventCreateWithFlags(&c->ev_bnd, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_comm, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_side, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_phi, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_dense_in, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_dense_out, hipEventDisableTiming));
    HIPCHK(hipHostMalloc(&c->h_scalar, sizeof(double) * (16 + (size_t)n_ranks)));
    for (int iv = 0; iv < kMaxVars; iv++)
      for (int nb = 0; nb < 6; nb++) {
        c->bc[iv].type[nb] = OMG_BC_DIRICHLET;
        c->bc[iv].value[nb] = 0.0;
      }
    transport_attach(c, unique_id);
    *out = c;
  });
}

int omg_ctx_destroy(omg_ctx* c) {
  return guarded([&] {
    if (!c) return;
    if (c->host_only) {
      g_host_only = true;
      free_levels(c);
      g_host_only = false;
      delete c;
      return;
    }
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->stream2);
    (void)hipStreamSynchronize(c->stream_comm);
    free_levels(c);
    dfree(c->d_scalar);
    if (c->d_tail) (void)hipFree(c->d_tail);
    if (c->d_tail_stamps) (void)hipFree(c->d_tail_stamps);
    delete c->h_tail;
    dfree(c->d_red);
    dfree(c->d_rhs_pend);
    dfree(c->d_maxslots);
    for (auto& kv : c->graphs)
      if (kv.second) (void)hipGraphExecDestroy(kv.second);
    c->graphs.clear();
    dfree(c->d_stage);
    if (c->ev_main) (void)hipEventDestroy(c->ev_main);
    if (c->ev_side) (void)hipEventDestroy(c->ev_side);
    if (c->ev_phi) (void)hipEventDestroy(c->ev_phi);
    if (c->ev_dense_in) (void)hipEventDestroy(c->ev_dense_in);
    if (c->ev_dense_out) (void)hipEventDestroy(c->ev_dense_out);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->stream_comm) (void)hipStreamDestroy(c->stream_comm);
    if (c->ev_bnd) (void)hipEventDestroy(c->ev_bnd);
    if (c->ev_comm) (void)hipEventDestroy(c->ev_comm);
    if (c->h_scalar) (void)hipHostFree(c->h_scalar);
    if (c->h_xsend) (void)hipHostFree(c->h_xsend);
    if (c->h_xrecv) (void)hipHostFree(c->h_xrecv);
    transport_detach(c);
    (void)hipStreamDestroy(c->stream);
    delete c;
  });
}

int omg_tree_setup(omg_ctx* c, int n_boxes, const int* lvl, const int* parent, const int* children,
                   const int* neighbors, const int* ix, const int* rank, int lowest_lvl,
                   int highest_lvl, int first_normal_lvl, int box_size, const int* box_size_lvl,
                   const double* dr, const int* list_off, const int* lists, int n_vars) {
  return guarded([&] {
    if (n_vars < 4 || n_vars > kMaxVars) throw OmgError("n_vars out of range");
    struct HostOnly {
      explicit HostOnly(bool on) { g_host_only = on; }
      ~HostOnly() { g_host_only = false; }
    } host_only_scope(c->host_only);
    if (!c->host_only) (void)hipSetDevice(c->device);
    free_levels(c);
    c->n_boxes = n_boxes;
    c->lvl.assign(lvl, lvl + n_boxes);
    c->parent.assign(parent, parent + n_boxes);
    c->children.assign(children, children + 8 * (size_t)n_boxes);
    c->neighbors.assign(neighbors, neighbors + 6 * (size_t)n_boxes);
    c->ix.assign(ix, ix + 3 * (size_t)n_boxes);
    c->rank_of.assign(rank, rank + n_boxes);
    c->lowest = lowest_lvl;
    c->highest = highest_lvl;
    c->first_normal = first_normal_lvl;
    c->box_size = box_size;
    c->n_vars = n_vars;
    c->bsl.clear();
    c->drl.clear();
    c->ids.clear(); c->leaves.clear(); c->parents.clear(); c->ref_bnds.clear();
    for (int l = lowest_lvl; l <= highest_lvl; l++) {
      const int li = l - lowest_lvl;
      c->bsl[l] = box_size_lvl[li];
      c->drl[l] = {dr[3 * li], dr[3 * li + 1], dr[3 * li + 2]};
      std::map<int, std::vector<int>>* dst[4] = {&c->ids, &c->leaves, &c->parents, &c->ref_bnds};
      for (int t = 0; t < 4; t++) {
        const int a = list_off[4 * li + t], b = list_off[4 * li + t + 1];
        (*dst[t])[l] = std::vector<int>(lists + a, lists + b);
      }
    }
    if (!c->host_only) {
      host_sync(c, c->stream);
      host_sync(c, c->stream2);
    }
    c->rhs_cache_valid = false;
    c->phi_shift_pending = false;
    c->phi_mean_on_side = false;
    build_plan(c);
    if (!c->host_only) HIPCHK(hipDeviceSynchronize());
  });
}

int omg_plan_transfer(omg_ctx* c, int lvl, int which, int dir, int cap, int* peers, long long* keys,
                      int* n_items, int* item_doubles) {
  return guarded([&] {
    Level* L = level_ptr(c, lvl);
    if (!L) throw OmgError("no such level");
    if (which < 0 || which > 5) throw OmgError("omg_plan_transfer: bad transfer");
    const Transfer* T[6] = {&L->halo, &L->restr, &L->prol, &L->rbx, &L->repl, &L->deep_phi};
    const auto& lists = dir ? T[which]->recv : T[which]->send;
    int n = 0;
    for (auto& p : lists)
      for (long long k : p.keys) {
        if (n < cap) {
          peers[n] = p.peer;
          keys[n] = k;
        }
        n++;
      }
    *n_items = n;
    *item_doubles = T[which]->item_doubles;
  });
}

int omg_plan_columns(omg_ctx* c, int lvl, int which, int cap, int* recs, int* n_cols, int* rec_ints) {
  return guarded([&] {
    const Level* L = level_ptr(c, lvl);
    if (!L) throw OmgError("no such level");
    if (which < 0 || which > 1) throw OmgError("omg_plan_columns: bad table");
    const std::vector<int>& h = columns_host(*L, which, rec_ints);
    *n_cols = (int)(h.size() / *rec_ints);
    if (cap > 0 && (size_t)cap >= h.size()) std::copy(h.begin(), h.end(), recs);
  });
}

int omg_set_operator(omg_ctx* c, int op, double lambda) {
  return guarded([&] { set_operator(c, op, lambda); });
}

int omg_set_smoother(omg_ctx* c, int smoother, int n_cycle_down, int n_cycle_up, int max_coarse_cycles,
                     double res_abs, double res_rel) {
  return guarded([&] {
    if (smoother != OMG_SMOOTHER_GS && smoother != OMG_SMOOTHER_GSRB)
      throw OmgError("unsupported smoother type");
    if (smoother != c->smoother || std::max(n_cycle_down, 0) != c->n_cycle_down ||
        std::max(n_cycle_up, 0) != c->n_cycle_up)
      rhs_pend_retry(c);
    c->smoother = smoother;
    c->n_substeps = smoother == OMG_SMOOTHER_GSRB ? 2 : 1;
    ensure_rhs_lex(c);
    // (negative counts: the reference's loops run zero times, m_multigrid.f90:407)
    c->n_cycle_down = std::max(n_cycle_down, 0);
    c->n_cycle_up = std::max(n_cycle_up, 0);
    c->max_coarse_cycles = max_coarse_cycles;
    c->res_abs = res_abs;
    c->res_rel = res_rel;
  });
}

int omg_set_subtract_mean(omg_ctx* c, int on) {
  return guarded([&] { c->subtract_mean = on; });
}

int omg_set_bc(omg_ctx* c, int iv, int nb, int bc_type, double bc_value) {
  return guarded([&] {
    if (iv < 1 || iv > kMaxVars || nb < 1 || nb > 6) throw OmgError("omg_set_bc: bad iv/nb");
    // (deferred ghosts are filled under the old condition first, as the
    // reference's last fill formed them; then every level's ghosts are stale)
    enter(c, false);
    phi_dirty_all(c);
    c->bc[iv - 1].type[nb - 1] = bc_type;
    c->bc[iv - 1].value[nb - 1] = bc_value;
  });
}

int omg_set_bc_faces(omg_ctx* c, int iv, const long long* face_off, const int* face_type,
                     const double* data, long long n_data) {
  return guarded([&] {
    if (iv < 1 || iv > kMaxVars) throw OmgError("omg_set_bc_faces: bad iv");
    if (!c->host_only) enter(c, false);   // (as omg_set_bc)
    phi_dirty_all(c);
    const int k = iv - 1;
    for (auto& kv : c->d_face_off_lvl[k]) dfree(kv.second);
    for (auto& kv : c->d_face_type_lvl[k]) dfree(kv.second);
    c->d_face_off_lvl[k].clear();
    c->d_face_type_lvl[k].clear();
    c->h_face_off_lvl[k].clear();
    c->h_face_type_lvl[k].clear();
    dfree(c->d_face_data[k]);
    if (!face_off) return;
    // only the faces of my boxes travel to the device, re-packed
    std::vector<double> packed;
    for (auto& kv : c->levels) {
      Level& L = kv.second;
      if (!L.n) continue;
      std::vector<long long> off(L.n * 6, -1);
      std::vector<int> typ(L.n * 6, 0);
      const long long n2 = (long long)L.nc * L.nc;
      if (L.replicated) {
        // every copy needs the table: a face tabulated for one box of the
        // level must be tabulated for every box with that physical face
        bool any[6] = {}, miss[6] = {};
        for (int b = 0; b < L.n; b++)
          for (int nb = 0; nb < 6; nb++) {
            if (L.h_nbk[(size_t)b * 6 + nb] != NB_PHYS) continue;
            (face_off[(size_t)(L.ids[b] - 1) * 6 + nb] >= 0 ? any : miss)[nb] = true;
          }
        for (int nb = 0; nb < 6; nb++)
          if (any[nb] && miss[nb])
            throw OmgError("omg_set_bc_faces: replicated level " + std::to_string(L.lvl) +
                           " needs the boundary table of every box (omg_replicated_level)");
      }
      for (int b = 0; b < L.n; b++)
        for (int nb = 0; nb < 6; nb++) {
          const long long o = face_off[(size_t)(L.ids[b] - 1) * 6 + nb];
          if (o < 0) continue;
          if (o + n2 > n_data) throw OmgError("omg_set_bc_faces: offset out of range");
          off[b * 6 + nb] = (long long)packed.size();
          typ[b * 6 + nb] = face_type[(size_t)(L.ids[b] - 1) * 6 + nb];
          packed.insert(packed.end(), data + o, data + o + n2);
        }
      c->d_face_off_lvl[k][kv.first] = to_device(off);
      c->d_face_type_lvl[k][kv.first] = to_device(typ);
      c->h_face_off_lvl[k][kv.first] = off;
      c->h_face_type_lvl[k][kv.first] = typ;
    }
    c->d_face_data[k] = to_device(packed);
  });
}

int omg_level_size(omg_ctx* c, int lvl, int* n_boxes, int* nc) {
  return guarded([&] {
    Level* L = level_ptr(c, lvl);
    if (!L) throw OmgError("no such level");
    *n_boxes = (int)L->host_local.size();
    *nc = L->nc;
  });
}

int omg_set_coarse_replication(omg_ctx* c, long long max_cells) {
  return guarded([&] {
    if (!c->levels.empty()) throw OmgError("omg_set_coarse_replication: call before omg_tree_setup");
    if (max_cells < 0) throw OmgError("omg_set_coarse_replication: max_cells < 0");
    c->rep_cells = max_cells;
  });
}

int omg_replicated_level(omg_ctx* c, int* lvl) {
  return guarded([&] { *lvl = c->rep_lvl == INT_MIN ? c->lowest - 1 : c->rep_lvl; });
}

int omg_upload_level(omg_ctx* c, int lvl, int iv, const double* host) {
  return guarded([&] {
    enter(c);
    Level* L = level_ptr(c, lvl);
    if (!L) throw OmgError("no such level");
    if (iv < 1 || iv > c->n_vars) throw OmgError("bad variable index");
    // (before the early return: a rank without boxes here still drops the
    // flag, which the multi-rank stand-alone fill decision relies on)
    if (iv == 1) phi_dirty(c, lvl);
    if (iv == 2) rhs_ghosts_written(c, lvl);   // (the upload writes the ghost slots too)
    if (!L->n) return;
    const size_t s = L->nc + 2, box = s * s * s, n = box * L->n;
    double* st = stage(c, n);
    if (L->replicated) {
      // the host's boxes into their slots, then to every peer (collective)
      std::vector<double> full(n, 0.0);
      for (size_t q = 0; q < L->host_local.size(); q++)
        std::memcpy(full.data() + box * L->host_local[q], host + box * q, sizeof(double) * box);
      HIPCHK(hipMemcpyAsync(st, full.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
      launch_from_ref(L->view(), iv, st, c->stream);
      if (L->repl.n_send || L->repl.n_recv) {
        launch_box_pack(L->view(), iv, L->repl.d_send_items, L->repl.n_send, L->d_sendbuf, c->stream);
        exchange(c, L->repl, L->d_sendbuf, L->d_recvbuf, nullptr, lvl);
        launch_box_unpack(L->view(), iv, L->repl.d_recv_items, L->repl.n_recv, L->d_recvbuf, c->stream);
      }
      host_sync(c, c->stream);
      return;
    }
    HIPCHK(hipMemcpyAsync(st, host, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    launch_from_ref(L->view(), iv, st, c->stream);
    host_sync(c, c->stream);
  });
}

int omg_download_level(omg_ctx* c, int lvl, int iv, double* host) {
  return guarded([&] {
    enter(c, false);
    Level* L = level_ptr(c, lvl);
    if (!L) throw OmgError("no such level");
    if (iv < 1 || iv > c->n_vars) throw OmgError("bad variable index");
    if (!L->n) return;
    const size_t s = L->nc + 2, box = s * s * s, n = box * L->n;
    double* st = stage(c, n);
    launch_to_ref(L->view(), iv, st, c->debug ? snan_value() : 0.0, c->stream);
    if (L->replicated) {   // the host's boxes only
      std::vector<double> full(n);
      HIPCHK(hipMemcpyAsync(full.data(), st, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
      host_sync(c, c->stream);
      for (size_t q = 0; q < L->host_local.size(); q++)
        std::memcpy(host + box * q, full.data() + box * L->host_local[q], sizeof(double) * box);
      return;
    }
    HIPCHK(hipMemcpyAsync(host, st, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    host_sync(c, c->stream);
  });
}

int omg_put_dense(omg_ctx* c, int lvl, int iv, const double* dev, const long long* lo, const long long* n,
                  const long long* stride, void* stream, long long* n_cells) {
  return guarded([&] { dense_io(c, lvl, iv, const_cast<double*>(dev), lo, n, stride, stream, n_cells, true); });
}

int omg_get_dense(omg_ctx* c, int lvl, int iv, double* dev, const long long* lo, const long long* n,
                  const long long* stride, void* stream, long long* n_cells) {
  return guarded([&] { dense_io(c, lvl, iv, dev, lo, n, stride, stream, n_cells, false); });
}

int omg_get_dense_grad(omg_ctx* c, int lvl, int iv, double* const* dev, const long long* lo, const long long* n,
                       const long long* stride, double scale, int fill, void* stream, long long* n_cells) {
  return guarded([&] { dense_grad(c, lvl, iv, dev, lo, n, stride, scale, fill != 0, stream, n_cells); });
}

int omg_put_boxes(omg_ctx* c, int iv, int n_boxes, const int* ids, const double* dev, const long long* box_off,
                  const long long* stride, int ghost, void* stream, long long* n_cells) {
  return guarded([&] {
    box_io(c, iv, n_boxes, ids, const_cast<double*>(dev), box_off, stride, ghost, false, stream, n_cells, true);
  });
}

int omg_get_boxes(omg_ctx* c, int iv, int n_boxes, const int* ids, double* dev, const long long* box_off,
                  const long long* stride, int ghost, int fill, void* stream, long long* n_cells) {
  return guarded([&] { box_io(c, iv, n_boxes, ids, dev, box_off, stride, ghost, fill != 0, stream, n_cells, false); });
}

int omg_get_boxes_grad(omg_ctx* c, int iv, int n_boxes, const int* ids, double* const* dev, const long long* box_off,
                       const long long* stride, double scale, int centering, int fill, void* stream,
                       long long* n_cells) {
  return guarded([&] {
    boxes_grad(c, iv, n_boxes, ids, dev, box_off, stride, scale, centering, fill != 0, stream, n_cells);
  });
}

int omg_put_boxes_div(omg_ctx* c, int iv, int n_boxes, const int* ids, const double* const* dev,
                      const long long* box_off, const long long* stride, double scale, int centering, void* stream,
                      long long* n_cells) {
  return guarded([&] { boxes_div(c, iv, n_boxes, ids, dev, box_off, stride, scale, centering, stream, n_cells); });
}

int omg_get_boxes_flux(omg_ctx* c, int iv, const int* iv_coef, int n_boxes, const int* ids, double* const* dev,
                       const long long* box_off, const long long* stride, double scale, int centering, int accumulate,
                       int fill, void* stream, long long* n_cells) {
  return guarded([&] {
    boxes_flux(c, iv, iv_coef, n_boxes, ids, dev, box_off, stride, scale, centering, accumulate != 0, fill != 0,
               stream, n_cells);
  });
}

int omg_fas_vcycle(omg_ctx* c, int highest_lvl, int want_max_res, double* max_res, int standalone) {
  return guarded([&] {
    const double r = run_cycle(c, 1 + (want_max_res ? 2 : 0) + 4 * (standalone != 0) + 8 * (highest_lvl + 64),
                               [&] { return fas_vcycle(c, highest_lvl, want_max_res != 0, standalone != 0); });
    if (want_max_res && max_res) *max_res = r;
    if (want_max_res) check_finite_res(r, "mg_fas_vcycle");
  });
}

int omg_fas_fmg(omg_ctx* c, int have_guess, int want_max_res, double* max_res) {
  return guarded([&] {
    const double r = run_cycle(c, 2 + (want_max_res ? 2 : 0) + 4 * (have_guess != 0),
                               [&] { return fas_fmg(c, have_guess != 0, want_max_res != 0); });
    if (want_max_res && max_res) *max_res = r;
    if (want_max_res) check_finite_res(r, "mg_fas_fmg");
  });
}

int omg_apply_op(omg_ctx* c, int i_out) {
  return guarded([&] { apply_op(c, i_out); });
}

int omg_set_rhs(omg_ctx* c, double f1, double f2) {
  return guarded([&] { set_rhs(c, f1, f2); });
}

int omg_diffusion_solve(omg_ctx* c, int op, double dt, double diffusion_coeff, int order, double max_res,
                        int* n_vcycles, double* res) {
  return guarded([&] { diffusion_solve(c, op, dt, diffusion_coeff, order, max_res, n_vcycles, res); });
}

int omg_restrict(omg_ctx* c, int iv) {
  return guarded([&] {
    enter(c);
    for (int l = c->highest; l >= c->lowest + 1; l--) restrict_lvl(c, iv, l);
  });
}
int omg_restrict_lvl(omg_ctx* c, int iv, int lvl) {
  return guarded([&] {
    enter(c);
    restrict_lvl(c, iv, lvl);
  });
}
int omg_fill_ghost_cells(omg_ctx* c, int iv) {
  return guarded([&] {
    enter(c);
    for (int l = c->lowest; l <= c->highest; l++) fill_gc_lvl(c, l, iv);
  });
}
int omg_fill_ghost_cells_lvl(omg_ctx* c, int lvl, int iv) {
  return guarded([&] {
    enter(c);
    fill_gc_lvl(c, lvl, iv);
  });
}
int omg_prolong(omg_ctx* c, int lvl, int iv, int iv_to, int add) {
  return guarded([&] {
    enter(c);
    prolong(c, lvl, iv, iv_to, add);
  });
}
int omg_smooth_boxes(omg_ctx* c, int lvl, int n_cycle) {
  return guarded([&] {
    enter(c);
    smooth_boxes(c, lvl, n_cycle);
  });
}
int omg_update_coarse(omg_ctx* c, int lvl) {
  return guarded([&] {
    enter(c);
    update_coarse(c, lvl);
  });
}
int omg_correct_children(omg_ctx* c, int lvl) {
  return guarded([&] {
    enter(c);
    correct_children(c, lvl);
  });
}
int omg_residual_lvl(omg_ctx* c, int lvl) {
  return guarded([&] {
    enter(c);
    residual_lvl(c, lvl, nullptr);
  });
}
int omg_max_residual_lvl(omg_ctx* c, int lvl, double* out) {
  return guarded([&] {
    enter(c);
    *out = max_residual_lvl(c, lvl);
    check_finite_res(*out, "max_residual_lvl");
  });
}
int omg_get_sum(omg_ctx* c, int iv, double* out) {
  return guarded([&] {
    enter(c, false);
    *out = get_sum(c, iv);
  });
}
int omg_subtract_mean(omg_ctx* c, int iv, int include_ghostcells) {
  return guarded([&] {
    // deferred ghosts are filled first: an interior-only subtraction leaves
    // the ghosts of the last fill as they are (m_multigrid.f90:262-273), and a
    // fill made afterwards would form them from the subtracted interior.  The
    // cached rhs sums stay: subtract_mean itself follows its writes of rhs
    enter(c, false);
    subtract_mean(c, iv, include_ghostcells);
  });
}

// mg_phi_bc_store (m_ghost_cells.f90:66-117): the bc values of phi go into
// the rhs ghost cells and the bc type into the neighbour slot.
int omg_phi_bc_store(omg_ctx* c) {
  return guarded([&] {
    enter(c);
    phi_bc_store(c);
  });
}

int omg_poisson_free_3d(omg_ctx* c, int new_rhs, double max_fft_frac, int fmgcycle, int want_max_res,
                        double* max_res, const double* r_min, const double* box_r_min) {
  return guarded([&] {
    enter(c);
    const double r = poisson_free_3d(c, new_rhs != 0, max_fft_frac, fmgcycle != 0, want_max_res != 0, r_min,
                                     box_r_min);
    if (max_res && want_max_res) *max_res = r;
    if (want_max_res) check_finite_res(r, "mg_poisson_free_3d");
  });
}

int omg_free_planes(omg_ctx* c, int* fft_lvl, int* nx, double* planes, long long cap) {
  return guarded([&] {
    omg_free_state* S = c->free_state;
    if (!S || !S->initialized) throw OmgError("omg_free_planes: no free-space solve yet");
    *fft_lvl = S->fft_lvl;
    for (int d = 0; d < 3; d++) nx[d] = S->G.nx[d];
    const size_t n = 2 * ((size_t)nx[1] * nx[2] + (size_t)nx[0] * nx[2] + (size_t)nx[0] * nx[1]);
    if (planes && cap >= (long long)n) {
      HIPCHK(hipMemcpyAsync(planes, S->d_planes, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
      host_sync(c, c->stream);
    }
  });
}

int omg_comm_info(omg_ctx* c, int* n_ranks, int* transport) {
  return guarded([&] {
    if (c->nccl) {
      NCCLCHK(ncclCommCount((ncclComm_t)c->nccl, n_ranks));
      *transport = OMG_TRANSPORT_RCCL;
    } else if (c->loop) {
      *n_ranks = c->loop->n_ranks;
      *transport = OMG_TRANSPORT_LOOPBACK;
    } else if (c->host_xport) {
      *n_ranks = c->n_ranks;
      *transport = OMG_TRANSPORT_HOST;
    } else {
      *n_ranks = c->n_ranks;
      *transport = OMG_TRANSPORT_NONE;
    }
  });
}

int omg_synchronize(omg_ctx* c) {
  return guarded([&] {
    host_sync(c, c->stream);
    host_sync(c, c->stream2);
  });
}

void* omg_stream(omg_ctx* c) { return (void*)c->stream; }

int omg_set_refinement_bnd(omg_ctx* c, int iv, int nb, omg_rb_fn fn, void* user) {
  return guarded([&] {
    if (iv < 1 || iv > kMaxVars || nb < 1 || nb > 6) throw OmgError("omg_set_refinement_bnd: bad iv/nb");
    if (c->rb_fn[iv - 1][nb - 1] == (void*)fn && c->rb_user[iv - 1][nb - 1] == user) return;
    if (!c->host_only) HIPCHK(hipStreamSynchronize(c->stream));   // (staging buffers in use)
    c->rb_fn[iv - 1][nb - 1] = (void*)fn;
    c->rb_user[iv - 1][nb - 1] = fn ? user : nullptr;
    rbh_build(c);
  });
}

int omg_host_sync_count(omg_ctx* c, long long* n) {
  return guarded([&] { *n = c->n_host_syncs; });
}

int omg_comm_stream_priority(omg_ctx* c, int* priority) {
  return guarded([&] { *priority = c->comm_priority; });
}

int omg_set_profiling(omg_ctx* c, int on) {
  return guarded([&] {
    resolve_stats(c);
    c->profiling = on != 0;
  });
}

int omg_kernel_stats(omg_ctx* c, const char* name, long long* launches, double* total_ms, double* cells) {
  return guarded([&] {
    resolve_stats(c);
    auto it = c->stats.find(name);
    if (it == c->stats.end()) {
      *launches = 0;
      *total_ms = 0;
      *cells = 0;
      return;
    }
    *launches = it->second.launches;
    *total_ms = it->second.ms;
    *cells = it->second.cells;
  });
}

int omg_reset_stats(omg_ctx* c) {
  return guarded([&] {
    resolve_stats(c);
    c->stats.clear();
  });
}

}  // extern "C"
