// omg_devio.cpp — device I/O: omg_put_dense / omg_get_dense (windows of a
// level's cell grid, kernels in omg_dense.hip), omg_get_dense_grad (the same
// windows of a gradient, omg_dense_grad.hip), omg_put_boxes / omg_get_boxes
// (block lists, omg_boxes.hip), omg_get_boxes_grad (the same lists of a
// gradient, omg_boxes_grad.hip), omg_put_boxes_div (the same lists from a
// divergence, omg_boxes_div.hip) and omg_get_boxes_flux (the gradient,
// weighted and optionally added, omg_boxes_flux.hip): the caller's device
// memory, in the order of the caller's stream, by cached records.  What the
// entries share stands first.
#include <algorithm>

#include "omg_host.h"

namespace omg {

// from pinned memory, in stream order ahead of the kernels that read the
// records: no host wait (who rewrites records in use waits first: take_slot)
template <typename T>
void RecordBuf<T>::upload(omg_ctx* c, const std::vector<T>& recs) {
  using host::OmgError;   // (HIPCHK)
  if (recs.size() > cap) {
    release();
    HIPCHK(hipHostMalloc((void**)&h, sizeof(T) * recs.size()));
    HIPCHK(hipMalloc(&d, sizeof(T) * recs.size()));
    cap = recs.size();
  }
  std::copy(recs.begin(), recs.end(), h);
  HIPCHK(hipMemcpyAsync(d, h, sizeof(T) * recs.size(), hipMemcpyHostToDevice, c->stream));
}

namespace host {

constexpr long long kDenseMax = 1LL << 40;   // bound on |lo|, n, the strides and box_off (no overflow below)

// how an entry reports a bad argument: "<entry>: <what>"
struct Fail {
  const char* who;
  [[noreturn]] void operator()(const std::string& what) const { throw OmgError(std::string(who) + ": " + what); }
};

[[noreturn]] static void refuse_replicated_put(int lvl, const Fail& fail) {
  fail("level " + std::to_string(lvl) + " is replicated on every rank: use omg_upload_level");
}

// The cache slot of a key, the most recently used from now on.  hit: the slot
// that holds it, or null: then a new one while there are fewer than `bound`,
// else the oldest makes room (its records may still be on their way to the
// device or being read there: the only host wait of these entries), and the
// caller rebuilds the slot completely.
template <typename Plan>
static Plan& take_slot(omg_ctx* c, std::vector<Plan>& plans, int bound, Plan* hit) {
  if (!hit) {
    if ((int)plans.size() < bound) plans.emplace_back();
    hit = &*std::min_element(plans.begin(), plans.end(), [](const Plan& a, const Plan& b) { return a.age < b.age; });
    if (hit->buf.d) host_sync(c, c->stream);
  }
  hit->age = ++c->dense_age;
  return *hit;
}

// `dev` must be device memory of the context's GPU, its elements first .. last
// (doubles from dev; `what` in the messages) inside its allocation
static void check_device_range(omg_ctx* c, const double* dev, long long first, long long last, const char* what,
                               const Fail& fail) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, dev) != hipSuccess) {
    (void)hipGetLastError();
    fail("the pointer is not device memory");
  }
  if (at.type != hipMemoryTypeDevice) fail("the pointer is not device memory");
  if (at.device != c->device) fail("the pointer belongs to another GPU than the context's");
  hipDeviceptr_t base = nullptr;
  size_t bytes = 0;
  if (hipMemGetAddressRange(&base, &bytes, (hipDeviceptr_t)dev) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  // (in doubles from the allocation's base: |offsets| <= 20 * 2^40 for blocks, < 2^60 + 2^41 for a window)
  const long long d0 = (long long)(((const char*)dev - (const char*)base) / 8);
  const long long rem = ((const char*)dev - (const char*)base) % 8;
  if (d0 + first < 0) fail(std::string(what) + " starts before the pointer's allocation");
  if ((unsigned long long)(d0 + last + 1) * 8 + (unsigned long long)rem > bytes)
    fail(std::string(what) + " reaches past the end of the pointer's allocation");
}

// The caller's stream around a call's kernels on the context stream: they
// start after what the caller queued, what it queues next starts after them.
static void stream_after(hipEvent_t ev, hipStream_t first, hipStream_t then) {
  if (first == then) return;
  HIPCHK(hipEventRecord(ev, first));
  HIPCHK(hipStreamWaitEvent(then, ev, 0));
}
static void join_in(omg_ctx* c, void* user) { stream_after(c->ev_dense_in, (hipStream_t)user, c->stream); }
static void join_out(omg_ctx* c, void* user) { stream_after(c->ev_dense_out, c->stream, (hipStream_t)user); }

// A get's entry and its fill of the levels l0 .. l1, before any early return
// (the fill is collective).  A fill of another variable than phi writes its
// ghosts, as omg_fill_ghost_cells; phi's is skipped where it stands, a
// decision every rank makes alike.
static void enter_get(omg_ctx* c, int iv, bool fill, int l0, int l1) {
  enter(c, fill && iv != 1);
  if (!fill) return;
  for (int l = l0; l <= l1; l++) {
    const Level* L = level_ptr(c, l);
    if (iv != 1 || !L || !L->phi_gc_ok) fill_gc_lvl(c, l, iv);
  }
}

// --- dense windows
// The clip records of a window, from the level's cache or built now.  aligned:
// the window's base is 16-B aligned; generic: the per-cell kernel for every
// box; own_only: the host's own partition of a replicated level.
static DensePlan& dense_plan(omg_ctx* c, Level& L, const long long* lo, const long long* n, const long long* stride,
                             bool aligned, bool generic, bool own_only) {
  DensePlan* hit = nullptr;
  for (auto& Q : L.dense)
    if (std::equal(lo, lo + 3, Q.lo) && std::equal(n, n + 3, Q.n) && std::equal(stride, stride + 3, Q.stride) &&
        Q.aligned == aligned && Q.generic == generic && Q.own_only == own_only)
      hit = &Q;
  DensePlan& P = take_slot(c, L.dense, kDensePlans, hit);
  if (hit) return P;
  std::copy(lo, lo + 3, P.lo);
  std::copy(n, n + 3, P.n);
  std::copy(stride, stride + 3, P.stride);
  P.aligned = aligned;
  P.generic = generic;
  P.own_only = own_only;
  P.n_cells = 0;
  std::vector<DenseClip> row, gen;
  const long long nc = L.nc;
  const bool row_ok = !generic && aligned && dense_row_nc(L.nc) && stride[1] % 2 == 0 && stride[2] % 2 == 0;
  auto clip = [&](int b) {
    DenseClip r{};
    r.box = b;
    int* lohi[3][2] = {{&r.i0, &r.i1}, {&r.j0, &r.j1}, {&r.k0, &r.k1}};
    long long cells = 1;
    for (int d = 0; d < 3; d++) {
      const long long g0 = ((long long)c->ix[(size_t)(L.ids[b] - 1) * 3 + d] - 1) * nc;   // global index of local cell 1
      const long long a = std::max(g0, lo[d]), e = std::min(g0 + nc, lo[d] + n[d]);
      if (a >= e) return;
      *lohi[d][0] = (int)(a - g0) + 1;
      *lohi[d][1] = (int)(e - g0);
      r.off += (a - lo[d]) * stride[d];
      cells *= e - a;
    }
    P.n_cells += cells;
    (row_ok && r.i0 == 1 && r.i1 == L.nc && r.off % 2 == 0 ? row : gen).push_back(r);
  };
  if (own_only)
    for (int b : L.host_local) clip(b);
  else
    for (int b = 0; b < L.n; b++) clip(b);
  P.n_row = (int)row.size();
  P.n_gen = (int)gen.size();
  row.insert(row.end(), gen.begin(), gen.end());
  if (!c->host_only && !row.empty()) P.buf.upload(c, row);
  return P;
}

// The argument checks the dense entries share (before anything is launched):
// level, variable and window; returns whether the window is empty.
static bool dense_check_window(omg_ctx* c, const Level* L, int iv, const long long* lo, const long long* n,
                               const long long* stride, const Fail& fail) {
  if (!L) fail("no such level");
  if (iv < 1 || iv > c->n_vars) fail("bad variable index");
  if (!lo || !n || !stride) fail("lo, n and stride are required");
  for (int d = 0; d < 3; d++) {
    if (n[d] < 0) fail("negative extent");
    if (n[d] > kDenseMax || lo[d] > kDenseMax || lo[d] < -kDenseMax || stride[d] > kDenseMax)
      fail("window out of range");
  }
  if (stride[0] != 1) fail("stride[0] must be 1");
  const bool empty = n[0] == 0 || n[1] == 0 || n[2] == 0;
  if (!empty) {
    if (stride[1] < n[0]) fail("stride[1] < n[0]");
    if (stride[2] / n[1] < stride[1]) fail("stride[2] < stride[1]*n[1]");
    if (stride[2] > LLONG_MAX / 8 / n[2]) fail("window out of range");
  }
  return empty;
}

// doubles from a non-empty window's first element to one past its last
static long long dense_extent(const long long* n, const long long* stride) {
  return (n[2] - 1) * stride[2] + (n[1] - 1) * stride[1] + n[0];
}

// The plan of a checked window and its count into *n_cells.  Null where there
// is nothing to launch: a plan-only context, an empty window, no cell of the
// window in a box of this rank.
static DensePlan* dense_claim(omg_ctx* c, Level& L, const long long* lo, const long long* n, const long long* stride,
                              bool empty, bool aligned, long long* n_cells, const Fail& fail) {
  if (n_cells) *n_cells = 0;
  if (empty || (!c->host_only && !L.n)) return nullptr;
  DensePlan& P = dense_plan(c, L, lo, n, stride, aligned, env_flag("OMG_DENSE_GENERIC"), L.replicated);
  if (n_cells) *n_cells = P.n_cells;
  if (c->host_only || !P.n_cells) return nullptr;
  if ((long long)P.n_gen * 16 > INT_MAX) fail("too many boxes for one launch");
  return &P;
}

void dense_io(omg_ctx* c, int lvl, int iv, double* dev, const long long* lo, const long long* n,
              const long long* stride, void* stream, long long* n_cells, bool put) {
  const Fail fail{put ? "omg_put_dense" : "omg_get_dense"};
  Level* L = level_ptr(c, lvl);
  const bool empty = dense_check_window(c, L, iv, lo, n, stride, fail);
  if (!empty && !dev) fail("NULL pointer with a non-empty window");
  if (put && L->replicated) refuse_replicated_put(lvl, fail);
  auto claim = [&] { return dense_claim(c, *L, lo, n, stride, empty, ((uintptr_t)dev & 15) == 0, n_cells, fail); };
  if (c->host_only) return (void)claim();
  if (!empty) check_device_range(c, dev, 0, dense_extent(n, stride) - 1, "the window", fail);
  if (put) {
    enter(c);
    // (before the early return, as omg_upload_level)
    if (iv == 1) phi_dirty(c, lvl);
  } else {
    enter_get(c, iv, false, lvl, lvl);
  }
  DensePlan* P = claim();
  if (!P) return;
  join_in(c, stream);
  {
    Prof p(c, put ? "dense_put" : "dense_get", (double)P->n_cells, lvl);
    const LevelView V = L->view();
    if (P->n_row) {
      Prof pr(c, put ? "dense_put_row" : "dense_get_row", (double)P->n_row * L->nc * L->nc * L->nc, lvl);
      launch_dense_row(V, iv, P->buf.d, P->n_row, dev, stride[1], stride[2], put, c->stream);
    }
    launch_dense_cell(V, iv, P->buf.d + P->n_row, P->n_gen, dev, stride[1], stride[2], put, c->stream);
    HIPCHK(hipGetLastError());
  }
  join_out(c, stream);
}

// omg_get_dense_grad: omg_get_dense's window, clip records and stream
// ordering; up to three component windows.
void dense_grad(omg_ctx* c, int lvl, int iv, double* const* dev, const long long* lo, const long long* n,
                const long long* stride, double scale, bool fill, void* stream, long long* n_cells) {
  const Fail fail{"omg_get_dense_grad"};
  Level* L = level_ptr(c, lvl);
  const bool empty = dense_check_window(c, L, iv, lo, n, stride, fail);
  if (!dev) fail("the array of component pointers is required");
  bool aligned = true, any = false;
  for (int d = 0; d < 3; d++)
    if (dev[d]) {
      any = true;
      aligned = aligned && ((uintptr_t)dev[d] & 15) == 0;
    }
  if (!empty) {
    if (!any) fail("NULL pointers for all three components with a non-empty window");
    const uintptr_t bytes = (uintptr_t)dense_extent(n, stride) * sizeof(double);
    for (int d = 0; d < 3; d++)
      for (int e = d + 1; e < 3; e++)
        if (dev[d] && dev[e] && (uintptr_t)dev[d] < (uintptr_t)dev[e] + bytes &&
            (uintptr_t)dev[e] < (uintptr_t)dev[d] + bytes)
          fail("the windows of components " + std::to_string(d) + " and " + std::to_string(e) + " overlap");
  }
  auto claim = [&] { return dense_claim(c, *L, lo, n, stride, empty, aligned, n_cells, fail); };
  if (c->host_only) return (void)claim();
  if (!empty)
    for (int d = 0; d < 3; d++)
      if (dev[d]) check_device_range(c, dev[d], 0, dense_extent(n, stride) - 1, "the window", fail);
  enter_get(c, iv, fill, lvl, lvl);
  DensePlan* P = claim();
  if (!P) return;
  DenseGrad G;
  for (int d = 0; d < 3; d++) {
    G.out[d] = dev[d];
    G.f[d] = (0.5 * scale) / L->dr[d];
  }
  join_in(c, stream);
  {
    Prof p(c, "dense_grad", (double)P->n_cells, lvl);
    const LevelView V = L->view();
    if (P->n_row) {
      Prof pr(c, "dense_grad_row", (double)P->n_row * L->nc * L->nc * L->nc, lvl);
      launch_dense_grad_tile(V, iv, P->buf.d, P->n_row, G, stride[1], stride[2], c->stream);
    }
    launch_dense_grad_cell(V, iv, P->buf.d + P->n_row, P->n_gen, G, stride[1], stride[2], c->stream);
    HIPCHK(hipGetLastError());
  }
  join_out(c, stream);
}

// --- block lists
// What tools/box_io_bench.py measured, in place of switches:
// blocks that are not 16-B aligned take the tile kernel's 8-B variant, except
// a get with ghosts, whose interior rows the shifted variant covers with
// whole pairs (OMG_BOXES_ODD=8 / 16 overrides, for A/B timing).  The per-cell kernel
// takes a level with fewer listed boxes than kBoxesTileMin (one workgroup per
// box leaves the GPU short of work: it won at 512 and 960 boxes, the tile
// kernel from 1728 on), and a get of interiors into rows with a gap between
// them (stride[1] > nc) of more than kBoxesGapGetCells cells (it won at 8000
// boxes of 16^3 and more, the tile kernel at 4096, whose pool the Infinity
// Cache still holds).  OMG_BOXES_TILE=1: the tile kernel wherever it can serve.
constexpr int kBoxesTileMin = 1536;
constexpr long long kBoxesGapGetCells = 6144LL * 4096;

static bool boxes_odd8(bool put, int ghost) {
  const char* v = getenv("OMG_BOXES_ODD");
  if (v && !std::strcmp(v, "8")) return true;
  if (v && !std::strcmp(v, "16")) return false;
  return put || !ghost;
}

// The records of a list: every id checked (range, owner, replicated level,
// listed once), grouped by level.  Touches nothing of the context.
static void boxes_build(omg_ctx* c, BoxPlan& P, int n_boxes, const int* ids, const long long* box_off, bool put,
                        const Fail& fail) {
  P.ids.assign(ids, ids + n_boxes);
  P.off.assign(box_off, box_off + n_boxes);
  P.recs.resize(n_boxes);
  std::map<int, int> per_lvl;   // level -> boxes listed
  std::vector<int> sorted(ids, ids + n_boxes);
  std::sort(sorted.begin(), sorted.end());
  for (int q = 0; q < n_boxes; q++) {
    const int id = sorted[q];
    if (id < 1 || id > c->n_boxes) fail("box id " + std::to_string(id) + " is out of range");
    if (q && sorted[q - 1] == id) fail("box id " + std::to_string(id) + " is listed twice");
  }
  for (int q = 0; q < n_boxes; q++) {
    const int id = ids[q], lvl = c->lvl[id - 1];
    const Level* L = level_ptr(c, lvl);
    if (!L || c->local_index[id] < 0) fail("box id " + std::to_string(id) + " is not owned by this rank");
    if (L->replicated) {
      if (put) refuse_replicated_put(lvl, fail);
      if (c->rank_of[id - 1] != c->rank)
        fail("box id " + std::to_string(id) + " on the replicated level " + std::to_string(lvl) +
             " is not one of this rank's own boxes");
      P.any_replicated = true;
    }
    if (box_off[q] > kDenseMax || box_off[q] < -kDenseMax) fail("box_off out of range");
    per_lvl[lvl]++;
  }
  int first = 0;
  for (auto& kv : per_lvl) {
    P.groups.push_back(BoxGroup{kv.first, first, 0, false});
    first += kv.second;
    P.nc_max = std::max(P.nc_max, level_ptr(c, kv.first)->nc);
  }
  bool have_ext = false;
  for (int q = 0; q < n_boxes; q++) {
    const int id = ids[q], lvl = c->lvl[id - 1];
    const Level* L = level_ptr(c, lvl);
    BoxGroup& G = *std::find_if(P.groups.begin(), P.groups.end(), [&](const BoxGroup& g) { return g.lvl == lvl; });
    P.recs[G.first + G.n++] = BoxRec{c->local_index[id], lvl, box_off[q]};
    if (!P.aligned || (box_off[q] | P.stride[1] | P.stride[2]) & 1) G.odd = true;
    const long long nc = L->nc;
    // (a face-centred gradient: nc + 1 faces along the component's direction)
    P.n_cells += P.centering == 1 ? (nc + 1) * nc * nc : nc * nc * nc + (long long)P.ghost * 6 * nc * nc;
    // first and last touched element: (1,1,0) and (nc,nc,nc+1) with ghosts
    // (a face-centred component starts one stride[d] lower: boxes_grad)
    const long long lo = box_off[q] - (P.ghost ? P.stride[2] : 0);
    const long long hi = box_off[q] + (nc - 1) + (nc - 1) * P.stride[1] + (nc - 1 + P.ghost) * P.stride[2];
    P.lo_ext = have_ext ? std::min(P.lo_ext, lo) : lo;
    P.hi_ext = have_ext ? std::max(P.hi_ext, hi) : hi;
    have_ext = true;
  }
}

// The checks of a list's arguments that the block entries share.
static void boxes_check_list(int n_boxes, const int* ids, const long long* box_off, const long long* stride,
                             const Fail& fail) {
  if (n_boxes < 0) fail("negative n_boxes");
  if (!stride) fail("stride is required");
  if (stride[0] != 1) fail("stride[0] must be 1");
  if (stride[1] < 1 || stride[2] < 1 || stride[1] > kDenseMax || stride[2] > kDenseMax) fail("stride out of range");
  if (n_boxes > 0 && (!ids || !box_off)) fail("NULL ids or box_off with n_boxes > 0");
}

// The cached records of a list, or null (a cached list was checked when it
// was built).  centering: kBoxCopy for the copies, omg_get_boxes_grad's, or
// kBoxDiv + omg_put_boxes_div's.
static BoxPlan* boxes_cached(omg_ctx* c, int n_boxes, const int* ids, const long long* box_off,
                             const long long* stride, int ghost, int centering, bool aligned) {
  BoxPlan* P = nullptr;
  for (auto& Q : c->box_plans)
    if ((int)Q.ids.size() == n_boxes && Q.ghost == ghost && Q.centering == centering &&
        std::equal(stride, stride + 3, Q.stride) && Q.aligned == aligned &&
        std::equal(ids, ids + n_boxes, Q.ids.begin()) && std::equal(box_off, box_off + n_boxes, Q.off.begin()))
      P = &Q;
  return P;
}

// The cache slot of a call's list, the most recently used from now on: the
// cached one, or `fresh` in a new or the oldest slot with its records on
// their way to the device.
static BoxPlan& boxes_claim(omg_ctx* c, BoxPlan* cached, BoxPlan& fresh) {
  BoxPlan& S = take_slot(c, c->box_plans, kBoxPlans, cached);
  if (!cached) {
    // (the slot keeps its buffers and its place in the order of use)
    fresh.buf = S.buf;
    fresh.age = S.age;
    S = std::move(fresh);
    S.buf.upload(c, S.recs);
  }
  return S;
}

void box_io(omg_ctx* c, int iv, int n_boxes, const int* ids, double* dev, const long long* box_off,
            const long long* stride, int ghost, bool fill, void* stream, long long* n_cells, bool put) {
  const Fail fail{put ? "omg_put_boxes" : "omg_get_boxes"};
  if (iv < 1 || iv > c->n_vars) fail("bad variable index");
  if (ghost != 0 && ghost != 1) fail("ghost must be 0 or 1");
  boxes_check_list(n_boxes, ids, box_off, stride, fail);
  if (n_boxes > 0 && !dev) fail("NULL pointer with n_boxes > 0");
  if (c->levels.empty()) fail("no tree (omg_tree_setup)");
  // (the switches choose the kernel at launch: the records do not depend on them)
  const bool generic = env_flag("OMG_BOXES_GENERIC"), force_tile = env_flag("OMG_BOXES_TILE");
  const bool odd8 = boxes_odd8(put, ghost);
  const bool aligned = ((uintptr_t)dev & 15) == 0;
  // a cached list was checked when it was built
  BoxPlan* P = boxes_cached(c, n_boxes, ids, box_off, stride, ghost, kBoxCopy, aligned);
  BoxPlan fresh;
  if (P) {
    for (int q = 0; q < n_boxes && put && P->any_replicated; q++)   // (refused again: a put)
      if (level_ptr(c, c->lvl[ids[q] - 1])->replicated) refuse_replicated_put(c->lvl[ids[q] - 1], fail);
  } else {
    fresh.ghost = ghost;
    std::copy(stride, stride + 3, fresh.stride);
    fresh.aligned = aligned;
    boxes_build(c, fresh, n_boxes, ids, box_off, put, fail);
  }
  const BoxPlan& R = P ? *P : fresh;
  if (n_boxes > 0) {
    const long long m = R.nc_max + 2 * ghost;
    if (stride[1] < m) fail("stride[1] < nc + 2*ghost");
    if (stride[2] / m < stride[1]) fail("stride[2] < stride[1]*(nc + 2*ghost)");
  }
  if (c->host_only) {
    if (n_cells) *n_cells = R.n_cells;
    return;
  }
  if (n_boxes > 0) {
    check_device_range(c, dev, R.lo_ext, R.hi_ext, "a block", fail);
    for (const BoxGroup& G : R.groups)
      if ((long long)G.n * 16 > INT_MAX) fail("too many boxes for one launch");
  }
  // --- nothing of the state was touched up to here
  if (put) {
    enter(c);
    // (every level: a rank cannot know which levels its peers list, and the
    // stand-alone fill decision must fall alike on every rank)
    if (iv == 1) phi_dirty_all(c);
    if (iv == 2 && ghost) rhs_ghosts_written_all(c);
  } else {
    enter_get(c, iv, fill, c->lowest, c->highest);
  }
  if (n_cells) *n_cells = R.n_cells;
  if (n_boxes == 0) return;
  BoxPlan& S = boxes_claim(c, P, fresh);
  join_in(c, stream);
  {
    Prof p(c, put ? "boxes_put" : "boxes_get", (double)S.n_cells);
    for (const BoxGroup& G : S.groups) {
      const Level* L = level_ptr(c, G.lvl);
      const LevelView V = L->view();
      const double cells = (double)G.n * ((double)L->nc * L->nc * L->nc + ghost * 6.0 * L->nc * L->nc);
      const bool tile = !generic && boxes_tile_nc(L->nc) &&
                        (force_tile || (G.n >= kBoxesTileMin && (put || ghost || stride[1] == L->nc ||
                                                                 (long long)G.n * L->nc * L->nc * L->nc <=
                                                                     kBoxesGapGetCells)));
      if (tile) {
        Prof pr(c, put ? "boxes_put_tile" : "boxes_get_tile", cells, G.lvl);
        launch_boxes_tile(V, iv, S.buf.d + G.first, G.n, dev, stride[1], stride[2], ghost, put, odd8 && G.odd,
                          c->stream);
      } else {
        launch_boxes_cell(V, iv, S.buf.d + G.first, G.n, dev, stride[1], stride[2], ghost, put, c->stream);
      }
    }
    HIPCHK(hipGetLastError());
  }
  join_out(c, stream);
}

// What tools/box_grad_bench.py measured for this entry's kernels (DESIGN §19,
// 16^3 boxes, listed boxes of one level): one workgroup per box leaves the
// GPU short of work on short lists here too.  Face centring: the per-cell
// kernel won at 256 boxes, the tile kernel from 512 on.  Cell centring: the
// per-cell kernel won up to 512 boxes and tied at 1024, the tile kernel won
// from 1536 on into whole rows (stride[1] == nc); into rows with a gap
// between them it won at 1536 and 2048 boxes only, the per-cell kernel from
// 3072 on, where both write partial lines.
constexpr int kBoxesGradTileMinFace = 512;
constexpr int kBoxesGradTileMinCell = 1536;
constexpr long long kBoxesGradGapCells = 2048LL * 4096;

// omg_get_boxes_grad: omg_get_boxes's list, records, cache and stream
// ordering; up to three component pools that share box_off and the strides.
void boxes_grad(omg_ctx* c, int iv, int n_boxes, const int* ids, double* const* dev, const long long* box_off,
                const long long* stride, double scale, int centering, bool fill, void* stream, long long* n_cells) {
  const Fail fail{"omg_get_boxes_grad"};
  if (iv < 1 || iv > c->n_vars) fail("bad variable index");
  if (centering != 0 && centering != 1) fail("centering must be 0 (cells) or 1 (faces)");
  boxes_check_list(n_boxes, ids, box_off, stride, fail);
  if (!dev) fail("the array of component pointers is required");
  bool aligned = true, any = false;
  for (int d = 0; d < 3; d++)
    if (dev[d]) {
      any = true;
      aligned = aligned && ((uintptr_t)dev[d] & 15) == 0;
      for (int e = 0; e < d; e++)
        if (dev[e] == dev[d])
          fail("components " + std::to_string(e) + " and " + std::to_string(d) + " share one pointer");
    }
  if (n_boxes > 0 && !any) fail("NULL pointers for all three components with n_boxes > 0");
  if (c->levels.empty()) fail("no tree (omg_tree_setup)");
  const bool generic = env_flag("OMG_BOXES_GENERIC"), force_tile = env_flag("OMG_BOXES_TILE");
  BoxPlan* P = boxes_cached(c, n_boxes, ids, box_off, stride, 0, centering, aligned);
  BoxPlan fresh;
  if (!P) {
    fresh.centering = centering;
    std::copy(stride, stride + 3, fresh.stride);
    fresh.aligned = aligned;
    boxes_build(c, fresh, n_boxes, ids, box_off, false, fail);
  }
  const BoxPlan& R = P ? *P : fresh;
  if (n_boxes > 0) {
    const long long m = R.nc_max + centering;
    if (stride[1] < m) fail(centering ? "stride[1] < nc + 1" : "stride[1] < nc");
    if (stride[2] / m < stride[1]) fail(centering ? "stride[2] < stride[1]*(nc + 1)" : "stride[2] < stride[1]*nc");
  }
  if (c->host_only) {
    if (n_cells) *n_cells = R.n_cells;
    return;
  }
  if (n_boxes > 0) {
    // (a face-centred component starts one element, row or plane below its boxes' interiors)
    for (int d = 0; d < 3; d++)
      if (dev[d]) check_device_range(c, dev[d], R.lo_ext - (centering ? stride[d] : 0), R.hi_ext, "a block", fail);
    for (const BoxGroup& G : R.groups)
      if ((long long)G.n * 16 > INT_MAX) fail("too many boxes for one launch");
  }
  // --- nothing of the state was touched up to here
  enter_get(c, iv, fill, c->lowest, c->highest);
  if (n_cells) *n_cells = R.n_cells;
  if (n_boxes == 0) return;
  BoxPlan& S = boxes_claim(c, P, fresh);
  join_in(c, stream);
  {
    Prof p(c, "boxes_grad", (double)S.n_cells);
    for (const BoxGroup& G : S.groups) {
      const Level* L = level_ptr(c, G.lvl);
      const LevelView V = L->view();
      DenseGrad A;
      for (int d = 0; d < 3; d++) {
        A.out[d] = dev[d];
        A.f[d] = (centering ? scale : 0.5 * scale) / L->dr[d];
      }
      const bool measured =
          centering ? G.n >= kBoxesGradTileMinFace
                    : G.n >= kBoxesGradTileMinCell &&
                          (stride[1] == L->nc || (long long)G.n * L->nc * L->nc * L->nc <= kBoxesGradGapCells);
      const bool tile = !generic && boxes_tile_nc(L->nc) && (force_tile || measured);
      if (tile) {
        Prof pr(c, "boxes_grad_tile", (double)G.n * (L->nc + centering) * L->nc * L->nc, G.lvl);
        launch_boxes_grad_tile(V, iv, S.buf.d + G.first, G.n, A, stride[1], stride[2], centering != 0, G.odd,
                               c->stream);
      } else {
        launch_boxes_grad_cell(V, iv, S.buf.d + G.first, G.n, A, stride[1], stride[2], centering != 0, c->stream);
      }
    }
    HIPCHK(hipGetLastError());
  }
  join_out(c, stream);
}

// What tools/box_div_bench.py measured for this entry's kernels (DESIGN §20,
// 16^3 boxes, 128 .. 8000 listed boxes of one level, both centrings, pools
// with one and two ghost layers): the per-cell kernel won at every length up
// to 2048 boxes (2.2x at 128, 1.1x at 1536); from 4096 on both run at the
// memory's rate, the per-cell kernel 5 % ahead with two ghost layers, within
// 4 % either way between runs with one.  By §14's rule the tile kernel stays
// nowhere: it is routed around and runs under OMG_BOXES_TILE=1 only.
constexpr int kBoxesDivTileMinCell = INT_MAX;
constexpr int kBoxesDivTileMinFace = INT_MAX;

// omg_put_boxes_div: omg_put_boxes's state with ghost == 0 and
// omg_get_boxes_grad's list, records, cache and stream ordering; up to three
// read-only component pools that share box_off and the strides.
void boxes_div(omg_ctx* c, int iv, int n_boxes, const int* ids, const double* const* dev, const long long* box_off,
               const long long* stride, double scale, int centering, void* stream, long long* n_cells) {
  const Fail fail{"omg_put_boxes_div"};
  if (iv < 1 || iv > c->n_vars) fail("bad variable index");
  if (centering != 0 && centering != 1) fail("centering must be 0 (cells) or 1 (faces)");
  boxes_check_list(n_boxes, ids, box_off, stride, fail);
  if (!dev) fail("the array of component pointers is required");
  bool aligned = true, any = false;
  for (int d = 0; d < 3; d++)
    if (dev[d]) {
      any = true;
      aligned = aligned && ((uintptr_t)dev[d] & 15) == 0;
    }
  if (n_boxes > 0 && !any) fail("NULL pointers for all three components with n_boxes > 0");
  if (c->levels.empty()) fail("no tree (omg_tree_setup)");
  const bool generic = env_flag("OMG_BOXES_GENERIC"), force_tile = env_flag("OMG_BOXES_TILE");
  BoxPlan* P = boxes_cached(c, n_boxes, ids, box_off, stride, 0, kBoxDiv + centering, aligned);
  BoxPlan fresh;
  if (P) {
    for (int q = 0; q < n_boxes && P->any_replicated; q++)   // (refused again: a put)
      if (level_ptr(c, c->lvl[ids[q] - 1])->replicated) refuse_replicated_put(c->lvl[ids[q] - 1], fail);
  } else {
    fresh.centering = kBoxDiv + centering;
    std::copy(stride, stride + 3, fresh.stride);
    fresh.aligned = aligned;
    boxes_build(c, fresh, n_boxes, ids, box_off, true, fail);
  }
  const BoxPlan& R = P ? *P : fresh;
  if (n_boxes > 0) {
    // (the layer 0 along each direction, and the layer nc+1 of cell centring)
    const long long m = R.nc_max + (centering ? 1 : 2);
    if (stride[1] < m) fail(centering ? "stride[1] < nc + 1" : "stride[1] < nc + 2");
    if (stride[2] / m < stride[1]) fail(centering ? "stride[2] < stride[1]*(nc + 1)" : "stride[2] < stride[1]*(nc + 2)");
  }
  if (c->host_only) {
    if (n_cells) *n_cells = R.n_cells;
    return;
  }
  if (n_boxes > 0) {
    // (component d reaches one element, row or plane below its boxes'
    // interiors, and with cell centring as far above them)
    for (int d = 0; d < 3; d++)
      if (dev[d])
        check_device_range(c, dev[d], R.lo_ext - stride[d], R.hi_ext + (centering ? 0 : stride[d]), "a block", fail);
    for (const BoxGroup& G : R.groups)
      if ((long long)G.n * 16 > INT_MAX) fail("too many boxes for one launch");
  }
  // --- nothing of the state was touched up to here
  enter(c);
  // (every level, as box_io's put)
  if (iv == 1) phi_dirty_all(c);
  if (n_cells) *n_cells = R.n_cells;
  if (n_boxes == 0) return;
  BoxPlan& S = boxes_claim(c, P, fresh);
  join_in(c, stream);
  {
    Prof p(c, "boxes_div", (double)S.n_cells);
    for (const BoxGroup& G : S.groups) {
      const Level* L = level_ptr(c, G.lvl);
      const LevelView V = L->view();
      BoxDiv A;
      for (int d = 0; d < 3; d++) {
        A.in[d] = dev[d];
        A.f[d] = (centering ? scale : 0.5 * scale) / L->dr[d];
      }
      const bool measured = G.n >= (centering ? kBoxesDivTileMinFace : kBoxesDivTileMinCell);
      const bool tile = !generic && boxes_tile_nc(L->nc) && (force_tile || measured);
      if (tile) {
        Prof pr(c, "boxes_div_tile", (double)G.n * L->nc * L->nc * L->nc, G.lvl);
        launch_boxes_div_tile(V, iv, S.buf.d + G.first, G.n, A, stride[1], stride[2], centering != 0, G.odd,
                              c->stream);
      } else {
        launch_boxes_div_cell(V, iv, S.buf.d + G.first, G.n, A, stride[1], stride[2], centering != 0, c->stream);
      }
    }
    HIPCHK(hipGetLastError());
  }
  join_out(c, stream);
}

// What tools/box_flux_bench.py measured for this entry's kernels (DESIGN §21,
// profiles/r13/boxes_flux_bench.jsonl: 16^3 boxes, 128 .. 8000 listed boxes
// of one level, face centring, no, one and three coefficients, writing and
// accumulating, pools with one and two ghost layers).  The constants started
// at "per-cell everywhere" (the sweep_* records) and moved only where the tile
// kernel won by more than the rounds' spread (§14's rule).  Face centring: the
// per-cell kernel won at 128 and 256 boxes in all twelve cases (1.1x to 1.6x);
// the tile kernel won from 512 boxes on in every case but one tie (no
// coefficient, writing, one ghost layer, 512 boxes: 0.0325 against 0.0346 ms,
// inside the spread), 1.1x to 1.3x at 512, 1.2x to 1.7x from 1024 to 8000.
// Cell centring was not timed: it stays with the per-cell kernel, and the
// tile kernel runs there under OMG_BOXES_TILE=1 only.
constexpr int kBoxesFluxTileMinCell = INT_MAX;
constexpr int kBoxesFluxTileMinFace = 512;

// omg_get_boxes_flux: omg_get_boxes_grad's checks, list, records, cache key
// and stream ordering; a coefficient variable per component, read as a get
// without a fill reads it, and an optional accumulate.
void boxes_flux(omg_ctx* c, int iv, const int* iv_coef, int n_boxes, const int* ids, double* const* dev,
                const long long* box_off, const long long* stride, double scale, int centering, bool accumulate,
                bool fill, void* stream, long long* n_cells) {
  const Fail fail{"omg_get_boxes_flux"};
  if (iv < 1 || iv > c->n_vars) fail("bad variable index");
  FluxCoef K{{0, 0, 0}};
  for (int d = 0; d < 3 && iv_coef; d++) {
    K.iv[d] = iv_coef[d];
    if (K.iv[d] < 0 || K.iv[d] > c->n_vars)
      fail("iv_coef[" + std::to_string(d) + "] = " + std::to_string(K.iv[d]) + " is not 0 or a variable 1.." +
           std::to_string(c->n_vars));
    if (K.iv[d] == iv) fail("iv_coef[" + std::to_string(d) + "] is iv itself");
  }
  if (centering != 0 && centering != 1) fail("centering must be 0 (cells) or 1 (faces)");
  boxes_check_list(n_boxes, ids, box_off, stride, fail);
  if (!dev) fail("the array of component pointers is required");
  bool aligned = true, any = false;
  for (int d = 0; d < 3; d++)
    if (dev[d]) {
      any = true;
      aligned = aligned && ((uintptr_t)dev[d] & 15) == 0;
      for (int e = 0; e < d; e++)
        if (dev[e] == dev[d])
          fail("components " + std::to_string(e) + " and " + std::to_string(d) + " share one pointer");
    }
  if (n_boxes > 0 && !any) fail("NULL pointers for all three components with n_boxes > 0");
  if (c->levels.empty()) fail("no tree (omg_tree_setup)");
  const bool generic = env_flag("OMG_BOXES_GENERIC"), force_tile = env_flag("OMG_BOXES_TILE");
  // (the gradient's key: a list either entry cached serves both)
  BoxPlan* P = boxes_cached(c, n_boxes, ids, box_off, stride, 0, centering, aligned);
  BoxPlan fresh;
  if (!P) {
    fresh.centering = centering;
    std::copy(stride, stride + 3, fresh.stride);
    fresh.aligned = aligned;
    boxes_build(c, fresh, n_boxes, ids, box_off, false, fail);
  }
  const BoxPlan& R = P ? *P : fresh;
  if (n_boxes > 0) {
    const long long m = R.nc_max + centering;
    if (stride[1] < m) fail(centering ? "stride[1] < nc + 1" : "stride[1] < nc");
    if (stride[2] / m < stride[1]) fail(centering ? "stride[2] < stride[1]*(nc + 1)" : "stride[2] < stride[1]*nc");
  }
  if (c->host_only) {
    if (n_cells) *n_cells = R.n_cells;
    return;
  }
  if (n_boxes > 0) {
    // (the gradient's range, with and without accumulate)
    for (int d = 0; d < 3; d++)
      if (dev[d]) check_device_range(c, dev[d], R.lo_ext - (centering ? stride[d] : 0), R.hi_ext, "a block", fail);
    for (const BoxGroup& G : R.groups)
      if ((long long)G.n * 16 > INT_MAX) fail("too many boxes for one launch");
  }
  // --- nothing of the state was touched up to here
  enter_get(c, iv, fill, c->lowest, c->highest);
  // (each distinct coefficient as a get without a fill: its ghosts as they stand)
  for (int d = 0; d < 3; d++)
    if (K.iv[d] && std::find(K.iv, K.iv + d, K.iv[d]) == K.iv + d) enter_get(c, K.iv[d], false, c->lowest, c->highest);
  if (n_cells) *n_cells = R.n_cells;
  if (n_boxes == 0) return;
  BoxPlan& S = boxes_claim(c, P, fresh);
  join_in(c, stream);
  {
    Prof p(c, "boxes_flux", (double)S.n_cells);
    for (const BoxGroup& G : S.groups) {
      const Level* L = level_ptr(c, G.lvl);
      const LevelView V = L->view();
      DenseGrad A;
      for (int d = 0; d < 3; d++) {
        A.out[d] = dev[d];
        A.f[d] = (centering ? scale : 0.5 * scale) / L->dr[d];
      }
      const bool measured = G.n >= (centering ? kBoxesFluxTileMinFace : kBoxesFluxTileMinCell);
      const bool tile = !generic && boxes_tile_nc(L->nc) && (force_tile || measured);
      if (tile) {
        Prof pr(c, "boxes_flux_tile", (double)G.n * (L->nc + centering) * L->nc * L->nc, G.lvl);
        launch_boxes_flux_tile(V, iv, S.buf.d + G.first, G.n, A, K, stride[1], stride[2], centering != 0, G.odd,
                               accumulate, c->stream);
      } else {
        launch_boxes_flux_cell(V, iv, S.buf.d + G.first, G.n, A, K, stride[1], stride[2], centering != 0, accumulate,
                               c->stream);
      }
    }
    HIPCHK(hipGetLastError());
  }
  join_out(c, stream);
}

}  // namespace host
}  // namespace omg
