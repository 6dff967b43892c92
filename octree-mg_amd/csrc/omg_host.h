// omg_host.h — what the host-side units of libomg.so share: error handling,
// device allocation, the tree and level helpers, the two transports' state
// and one declaration for every function called across units.  Host only: no
// .hip file includes it (the kernels' data model is omg_internal.h).
#pragma once

#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>
#include <rccl/rccl.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <climits>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/omg.h"
#include "omg_free.h"
#include "omg_kernels.h"

// ---------------------------------------------------------------------------
// In-process loopback transport.  n_ranks contexts of ONE process (one host
// thread each, typically sharing one GPU) exchange their transfer segments by
// device-to-device copies ordered with HIP events, instead of RCCL.  The plans,
// the packing/unpacking kernels, the wire order and the reductions are those
// of the RCCL path, so multi-rank parity can be checked on a single GPU.
struct omg_loop {
  struct Msg {
    const double* src;
    size_t n;
    hipEvent_t ev;
  };
  using Key = std::tuple<int, int, long long>;   // (from, to, sequence of that pair)
  int n_ranks = 0;
  std::mutex mu;
  std::condition_variable cv;
  std::map<Key, Msg> box;
  std::map<Key, hipEvent_t> acks;               // (receiver, sender, seq) -> copies done
  std::map<long long, std::vector<double>> vals;
  std::map<long long, int> n_in, n_out;
};

// m_free_space's free_bc (src/m_free_space.f90:9-24) on the device: the FFT
// grid, the kernel spectrum, the boundary planes and the gather plan of the
// FFT level's right-hand side.
struct omg_free_state {
  bool initialized = false;
  int fft_lvl = INT_MIN;
  omg::FreeGrid G{};
  double r_min[3] = {0, 0, 0};       // mg%r_min of the domain
  double* d_R = nullptr;             // real padded grid [N3][N2][N1] (density, then potential)
  double2* d_Z = nullptr;            // its D2Z spectrum [N3][N2][N1/2+1]
  double* d_karray = nullptr;        // kernel spectrum * scal, same shape, real
  double* d_planes = nullptr;        // bc_x0, bc_x1, bc_y0, bc_y1, bc_z0, bc_z1
  hipfftHandle fwd = 0, inv = 0;
  bool have_plans = false;
  // my boxes at the FFT level: local index and ix
  int n_my = 0;
  int* d_my = nullptr;
  int* d_my_ix = nullptr;
  // the other ranks' boxes (multi-rank, FFT level not replicated)
  omg::Transfer gather;
  double* d_send = nullptr;
  double* d_recv = nullptr;
  int* d_recv_ix = nullptr;
  omg::FreePlaneGeom P{};
};

namespace omg {
namespace host {

struct OmgError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define HIPCHK(x)                                                                            \
  do {                                                                                       \
    hipError_t e_ = (x);                                                                     \
    if (e_ != hipSuccess)                                                                    \
      throw OmgError(std::string(#x) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + ":" + \
                     std::to_string(__LINE__) + ")");                                        \
  } while (0)

#define NCCLCHK(x)                                                                         \
  do {                                                                                     \
    ncclResult_t r_ = (x);                                                                 \
    if (r_ != ncclSuccess) throw OmgError(std::string(#x) + ": " + ncclGetErrorString(r_)); \
  } while (0)

// Every place the host waits for a context stream goes through here, so the
// waits of a call can be counted (omg_host_sync_count: a multi-rank stand-alone
// V-cycle makes none unless max_res is requested).
inline void host_sync(omg_ctx* c, hipStream_t st) {
  c->n_host_syncs++;
  HIPCHK(hipStreamSynchronize(st));
}

// Plan-only contexts (omg_ctx_create with OMG_DEVICE_NONE) build every host
// table of omg_tree_setup but allocate nothing on a device.
extern thread_local bool g_host_only;   // (defined in omg_api.cpp)

template <typename T>
void dmalloc(T** p, size_t bytes, bool zero = false) {
  *p = nullptr;
  if (g_host_only || bytes == 0) return;
  HIPCHK(hipMalloc((void**)p, bytes));
  if (zero) HIPCHK(hipMemset(*p, 0, bytes));
}

template <typename T>
T* to_device(const std::vector<T>& v) {
  if (v.empty() || g_host_only) return nullptr;
  T* d = nullptr;
  HIPCHK(hipMalloc(&d, sizeof(T) * v.size()));
  HIPCHK(hipMemcpy(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
  return d;
}

template <typename T>
void dfree(T*& p) {
  if (p) (void)hipFree((void*)p);
  p = nullptr;
}

const int kNeighbRev[6] = {2, 1, 4, 3, 6, 5};

// an on/off switch from the environment: set and not "0" (or empty)
inline bool env_flag(const char* name) {
  const char* v = getenv(name);
  return v && *v && std::strcmp(v, "0") != 0;
}

// a signalling NaN (quiet bit clear): OMG_DEBUG's poison
inline double snan_value() {
  const unsigned long long bits = 0x7FF4000000000000ULL;
  double d;
  std::memcpy(&d, &bits, 8);
  return d;
}

inline int pack_dix(const int d[3]) { return d[0] | (d[1] << 10) | (d[2] << 20); }

// ---------------------------------------------------------------------------
// tree helpers (reference src/m_data_structures.f90)
struct Tree {
  omg_ctx* c;
  int lvl(int id) const { return c->lvl[id - 1]; }
  int parent(int id) const { return c->parent[id - 1]; }
  int child(int id, int s) const { return c->children[(id - 1) * 8 + s - 1]; }
  int nbr(int id, int nb) const { return c->neighbors[(id - 1) * 6 + nb - 1]; }
  int rank(int id) const { return c->rank_of[id - 1]; }
  // mg_get_child_offset (m_data_structures.f90:456-467)
  void child_offset(int id, int d[3]) const {
    if (lvl(id) <= c->first_normal) {
      d[0] = d[1] = d[2] = 0;
    } else {
      for (int q = 0; q < 3; q++) d[q] = ((c->ix[(id - 1) * 3 + q] - 1) & 1) * (c->box_size >> 1);
    }
  }
};

inline Level* level_ptr(omg_ctx* c, int l) {
  auto it = c->levels.find(l);
  return it == c->levels.end() ? nullptr : &it->second;
}

inline LevelView empty_view() {
  LevelView v;
  std::memset(&v, 0, sizeof(v));
  return v;
}

inline LevelView view_of(omg_ctx* c, int l) {
  Level* L = level_ptr(c, l);
  return L ? L->view() : empty_view();
}

// Group key-sorted (peer, key, item...) records into per-peer lists.
struct Rec {
  int peer;
  long long key;
  int a, b, c = 0;
};
std::vector<PeerList> group(std::vector<Rec>& recs, int ints_per_item);

// ---------------------------------------------------------------------------
// profiling: HIP events around kernel families on the context stream
constexpr int NO_LVL = INT_MIN;

// (on `st`, the context stream by default; with OMG_ROCTX set, a roctx range
// "name@lvl" around the host side of the step for rocprofv3 --marker-trace)
struct Prof {
  omg_ctx* c;
  const char* name;
  double cells;
  int lvl;
  hipStream_t st;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool range = false;
  Prof(omg_ctx* c_, const char* n, double cl, int l = NO_LVL, hipStream_t s = nullptr)
      : c(c_), name(n), cells(cl), lvl(l), st(s ? s : c_->stream) {
    if (c->roctx) {
      char buf[64];
      if (lvl == NO_LVL) std::snprintf(buf, sizeof(buf), "%s", name);
      else std::snprintf(buf, sizeof(buf), "%s@%d", name, lvl);
      roctxRangePushA(buf);
      range = true;
    }
    if (!c->profiling) return;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, st));
  }
  ~Prof() {
    if (range) roctxRangePop();
    if (!e0) return;
    (void)hipEventRecord(e1, st);
    c->pending.push_back({name, e0, e1, cells, lvl});
  }
};

// --- omg_transport.cpp
void loopback_unique_id(long long tag, void* out);
void host_unique_id(void* out);
void transport_attach(omg_ctx* c, const void* unique_id);
void transport_detach(omg_ctx* c);
std::vector<double> loop_allgather(omg_ctx* c, double v);
std::vector<double> host_allgather(omg_ctx* c, double v);
void exchange(omg_ctx* c, const Transfer& T, const double* sendbuf, double* recvbuf, hipStream_t st = nullptr,
              int lvl = NO_LVL);
double allreduce(omg_ctx* c, double v, bool is_max);

// --- omg_plan.cpp
void pack_topo(Level& L);
void finalize_transfer(Transfer& T);
void rbh_build(omg_ctx* c);
void ensure_rhs_lex(omg_ctx* c);
void free_levels(omg_ctx* c);
void build_plan(omg_ctx* c);

// --- omg_columns.cpp: the block passes' column and coarse records
void build_columns(omg_ctx* c, Level& L);
void build_coarse_columns(omg_ctx* c, Level& F, const Level& C);
void agree_columns(omg_ctx* c);
bool b3_usable(omg_ctx* c, int lvl, B3Phys& P, const B3Phys*& ph);
// (which 0: the column records, 1: the coarse records; empty: the level has none)
const std::vector<int>& columns_host(const Level& L, int which, int* rec_ints);

// --- omg_lazy.cpp: the lazy per-level state (omg_internal.h, above Level's
// lazy fields).  What a pass on a level reads and writes: ready() before its
// launch makes the level fit for it, wrote() after it records what it left.
enum Pass : unsigned {
  kPhi = 1,           // reads phi as stored: a pending mean is applied first
  kPhiAbsorb = 2,     // subtracts the pending mean while loading (its shift argument, red_mean)
  kPhiDead = 4,       // overwrites every value of phi unread: a pending mean is dropped
  kGhosts = 8,        // reads phi's ghost faces (the block passes read none of the same-GPU ones)
  kRhs = 16,          // reads rhs as stored (a pass that takes rhs_shifts says nothing)
  kRhsWrite = 32,     // writes rhs
  kResWrite = 64,     // writes res of every box
  kWrite = 128,       // writes d_phi
  kWriteOther = 256,  // writes other_phi, which becomes d_phi
  kGcAll = 512, kGcNone = 1024, kGcStale = 2048,   // wrote(): the ghost faces it left (none of these: as they were)
};
void ready(omg_ctx* c, int lvl, unsigned pass);
void wrote(omg_ctx* c, int lvl, unsigned pass);
double* other_phi(const Level* L);
void rb_stale_above(omg_ctx* c, int lvl);
void phi_dirty(omg_ctx* c, int lvl);
void phi_dirty_all(omg_ctx* c);
// rhs's ghost slots were written: phi's ghosts are stale where they hold mg_phi_bc_store's data
void rhs_ghosts_written(omg_ctx* c, int lvl);
void rhs_ghosts_written_all(omg_ctx* c);
// (dead_lvl: that level's cycle overwrites its res, a pending one is dropped)
void materialize_res_all(omg_ctx* c, int dead_lvl = INT_MIN);
bool res_pend_ok(omg_ctx* c, const Level* L);
void phi_mean_ready(omg_ctx* c);
void materialize_phi(omg_ctx* c);
RhsShifts rhs_shifts(omg_ctx* c, const Level* L);
void materialize_rhs_all(omg_ctx* c);
// the smoothing counts, the smoother or the operator changed (rhs_pend_off and res_pend_off)
void rhs_pend_retry(omg_ctx* c);
bool rhs_pend_ok(omg_ctx* c, const Level* L);
void drop_rhs_lex(omg_ctx* c);
void drop_rhs_cache(omg_ctx* c);
void enter(omg_ctx* c, bool writes = true);

// --- omg_cycle.cpp
void fill_gc_lvl(omg_ctx* c, int lvl, int iv);
// block4: runs of four substeps as one k_gsrb4 pass, the last one's remote faces left in flight
bool smooth_boxes(omg_ctx* c, int lvl, int n_cycle, int first_substep = 1, int skip_last = 0,
                  bool want_res = false, bool block4 = false);
void residual_lvl(omg_ctx* c, int lvl, unsigned long long* maxbits);
double max_residual_lvl(omg_ctx* c, int lvl);
void restrict_lvl(omg_ctx* c, int iv, int lvl);
void prolong(omg_ctx* c, int lvl, int iv, int iv_to, int add);
// res_may_pend: the caller is a stand-alone cycle on its top level, whose
// stored res nothing reads before it is overwritten (Level::res_pend)
void update_coarse(omg_ctx* c, int lvl, bool fused = false, bool tail_crhs = false, bool res_may_pend = false);
void correct_children(omg_ctx* c, int lvl);
void check_finite_res(double r, const char* where);
double fas_vcycle(omg_ctx* c, int highest_lvl, bool want_max_res, bool standalone);
double fas_fmg(omg_ctx* c, bool have_guess, bool want_max_res);
// (the cycle `body` as one HIP graph where graph_ok(), else called directly)
double run_cycle(omg_ctx* c, int key, const std::function<double()>& body);
void set_operator(omg_ctx* c, int op, double lambda);
void apply_op(omg_ctx* c, int i_out);
void set_rhs(omg_ctx* c, double f1, double f2);
void diffusion_solve(omg_ctx* c, int op, double dt, double coeff, int order, double max_res, int* n_vcycles,
                     double* res_out);
void phi_bc_store(omg_ctx* c);

// --- omg_mean.cpp
enum { kChPhi = 0, kChRhs = 1 };
double* red_mean(omg_ctx* c, int ch);
void mean_device(omg_ctx* c, int ch, double* mean);
double get_sum(omg_ctx* c, int iv);
enum { kPlain = 0, kInCycle = 1 };
void subtract_mean(omg_ctx* c, int iv, int ghosts, int mode = kPlain);

// --- omg_devio.cpp
void dense_io(omg_ctx* c, int lvl, int iv, double* dev, const long long* lo, const long long* n,
              const long long* stride, void* stream, long long* n_cells, bool put);
void dense_grad(omg_ctx* c, int lvl, int iv, double* const* dev, const long long* lo, const long long* n,
                const long long* stride, double scale, bool fill, void* stream, long long* n_cells);
void box_io(omg_ctx* c, int iv, int n_boxes, const int* ids, double* dev, const long long* box_off,
            const long long* stride, int ghost, bool fill, void* stream, long long* n_cells, bool put);
void boxes_grad(omg_ctx* c, int iv, int n_boxes, const int* ids, double* const* dev, const long long* box_off,
                const long long* stride, double scale, int centering, bool fill, void* stream, long long* n_cells);
void boxes_div(omg_ctx* c, int iv, int n_boxes, const int* ids, const double* const* dev, const long long* box_off,
               const long long* stride, double scale, int centering, void* stream, long long* n_cells);
void boxes_flux(omg_ctx* c, int iv, const int* iv_coef, int n_boxes, const int* ids, double* const* dev,
                const long long* box_off, const long long* stride, double scale, int centering, bool accumulate,
                bool fill, void* stream, long long* n_cells);

// --- omg_free_host.cpp
void free_state_destroy(omg_ctx* c);
double poisson_free_3d(omg_ctx* c, bool new_rhs, double max_fft_frac, bool fmgcycle, bool want_max_res,
                       const double* r_min, const double* box_r_min);

}  // namespace host
}  // namespace omg
