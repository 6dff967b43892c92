// omg_transport.cpp — how the ranks of a context talk: the in-process
// loopback transport, the caller's host transport, the grouped RCCL round
// (exchange) and the one-double allreduce in the reference's MPI order.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "omg_host.h"

namespace omg {
namespace host {

constexpr char kLoopMagic[16] = "OMG-LOOPBACK-v1";
static std::mutex g_loop_mu;
static std::map<long long, std::shared_ptr<omg_loop>> g_loops;

template <typename Pred>
static void loop_wait(omg_ctx* c, std::unique_lock<std::mutex>& lk, Pred pred, const std::string& what) {
  if (!c->loop->cv.wait_for(lk, std::chrono::seconds(60), pred))
    throw OmgError(std::string("loopback transport: rank ") + std::to_string(c->rank) +
                   " timed out waiting for " + what);
}

static hipEvent_t loop_event(hipStream_t st) {
  hipEvent_t e;
  HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIPCHK(hipEventRecord(e, st));
  return e;
}

static void loop_exchange(omg_ctx* c, const Transfer& T, const double* sendbuf, double* recvbuf, hipStream_t st) {
  omg_loop& G = *c->loop;
  const size_t per = (size_t)T.item_doubles;
  const int me = c->rank;
  for (auto& p : T.send) {
    const size_t n = p.items.size() / T.send_ints * per;
    hipEvent_t ev = loop_event(st);
    std::lock_guard<std::mutex> lk(G.mu);
    G.box[{me, p.peer, c->loop_seq_send[p.peer]}] = {sendbuf + (size_t)p.offset * per, n, ev};
    G.cv.notify_all();
  }
  for (auto& p : T.recv) {
    const size_t n = p.items.size() / T.recv_ints * per;
    const omg_loop::Key k{p.peer, me, c->loop_seq_recv[p.peer]};
    omg_loop::Msg m;
    {
      std::unique_lock<std::mutex> lk(G.mu);
      loop_wait(c, lk, [&] { return G.box.count(k) > 0; },
                "a message from rank " + std::to_string(p.peer) + " (pair sequence " +
                    std::to_string(std::get<2>(k)) + ", " + std::to_string(n) + " doubles)");
      m = G.box[k];
      G.box.erase(k);
    }
    if (m.n != n) throw OmgError("loopback transport: message size mismatch");
    HIPCHK(hipStreamWaitEvent(st, m.ev, 0));
    HIPCHK(hipMemcpyAsync(recvbuf + (size_t)p.offset * per, m.src, n * sizeof(double),
                          hipMemcpyDeviceToDevice, st));
    HIPCHK(hipEventDestroy(m.ev));
  }
  for (auto& p : T.recv) {   // the sender may reuse its buffer once our copies ran
    hipEvent_t ev = loop_event(st);
    std::lock_guard<std::mutex> lk(G.mu);
    G.acks[{me, p.peer, c->loop_seq_recv[p.peer]++}] = ev;
    G.cv.notify_all();
  }
  for (auto& p : T.send) {
    const omg_loop::Key k{p.peer, me, c->loop_seq_send[p.peer]++};
    hipEvent_t ev;
    {
      std::unique_lock<std::mutex> lk(G.mu);
      loop_wait(c, lk, [&] { return G.acks.count(k) > 0; },
                "the acknowledgement of rank " + std::to_string(p.peer) + " (pair sequence " +
                    std::to_string(std::get<2>(k)) + ")");
      ev = G.acks[k];
      G.acks.erase(k);
    }
    HIPCHK(hipStreamWaitEvent(st, ev, 0));
    HIPCHK(hipEventDestroy(ev));
  }
}

// every rank's value, in rank order (the loopback MPI_Allgather)
std::vector<double> loop_allgather(omg_ctx* c, double v) {
  omg_loop& G = *c->loop;
  const long long s = c->loop_ar_seq++;
  std::unique_lock<std::mutex> lk(G.mu);
  auto& vals = G.vals[s];
  vals.resize(G.n_ranks);
  vals[c->rank] = v;
  G.n_in[s]++;
  G.cv.notify_all();
  loop_wait(c, lk, [&] { return G.n_in[s] == G.n_ranks; },
            "allreduce #" + std::to_string(s) + " (" + std::to_string(G.n_in[s]) + " ranks in)");
  std::vector<double> all = G.vals[s];
  if (++G.n_out[s] == G.n_ranks) {
    G.vals.erase(s);
    G.n_in.erase(s);
    G.n_out.erase(s);
  }
  return all;
}

// ---------------------------------------------------------------------------
// Host transport (omg_set_host_transport): the caller's messaging (the
// Fortran drop-in: MPI, the reference's own transport) over pinned host
// staging.  Every round waits on the host: the segments leave the device
// after the stream's work so far, arrive before anything queued after.
constexpr char kHostMagic[16] = "OMG-HOSTXPRT-v1";

static double* host_stage(double*& p, size_t& cap, size_t n) {
  if (n > cap) {
    if (p) HIPCHK(hipHostFree(p));
    p = nullptr;
    HIPCHK(hipHostMalloc(&p, sizeof(double) * std::max<size_t>(n, 1)));
    cap = n;
  }
  return p;
}

static void host_exchange(omg_ctx* c, const Transfer& T, const double* sendbuf, double* recvbuf, hipStream_t st) {
  if (!c->hx_exchange) throw OmgError("host transport: omg_set_host_transport was not called");
  const size_t per = (size_t)T.item_doubles;
  size_t ns = 0, nr = 0;
  for (auto& p : T.send) ns = std::max(ns, ((size_t)p.offset + p.items.size() / T.send_ints) * per);
  for (auto& p : T.recv) nr = std::max(nr, ((size_t)p.offset + p.items.size() / T.recv_ints) * per);
  double* hs = host_stage(c->h_xsend, c->h_xsend_n, ns);
  double* hr = host_stage(c->h_xrecv, c->h_xrecv_n, nr);
  std::vector<int> sp, rp;
  std::vector<long long> sn, rn;
  std::vector<const double*> sb;
  std::vector<double*> rb;
  for (auto& p : T.send) {
    const size_t n = p.items.size() / T.send_ints * per;
    HIPCHK(hipMemcpyAsync(hs + (size_t)p.offset * per, sendbuf + (size_t)p.offset * per, n * sizeof(double),
                          hipMemcpyDeviceToHost, st));
    sp.push_back(p.peer);
    sn.push_back((long long)n);
    sb.push_back(hs + (size_t)p.offset * per);
  }
  for (auto& p : T.recv) {
    rp.push_back(p.peer);
    rn.push_back((long long)(p.items.size() / T.recv_ints * per));
    rb.push_back(hr + (size_t)p.offset * per);
  }
  host_sync(c, st);
  if (c->hx_exchange(c->hx_user, (int)sp.size(), sp.data(), sn.data(), sb.data(), (int)rp.size(), rp.data(),
                     rn.data(), rb.data()) != 0)
    throw OmgError("host transport: the exchange callback failed");
  for (size_t i = 0; i < rp.size(); i++)
    HIPCHK(hipMemcpyAsync(recvbuf + (rb[i] - hr), rb[i], (size_t)rn[i] * sizeof(double), hipMemcpyHostToDevice,
                          st));
  host_sync(c, st);   // (the staging is reused by the next round)
}

std::vector<double> host_allgather(omg_ctx* c, double v) {
  if (!c->hx_allgather) throw OmgError("host transport: omg_set_host_transport was not called");
  std::vector<double> all(c->n_ranks);
  if (c->hx_allgather(c->hx_user, &v, 1, all.data()) != 0)
    throw OmgError("host transport: the allgather callback failed");
  return all;
}

// One grouped RCCL round: send segment i to peer i, receive likewise
// (replaces sort_and_transfer_buffers, m_communication.f90:37-66).
void exchange(omg_ctx* c, const Transfer& T, const double* sendbuf, double* recvbuf, hipStream_t st, int lvl) {
  if (c->n_ranks == 1) return;
  if (T.send.empty() && T.recv.empty()) return;
  if (!st) st = c->stream;
  // "comm": one grouped round, timed on the stream it runs on; cells = the
  // doubles this rank receives
  Prof prof(c, st == c->stream ? "comm" : "comm_overlap", (double)T.n_recv * T.item_doubles, lvl, st);
  if (c->loop) {
    loop_exchange(c, T, sendbuf, recvbuf, st);
    return;
  }
  if (c->host_xport) {
    host_exchange(c, T, sendbuf, recvbuf, st);
    return;
  }
  ncclComm_t comm = (ncclComm_t)c->nccl;
  const size_t per = (size_t)T.item_doubles;
  NCCLCHK(ncclGroupStart());
  for (auto& p : T.send) {
    size_t n = p.items.size() / (T.send_ints) * per;
    NCCLCHK(ncclSend(sendbuf + (size_t)p.offset * per, n, ncclDouble, p.peer, comm, st));
  }
  for (auto& p : T.recv) {
    size_t n = p.items.size() / (T.recv_ints) * per;
    NCCLCHK(ncclRecv(recvbuf + (size_t)p.offset * per, n, ncclDouble, p.peer, comm, st));
  }
  NCCLCHK(ncclGroupEnd());
}

// MPI_Allreduce of one double: max exactly; sum in the recursive-doubling
// pairwise order of MPICH for power-of-two communicators.
double allreduce(omg_ctx* c, double v, bool is_max) {
  if (c->n_ranks == 1) return v;
  std::vector<double> all(c->n_ranks);
  if (c->loop) {
    all = loop_allgather(c, v);
  } else if (c->host_xport) {
    all = host_allgather(c, v);
  } else {
    double* d = c->d_scalar + 8;
    c->h_scalar[1] = v;
    HIPCHK(hipMemcpyAsync(d, &c->h_scalar[1], 8, hipMemcpyHostToDevice, c->stream));
    NCCLCHK(ncclAllGather(d, d + 1, 1, ncclDouble, (ncclComm_t)c->nccl, c->stream));
    HIPCHK(hipMemcpyAsync(all.data(), d + 1, 8 * c->n_ranks, hipMemcpyDeviceToHost, c->stream));
    host_sync(c, c->stream);
  }
  if (is_max) {
    // the device max is on IEEE bits (amax): NaN and Inf propagate; so must
    // the combination over ranks (std::max_element skips a NaN past all[0])
    double m = all[0];
    for (double x : all) {
      if (std::isnan(x)) return x;
      m = x > m ? x : m;
    }
    return m;
  }
  // MPI_Allreduce(MPI_SUM) as MPICH 3.3.2 computes it on one node
  // (m_multigrid.f90:255): a binomial-tree reduce to rank 0 in rank order,
  // ((a0+a1)+(a2+a3))+a4 ..., then a broadcast.  Pinned by the golden runs
  // of the reference at 1-6 and 8 ranks (per32_gsrb_v).
  for (int w = 1; w < c->n_ranks; w *= 2)
    for (int r = 0; r + w < c->n_ranks; r += 2 * w) all[r] = all[r] + all[r + w];
  return all[0];
}

// ---------------------------------------------------------------------------
// The unique ids that select the two in-process transports
// (omg_loopback_unique_id, omg_host_unique_id): a magic string, then the
// loopback group's tag.
void loopback_unique_id(long long tag, void* out) {
  std::memset(out, 0, OMG_UNIQUE_ID_BYTES);
  std::memcpy(out, kLoopMagic, sizeof(kLoopMagic));
  std::memcpy((char*)out + sizeof(kLoopMagic), &tag, sizeof(tag));
}

void host_unique_id(void* out) {
  std::memset(out, 0, OMG_UNIQUE_ID_BYTES);
  std::memcpy(out, kHostMagic, sizeof(kHostMagic));
}

// omg_ctx_create: the context joins the transport its unique_id names
void transport_attach(omg_ctx* c, const void* unique_id) {
  const int n_ranks = c->n_ranks, rank = c->rank;
  if (n_ranks > 1 && std::memcmp(unique_id, kLoopMagic, sizeof(kLoopMagic)) == 0) {
    long long tag;
    std::memcpy(&tag, (const char*)unique_id + sizeof(kLoopMagic), sizeof(tag));
    std::lock_guard<std::mutex> lk(g_loop_mu);
    auto& g = g_loops[tag];
    if (!g) {
      g = std::make_shared<omg_loop>();
      g->n_ranks = n_ranks;
    }
    if (g->n_ranks != n_ranks) throw OmgError("loopback group: n_ranks mismatch");
    c->loop = g;
  } else if (n_ranks > 1 && std::memcmp(unique_id, kHostMagic, sizeof(kHostMagic)) == 0) {
    c->host_xport = true;   // the callbacks come with omg_set_host_transport
  } else if (n_ranks > 1) {
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    ncclComm_t comm;
    NCCLCHK(ncclCommInitRank(&comm, n_ranks, id, rank));
    c->nccl = comm;
  }
}

// omg_ctx_destroy: and leaves it
void transport_detach(omg_ctx* c) {
  if (c->nccl) (void)ncclCommDestroy((ncclComm_t)c->nccl);
  if (c->loop) {   // the last context of a loopback group removes it
    std::lock_guard<std::mutex> lk(g_loop_mu);
    for (auto it = g_loops.begin(); it != g_loops.end(); ++it)
      if (it->second == c->loop && it->second.use_count() == 2) {
        g_loops.erase(it);
        break;
      }
    c->loop.reset();
  }
}

}  // namespace host
}  // namespace omg
