// omg_boxes.hip — device block I/O (omg_put_boxes / omg_get_boxes): variable
// iv of a list of boxes, on any levels, <-> the caller's block pool in device
// memory.  Element (i,j,k) of a record's block is
//     dev[rec.off + (i-1) + (j-1)*s1 + (k-1)*s2],
// GHOST = 0 moves the interior 1 <= i,j,k <= nc, GHOST = 1 also the six
// face-ghost layers (the cells the device stores, omg_device.h); edge and
// corner elements of the block are never touched.
//
// Tile kernel (box sizes 16 and 8).  One workgroup per record, an LDS copy of
// the stored box in the stored layout (Tl<NC>):
//   library side: the stored box [colour 0 | colour 1 | 6 faces] is one
//     contiguous, 16-B aligned run, so the copy between it and LDS is linear,
//     16 B per lane on both (ds_*_b128 at consecutive addresses);
//   caller's side: a row (j,k) is contiguous over i = 0..nc+1, so the x-face
//     ghosts ride at the ends of the interior rows and the y and z faces are
//     whole rows.  Every row is cut into 16-B aligned pairs of cells by the
//     parity a of the address of its cell i = 1:
//       a = 0  pairs (1,2) .. (nc-1,nc); with ghosts, the cells 0 and nc+1
//              are single 8-B accesses;
//       a = 1  pairs (0,1) .. (nc,nc+1): with ghosts every access of an
//              interior row is a whole pair; without, cells 1 and nc are
//              peeled (8-B accesses).
//     The parity is taken per row, so odd strides stay here too.  W8: the
//     other odd-alignment variant, one 8-B access per cell.
//   LDS pitch: the stored layout itself, unpadded.  The two cells of a pair
//     are one slot of each colour half; lanes that walk along a row, and on
//     into the next row, read consecutive 8-B words of a half, and the halves
//     (and the rows' alternation between them) lie HV*8 = 16 KiB (2 KiB for
//     8^3) apart, a multiple of the 256-B bank cycle: the 64 lanes of a wave
//     fall on 64 different word pairs modulo the banks except where a row
//     ends (the shorter rows of unit slots), conflict-free for the interior.
//     The x-face ghosts of rows j and j+1 are the same slot of the two colour
//     halves of a face, FH*8 B apart (a multiple of 256 B): a two-way
//     conflict on 2/(nc+6) of the cells, left as it is.
// A lane issues its global loads before its stores; plain (temporal) accesses
// (DESIGN §14 measured non-temporal ones slower on both sides).
//
// Per-cell kernel: any box size, through off_cell, `bpc` workgroups per
// record; also everything under OMG_BOXES_GENERIC=1.  Both give the same
// bits: they copy.
#include "omg_device.h"
#include "omg_kernels.h"

namespace omg {

typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int boxes_tile_block(int NC) { return NC == 16 ? 256 : 128; }
// doubles of the LDS copy: the stored box, without the faces when they stay
template <int NC, int GHOST>
constexpr int kBoxesLds = GHOST ? Tl<NC>::NST : 2 * Tl<NC>::HV;

// One unit of the caller's side: the cells c and c+1 of row (j,k), or only c
// (W8).  Returns the validity of the two cells and their LDS slots.
template <int NC, int GHOST, bool W8>
struct BoxUnits {
  static constexpr int M = NC + 2 * GHOST;                         // rows per plane, planes
  static constexpr int UPR = W8 ? M : NC / 2 + 1 + GHOST;          // units per row
  static constexpr int N = M * M * UPR;                            // units per box
  static constexpr int BS = boxes_tile_block(NC);
  static constexpr int IT = (N + BS - 1) / BS;
  const double* base;   // the address of the record's cell (1,1,1)
  long long s1, s2;
  // v0, v1: the cells are stored cells of the block; o0, o1 their LDS slots;
  // returns the address of cell c
  __device__ __forceinline__ double* unit(int t, bool& v0, bool& v1, int& o0, int& o1) const {
    const int u = t % UPR, r = t / UPR;
    const int j = r % M + 1 - GHOST, k = r / M + 1 - GHOST;
    double* row = const_cast<double*>(base) + ((long long)(j - 1) * s1 + (long long)(k - 1) * s2);
    const bool jb = j == 0 || j == NC + 1, kb = k == 0 || k == NC + 1;
    const int g = (GHOST && !jb && !kb) ? 1 : 0;   // the row carries its x-face ghosts
    int c;
    if (W8) {
      c = u + 1 - GHOST;
    } else {
      const int a = (int)(((unsigned long long)row >> 3) & 1);
      c = 2 * u + (GHOST ? a - 1 : 1 - a);
    }
    const bool rv = t < N && !(jb && kb);
    v0 = rv && c >= 1 - g && c <= NC + g;
    v1 = !W8 && rv && c + 1 >= 1 - g && c + 1 <= NC + g;
    o0 = v0 ? Tl<NC>::ocell(c, j, k) : 0;
    o1 = v1 ? Tl<NC>::ocell(c + 1, j, k) : 0;
    return row + (c - 1);
  }
};

template <int NC, int GHOST, bool PUT, bool W8>
__global__ void __launch_bounds__(boxes_tile_block(NC))
k_boxes_tile(LevelView L, int iv, const BoxRec* __restrict__ recs, double* __restrict__ dev, long long s1,
             long long s2) {
  using U = BoxUnits<NC, GHOST, W8>;
  constexpr int BS = U::BS, NL = kBoxesLds<NC, GHOST>, NQ = NL / 2, ITL = (NQ + BS - 1) / BS;
  __shared__ __attribute__((aligned(16))) double sh[NL];
  const BoxRec rec = recs[blockIdx.x];
  double* __restrict__ box = boxp(L, iv, rec.box);
  const U un{dev + rec.off, s1, s2};
  const int tid = threadIdx.x;
  if (PUT) {
    // the caller's block -> LDS (every load first) ...
    d2 w[U::IT];
#pragma unroll
    for (int q = 0; q < U::IT; q++) {
      bool v0, v1;
      int o0, o1;
      const double* p = un.unit(tid + q * BS, v0, v1, o0, o1);
      w[q] = d2{0.0, 0.0};
      if (v0 && v1) w[q] = *reinterpret_cast<const d2*>(p);
      else if (v0) w[q].x = p[0];
      else if (v1) w[q].y = p[1];
    }
#pragma unroll
    for (int q = 0; q < U::IT; q++) {
      bool v0, v1;
      int o0, o1;
      (void)un.unit(tid + q * BS, v0, v1, o0, o1);
      if (v0) sh[o0] = w[q].x;
      if (v1) sh[o1] = w[q].y;
    }
    __syncthreads();
    // ... -> the stored box, linear
    d2 x[ITL];
#pragma unroll
    for (int q = 0; q < ITL; q++) {
      const int t = tid + q * BS;
      if (t < NQ) x[q] = reinterpret_cast<const d2*>(sh)[t];
    }
#pragma unroll
    for (int q = 0; q < ITL; q++) {
      const int t = tid + q * BS;
      if (t < NQ) reinterpret_cast<d2*>(box)[t] = x[q];
    }
  } else {
    d2 x[ITL];
#pragma unroll
    for (int q = 0; q < ITL; q++) {
      const int t = tid + q * BS;
      if (t < NQ) x[q] = reinterpret_cast<const d2*>(box)[t];
    }
#pragma unroll
    for (int q = 0; q < ITL; q++) {
      const int t = tid + q * BS;
      if (t < NQ) reinterpret_cast<d2*>(sh)[t] = x[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < U::IT; q++) {
      bool v0, v1;
      int o0, o1;
      double* p = un.unit(tid + q * BS, v0, v1, o0, o1);
      const d2 w{sh[o0], sh[o1]};
      if (v0 && v1) *reinterpret_cast<d2*>(p) = w;
      else if (v0) p[0] = w.x;
      else if (v1) p[1] = w.y;
    }
  }
}

// Any box size: one stored cell of the (nc + 2*ghost)^3 block per thread.
template <bool PUT>
__global__ void __launch_bounds__(256)
k_boxes_cell(LevelView L, int iv, const BoxRec* recs, int bpc, int ghost, double* dev, long long s1, long long s2) {
  const BoxRec rec = recs[blockIdx.x / bpc];
  const int nc = L.nc, m = nc + 2 * ghost, total = m * m * m;
  double* box = boxp(L, iv, rec.box);
  double* blk = dev + rec.off;
  for (int t = (blockIdx.x % bpc) * 256 + threadIdx.x; t < total; t += bpc * 256) {
    const int i = t % m + 1 - ghost, j = (t / m) % m + 1 - ghost, k = t / (m * m) + 1 - ghost;
    const int nb = (i == 0 || i == nc + 1) + (j == 0 || j == nc + 1) + (k == 0 || k == nc + 1);
    if (nb > 1) continue;   // edges and corners are not stored
    double* d = blk + ((i - 1) + (long long)(j - 1) * s1 + (long long)(k - 1) * s2);
    double* p = box + off_cell(L, i, j, k);
    if (PUT) *p = *d;
    else *d = *p;
  }
}

bool boxes_tile_nc(int nc) { return nc == 16 || nc == 8; }

template <int NC, int GHOST, bool PUT>
static void launch_tile_w(const LevelView& L, int iv, const BoxRec* recs, int n, double* dev, long long s1,
                          long long s2, bool w8, hipStream_t st) {
  if (w8) k_boxes_tile<NC, GHOST, PUT, true><<<n, boxes_tile_block(NC), 0, st>>>(L, iv, recs, dev, s1, s2);
  else k_boxes_tile<NC, GHOST, PUT, false><<<n, boxes_tile_block(NC), 0, st>>>(L, iv, recs, dev, s1, s2);
}

template <int NC>
static void launch_tile_nc(const LevelView& L, int iv, const BoxRec* recs, int n, double* dev, long long s1,
                           long long s2, int ghost, bool put, bool w8, hipStream_t st) {
  if (ghost) {
    if (put) launch_tile_w<NC, 1, true>(L, iv, recs, n, dev, s1, s2, w8, st);
    else launch_tile_w<NC, 1, false>(L, iv, recs, n, dev, s1, s2, w8, st);
  } else {
    if (put) launch_tile_w<NC, 0, true>(L, iv, recs, n, dev, s1, s2, w8, st);
    else launch_tile_w<NC, 0, false>(L, iv, recs, n, dev, s1, s2, w8, st);
  }
}

void launch_boxes_tile(const LevelView& L, int iv, const BoxRec* recs, int n, double* dev, long long s1,
                       long long s2, int ghost, bool put, bool w8, hipStream_t st) {
  if (n <= 0) return;
  if (L.nc == 16) launch_tile_nc<16>(L, iv, recs, n, dev, s1, s2, ghost, put, w8, st);
  else launch_tile_nc<8>(L, iv, recs, n, dev, s1, s2, ghost, put, w8, st);
}

int boxes_cell_bpc(int nc, int ghost) {
  const long long m = nc + 2 * ghost;
  return cell_bpc(m * m * m);
}

void launch_boxes_cell(const LevelView& L, int iv, const BoxRec* recs, int n, double* dev, long long s1,
                       long long s2, int ghost, bool put, hipStream_t st) {
  if (n <= 0) return;
  const int bpc = boxes_cell_bpc(L.nc, ghost);
  const unsigned grid = (unsigned)((long long)n * bpc);
  if (put) k_boxes_cell<true><<<grid, 256, 0, st>>>(L, iv, recs, bpc, ghost, dev, s1, s2);
  else k_boxes_cell<false><<<grid, 256, 0, st>>>(L, iv, recs, bpc, ghost, dev, s1, s2);
}

}  // namespace omg
