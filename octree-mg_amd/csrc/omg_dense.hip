// omg_dense.hip — dense device I/O (omg_put_dense / omg_get_dense): the
// interior cells of a level's boxes <-> a dense window [z][y][x] of the
// level's cell grid in the caller's device memory.  Ghost slots are never
// touched.  The host (omg_devio.cpp) clips every box against the window into a
// DenseClip record; the row kernel serves the boxes whose covered rows are
// whole in x and 16-B aligned in the window, the per-cell kernel the others.
//
// Row kernel (box sizes 16 and 8).  One workgroup per box; a lane owns the
// four cells i = 4q+1 .. 4q+4 of one row (j, k): two 16-B accesses on the
// dense side.  The colour of cell i is e = (i+j+k) & 1 and its slot in the
// colour half (i-1) >> 1 (omg_device.h), so cells 4q+1 and 4q+3 are slots 2q
// and 2q+1 of colour (1+j+k) & 1 and cells 4q+2 and 4q+4 the same slots of
// the other colour: one 16-B access per colour half at
//     e*HV + 2q + H*((j-1) + NC*(k-1)),
// 16-B aligned because H and the boxes' stride are even.  16 B of traffic per
// cell, all of it 16 B per lane; no LDS, no division by a runtime value.
// Plain accesses: non-temporal ones on either side measured slower.
#include "omg_device.h"
#include "omg_kernels.h"

namespace omg {

typedef double d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ d2 ld2(const double* p) { return *reinterpret_cast<const d2*>(p); }
__device__ __forceinline__ void st2(double* p, d2 v) { *reinterpret_cast<d2*>(p) = v; }

constexpr int dense_row_block(int NC) { return NC == 16 ? 256 : 128; }

// WHOLE: the window covers every row of the box (no test per row)
template <int NC, bool PUT, bool WHOLE>
__device__ __forceinline__ void dense_rows(const DenseClip& c, double* __restrict__ box, double* __restrict__ dense,
                                           long long s1, long long s2) {
  constexpr int H = NC / 2, HV = H * NC * NC, LPR = NC / 4, BS = dense_row_block(NC);
  constexpr int RPP = BS / LPR, IT = NC * NC / RPP;   // rows per pass, passes
  const int q = threadIdx.x % LPR, r0 = threadIdx.x / LPR;
  // every load of the lane's rows first, then the stores: the loads of all
  // passes are in flight together
  d2 u[IT], v[IT];
#pragma unroll
  for (int t = 0; t < IT; t++) {
    const int r = r0 + t * RPP, j = r % NC + 1, k = r / NC + 1;
    if (!WHOLE && (j < c.j0 || j > c.j1 || k < c.k0 || k > c.k1)) continue;
    const int o = 2 * q + H * ((j - 1) + NC * (k - 1));
    const int ea = (1 + j + k) & 1;   // colour of cells 4q+1 and 4q+3
    if (PUT) {
      const double* d = dense + (c.off + (long long)(j - c.j0) * s1 + (long long)(k - c.k0) * s2 + 4 * q);
      u[t] = ld2(d);
      v[t] = ld2(d + 2);
    } else {
      u[t] = ld2(box + ea * HV + o);
      v[t] = ld2(box + (ea ^ 1) * HV + o);
    }
  }
#pragma unroll
  for (int t = 0; t < IT; t++) {
    const int r = r0 + t * RPP, j = r % NC + 1, k = r / NC + 1;
    if (!WHOLE && (j < c.j0 || j > c.j1 || k < c.k0 || k > c.k1)) continue;
    const int o = 2 * q + H * ((j - 1) + NC * (k - 1));
    const int ea = (1 + j + k) & 1;
    if (PUT) {
      st2(box + ea * HV + o, d2{u[t].x, v[t].x});
      st2(box + (ea ^ 1) * HV + o, d2{u[t].y, v[t].y});
    } else {
      double* d = dense + (c.off + (long long)(j - c.j0) * s1 + (long long)(k - c.k0) * s2 + 4 * q);
      st2(d, d2{u[t].x, v[t].x});
      st2(d + 2, d2{u[t].y, v[t].y});
    }
  }
}

template <int NC, bool PUT>
__global__ void __launch_bounds__(dense_row_block(NC))
k_dense_row(LevelView L, int iv, const DenseClip* __restrict__ clips, double* __restrict__ dense, long long s1,
            long long s2) {
  const DenseClip c = clips[blockIdx.x];
  double* __restrict__ box = boxp(L, iv, c.box);
  if (c.j0 == 1 && c.j1 == NC && c.k0 == 1 && c.k1 == NC) dense_rows<NC, PUT, true>(c, box, dense, s1, s2);
  else dense_rows<NC, PUT, false>(c, box, dense, s1, s2);
}

// Everything else (odd box sizes, 2^3 and 4^3 boxes, partial rows, odd offsets,
// unaligned bases): one cell per thread, `bpc` workgroups per record.
template <bool PUT>
__global__ void __launch_bounds__(256)
k_dense_cell(LevelView L, int iv, const DenseClip* clips, int bpc, double* dense, long long s1, long long s2) {
  const DenseClip c = clips[blockIdx.x / bpc];
  const int ni = c.i1 - c.i0 + 1, nj = c.j1 - c.j0 + 1, nk = c.k1 - c.k0 + 1;
  const int total = ni * nj * nk;
  double* box = boxp(L, iv, c.box);
  for (int t = (blockIdx.x % bpc) * 256 + threadIdx.x; t < total; t += bpc * 256) {
    const int di = t % ni, dj = (t / ni) % nj, dk = t / (ni * nj);
    double* d = dense + (c.off + di + (long long)dj * s1 + (long long)dk * s2);
    double* p = box + off_int(L, c.i0 + di, c.j0 + dj, c.k0 + dk);
    if (PUT) *p = *d;
    else *d = *p;
  }
}

bool dense_row_nc(int nc) { return nc == 16 || nc == 8; }

void launch_dense_row(const LevelView& L, int iv, const DenseClip* clips, int n, double* dense, long long s1,
                      long long s2, bool put, hipStream_t st) {
  if (n <= 0) return;
  if (L.nc == 16) {
    if (put) k_dense_row<16, true><<<n, dense_row_block(16), 0, st>>>(L, iv, clips, dense, s1, s2);
    else k_dense_row<16, false><<<n, dense_row_block(16), 0, st>>>(L, iv, clips, dense, s1, s2);
  } else {
    if (put) k_dense_row<8, true><<<n, dense_row_block(8), 0, st>>>(L, iv, clips, dense, s1, s2);
    else k_dense_row<8, false><<<n, dense_row_block(8), 0, st>>>(L, iv, clips, dense, s1, s2);
  }
}

void launch_dense_cell(const LevelView& L, int iv, const DenseClip* clips, int n, double* dense, long long s1,
                       long long s2, bool put, hipStream_t st) {
  if (n <= 0) return;
  const int bpc = cell_bpc((long long)L.nc * L.nc * L.nc);
  const unsigned grid = (unsigned)((long long)n * bpc);
  if (put) k_dense_cell<true><<<grid, 256, 0, st>>>(L, iv, clips, bpc, dense, s1, s2);
  else k_dense_cell<false><<<grid, 256, 0, st>>>(L, iv, clips, bpc, dense, s1, s2);
}

}  // namespace omg
