// omg_dense_grad.hip — omg_get_dense_grad: the central differences of a
// variable over the stored box and its six ghost faces,
//     g_d(i,j,k) = (cc(+1 in d) - cc(-1 in d)) * f_d,   f_d = 0.5*scale/dr_d,
// written as up to three dense windows [z][y][x] that share the clip records
// of omg_get_dense (DenseClip).  One subtraction and one multiplication per
// value (grad_value, shared by both kernels; the library builds with
// -ffp-contract=off).  Edge and corner ghosts are never needed.
//
// Tile kernel (box sizes 16 and 8, the row conditions of k_dense_row).  One
// workgroup per record stages the stored box in LDS in plain (NC+2)^3 order,
// T[i + PT*(j + PT*k)] with PT = NC+2 doubles (even: every 16-B read below is
// aligned): both colour halves with 16-B loads as k_dense_row does, the six
// ghost faces with 16-B loads of two ghosts of one colour (tangential a and
// a+2).  All global loads are issued before the one barrier.  Then a lane
// owns the cells i = 4q+1 .. 4q+4 of a row (j, k): the x component reads the
// row's cells 4q .. 4q+5 as three 16-B LDS reads, the y and z components the
// same three pairs of rows j-1, j+1 / k-1, k+1, and every component goes out
// as two 16-B stores.  A skipped component is a wave-uniform branch.
//
// LDS banks (ds_read_b128: groups of 16 lanes, 16-B slots modulo 16 must
// differ inside a group).  At NC = 16 a row's four lanes take the slots
// 9*row + 162*k + {0, 2, 4, 6} (+ a constant per read), so a group is
// conflict-free when its four rows are {a, a+8, b, b+8} with a even and b
// odd; tile_row16() hands the wave's 16 rows of a plane out that way.  At
// NC = 8 the natural order stays (two lanes per row, DESIGN).
#include "omg_device.h"
#include "omg_kernels.h"

namespace omg {

typedef double d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ d2 ld2(const double* p) { return *reinterpret_cast<const d2*>(p); }
__device__ __forceinline__ void st2(double* p, d2 v) { *reinterpret_cast<d2*>(p) = v; }

// the one place the arithmetic lives: both kernels give the same bits
__device__ __forceinline__ double grad_value(double hi, double lo, double f) { return (hi - lo) * f; }

constexpr int grad_tile_block(int NC) { return NC == 16 ? 256 : 128; }

// The row (0-based j) of the wave's row slot s = 0..15 at NC = 16.  The 16-B
// reads are served in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}
// and the same of the upper half: row slots {0,3,5,6}, {1,2,4,7}, {8,11,13,14},
// {9,10,12,15}, i.e. group g = 2*(s>>3) + parity(s&7), member m = (s>>1)&3.
// Group g gets the rows 2g, 2g+8, 2g+1, 2g+9.
__device__ __forceinline__ int tile_row16(int s) {
  const int g = 2 * (s >> 3) + (__popc(s & 7) & 1), m = (s >> 1) & 3;
  return 2 * g + 8 * (m & 1) + (m >> 1);
}

template <int NC>
__global__ void __launch_bounds__(grad_tile_block(NC))
k_dense_grad_tile(LevelView L, int iv, const DenseClip* __restrict__ clips, DenseGrad G, long long s1, long long s2) {
  typedef Tl<NC> TL;
  constexpr int H = TL::H, HV = TL::HV, FH = TL::FH, FS = TL::FS;
  constexpr int PT = NC + 2, PP = PT * PT;
  constexpr int LPR = NC / 4, BS = grad_tile_block(NC);
  constexpr int RPP = BS / LPR, IT = NC * NC / RPP;   // rows per pass, passes
  constexpr int NG = 6 * FS / 2, GIT = (NG + BS - 1) / BS;   // ghost pairs, per thread
  __shared__ __attribute__((aligned(16))) double T[PT * PP];

  const DenseClip c = clips[blockIdx.x];
  const double* __restrict__ box = boxp(L, iv, c.box);
  const int q = threadIdx.x % LPR, rs = threadIdx.x / LPR;
  // the lane's row of pass t: (j, k), 1-based
  auto row_of = [&](int t, int& j, int& k) {
    const int r = rs + t * RPP;
    if (NC == 16) {
      j = tile_row16(r % NC) + 1;
      k = r / NC + 1;
    } else {
      j = r % NC + 1;
      k = r / NC + 1;
    }
  };

  // every global load first: the interior (two 16-B loads per row and lane) ...
  d2 u[IT], v[IT], gh[GIT];
#pragma unroll
  for (int t = 0; t < IT; t++) {
    int j, k;
    row_of(t, j, k);
    const int o = 2 * q + H * ((j - 1) + NC * (k - 1));
    const int ea = (1 + j + k) & 1;   // colour of cells 4q+1 and 4q+3
    u[t] = ld2(box + ea * HV + o);
    v[t] = ld2(box + (ea ^ 1) * HV + o);
  }
  // ... and the ghost faces: pair p = two ghosts of one colour, tangential
  // (a, cc) and (a+2, cc), of face nb
#pragma unroll
  for (int t = 0; t < GIT; t++) {
    const int p = threadIdx.x + t * BS;
    if (NG % BS == 0 || p < NG) gh[t] = ld2(box + 2 * HV + 2 * p);
  }
#pragma unroll
  for (int t = 0; t < IT; t++) {
    int j, k;
    row_of(t, j, k);
    double* w = T + 4 * q + 1 + PT * j + PP * k;
    w[0] = u[t].x;
    w[1] = v[t].x;
    w[2] = u[t].y;
    w[3] = v[t].y;
  }
#pragma unroll
  for (int t = 0; t < GIT; t++) {
    const int p = threadIdx.x + t * BS;
    if (NG % BS == 0 || p < NG) {
      // slot 2p of the faces: face, colour half, row cc, first half-index
      const int s = 2 * p, nb = s / FS, r1 = s % FS, e = r1 / FH, r = r1 % FH;
      const int ah = r % H, cc = r / H + 1;
      const int g = (nb & 1) ? NC + 1 : 0;   // (nb is 0-based here: even = the low face)
      const int a = 2 * ah + 1 + ((1 + g + cc + e) & 1);
      const int d = nb >> 1;
      // tile offset of ghost (a, cc) and the step to (a+2, cc)
      const int o = d == 0 ? g + PT * a + PP * cc : d == 1 ? a + PT * g + PP * cc : a + PT * cc + PP * g;
      const int st = d == 0 ? 2 * PT : 2;
      T[o] = gh[t].x;
      T[o + st] = gh[t].y;
    }
  }
  __syncthreads();

  const bool whole = c.j0 == 1 && c.j1 == NC && c.k0 == 1 && c.k1 == NC;
#pragma unroll
  for (int t = 0; t < IT; t++) {
    int j, k;
    row_of(t, j, k);
    if (!whole && (j < c.j0 || j > c.j1 || k < c.k0 || k > c.k1)) continue;
    const long long off = c.off + (long long)(j - c.j0) * s1 + (long long)(k - c.k0) * s2 + 4 * q;
    const double* m = T + 4 * q + PT * j + PP * k;   // cell 4q of the row
    if (G.out[0]) {
      const d2 a = ld2(m), b = ld2(m + 2), e = ld2(m + 4);
      const double f = G.f[0];
      st2(G.out[0] + off, d2{grad_value(b.x, a.x, f), grad_value(b.y, a.y, f)});
      st2(G.out[0] + off + 2, d2{grad_value(e.x, b.x, f), grad_value(e.y, b.y, f)});
    }
#pragma unroll
    for (int d = 1; d < 3; d++) {
      if (!G.out[d]) continue;
      const int step = d == 1 ? PT : PP;
      const d2 la = ld2(m - step), lb = ld2(m - step + 2), le = ld2(m - step + 4);
      const d2 ha = ld2(m + step), hb = ld2(m + step + 2), he = ld2(m + step + 4);
      const double f = G.f[d];
      st2(G.out[d] + off, d2{grad_value(ha.y, la.y, f), grad_value(hb.x, lb.x, f)});
      st2(G.out[d] + off + 2, d2{grad_value(hb.y, lb.y, f), grad_value(he.x, le.x, f)});
    }
  }
}

// Everything else (odd box sizes, 2^3 and 4^3 boxes, partial rows, odd
// offsets, unaligned bases, OMG_DENSE_GENERIC): one cell per thread through
// off_cell, `bpc` workgroups per record.
__global__ void __launch_bounds__(256)
k_dense_grad_cell(LevelView L, int iv, const DenseClip* clips, int bpc, DenseGrad G, long long s1, long long s2) {
  const DenseClip c = clips[blockIdx.x / bpc];
  const int ni = c.i1 - c.i0 + 1, nj = c.j1 - c.j0 + 1, nk = c.k1 - c.k0 + 1;
  const int total = ni * nj * nk;
  const double* box = boxp(L, iv, c.box);
  for (int t = (blockIdx.x % bpc) * 256 + threadIdx.x; t < total; t += bpc * 256) {
    const int di = t % ni, dj = (t / ni) % nj, dk = t / (ni * nj);
    const int i = c.i0 + di, j = c.j0 + dj, k = c.k0 + dk;
    const long long off = c.off + di + (long long)dj * s1 + (long long)dk * s2;
    if (G.out[0]) G.out[0][off] = grad_value(box[off_cell(L, i + 1, j, k)], box[off_cell(L, i - 1, j, k)], G.f[0]);
    if (G.out[1]) G.out[1][off] = grad_value(box[off_cell(L, i, j + 1, k)], box[off_cell(L, i, j - 1, k)], G.f[1]);
    if (G.out[2]) G.out[2][off] = grad_value(box[off_cell(L, i, j, k + 1)], box[off_cell(L, i, j, k - 1)], G.f[2]);
  }
}

void launch_dense_grad_tile(const LevelView& L, int iv, const DenseClip* clips, int n, const DenseGrad& G,
                            long long s1, long long s2, hipStream_t st) {
  if (n <= 0) return;
  if (L.nc == 16) k_dense_grad_tile<16><<<n, grad_tile_block(16), 0, st>>>(L, iv, clips, G, s1, s2);
  else k_dense_grad_tile<8><<<n, grad_tile_block(8), 0, st>>>(L, iv, clips, G, s1, s2);
}

void launch_dense_grad_cell(const LevelView& L, int iv, const DenseClip* clips, int n, const DenseGrad& G,
                            long long s1, long long s2, hipStream_t st) {
  if (n <= 0) return;
  const int bpc = cell_bpc((long long)L.nc * L.nc * L.nc);
  const unsigned grid = (unsigned)((long long)n * bpc);
  k_dense_grad_cell<<<grid, 256, 0, st>>>(L, iv, clips, bpc, G, s1, s2);
}

}  // namespace omg
