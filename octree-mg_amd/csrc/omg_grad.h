// omg_grad.h — what the gradient kernels share (omg_dense_grad.hip,
// omg_boxes_grad.hip): the one function that holds the arithmetic and the LDS
// staging of a stored box with its six ghost faces.
//
// Staging (box sizes 16 and 8).  One workgroup stages the stored box in LDS in
// plain (NC+2)^3 order, T[i + PT*(j + PT*k)] with PT = NC+2 doubles (even:
// every 16-B read of a cell pair 2a, 2a+1 is aligned): both colour halves with
// 16-B loads as k_dense_row does, the six ghost faces with 16-B loads of two
// ghosts of one colour (tangential a and a+2).  All global loads are issued
// before the one barrier.  Then a lane owns the cells i = 4q+1 .. 4q+4 of a
// row (j, k) per pass.
//
// LDS banks (ds_read_b128: groups of 16 lanes, 16-B slots modulo 16 must
// differ inside a group).  At NC = 16 a row's four lanes take the slots
// 9*row + 162*k + {0, 2, 4, 6} (+ a constant per read), so a group is
// conflict-free when its four rows are {a, a+8, b, b+8} with a even and b
// odd; tile_row16() hands the wave's 16 rows of a plane out that way.  At
// NC = 8 the natural order stays (two lanes per row, DESIGN).
#pragma once

#include "omg_device.h"

namespace omg {

typedef double d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ d2 ld2(const double* p) { return *reinterpret_cast<const d2*>(p); }
__device__ __forceinline__ void st2(double* p, d2 v) { *reinterpret_cast<d2*>(p) = v; }

// the one place the arithmetic lives: every kernel gives the same bits
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
struct GradTile {
  typedef Tl<NC> TL;
  static constexpr int H = TL::H, HV = TL::HV, FH = TL::FH, FS = TL::FS;
  static constexpr int PT = NC + 2, PP = PT * PT, NT = PT * PP;   // pitches and doubles of the tile
  static constexpr int LPR = NC / 4, BS = grad_tile_block(NC);
  static constexpr int RPP = BS / LPR, IT = NC * NC / RPP;        // rows per pass, passes
  static constexpr int NG = 6 * FS / 2, GIT = (NG + BS - 1) / BS; // ghost pairs, per thread

  // the lane's quarter of a row
  static __device__ __forceinline__ int quarter() { return threadIdx.x % LPR; }
  // the lane's row of pass t: (j, k), 1-based
  static __device__ __forceinline__ void row_of(int t, int& j, int& k) {
    const int r = threadIdx.x / LPR + t * RPP;
    j = (NC == 16 ? tile_row16(r % NC) : r % NC) + 1;
    k = r / NC + 1;
  }

  // the stored box -> T, and the barrier
  static __device__ __forceinline__ void stage(double* T, const double* __restrict__ box) {
    const int q = quarter();
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
  }
};

}  // namespace omg
