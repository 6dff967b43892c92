// omg_boxes_grad.hip — omg_get_boxes_grad: the gradient of a variable over a
// list of boxes, on any levels, as blocks of up to three component pools in
// the caller's device memory.  With o = rec.off + (i-1) + (j-1)*s1 + (k-1)*s2
// (the slot of cell (i,j,k) of a record's block, as omg_boxes.hip),
//   cell-centred  out[d][o] = (cc(+1 in d) - cc(-1 in d)) * f_d   1 <= i,j,k <= nc,
//                 f_d = 0.5*scale/dr_d: omg_get_dense_grad's values;
//   face-centred  out[d][o] = (cc(+1 in d) - cc) * f_d,  f_d = scale/dr_d,
//                 the index along d from 0 to nc, the two others from 1 to nc:
//                 the face between the cells i and i+1 at cell i's slot, so
//                 face 0 lies one element (row, plane) below the interior.
// One subtraction and one multiplication per value (grad_value, omg_grad.h:
// every kernel here and in omg_dense_grad.hip calls it; the library builds
// with -ffp-contract=off).  Only the stored box and its six ghost faces are
// read; every store is a plain C++ (vector) store.
//
// Tile kernel (box sizes 16 and 8).  One workgroup per record stages the
// stored box in LDS with GradTile::stage (omg_grad.h: the staging of
// k_dense_grad_tile, all global loads before the one barrier), then a lane
// owns the cells i = 4q+1 .. 4q+4 of a row (j, k) per pass, rows handed out by
// tile_row16.  It reads the row's cells 4q .. 4q+5 as three 16-B LDS reads
// and, per component y / z, the same three pairs of the rows j-1, j+1 /
// k-1, k+1 (cell centring) or of the row j+1 / k+1 (face centring), and
// writes its four values as two 16-B stores, or as four 8-B stores (W8) when
// a base, a box_off or a stride is odd.
// The extra layer of face centring: the x face 0 of a row is one 8-B store of
// the lane q = 0; the y row 0 of a plane is written by the lanes of row
// j = 1 (four values from one more triple of reads, the row j-1 = 0), the z
// plane 0 by the lanes of plane k = 1 (a whole wave at 16^3).
// LDS banks: every 16-B read is at m + const with m = T + 4q + PT*j + PP*k,
// the address pattern of k_dense_grad_tile, for which omg_grad.h shows that
// the tile_row16 assignment is conflict-free; the constants used here (0, 2,
// 4, +-PT, +-PP plus those) are the ones used there.  The extra reads of row
// 0 / plane 0 are made by a subset of those lanes at the same pattern: a
// subset of a conflict-free group is conflict-free.
//
// Per-cell kernel: any box size, through off_cell, `bpc` workgroups per
// record; also short lists and everything under OMG_BOXES_GENERIC=1.  Both
// kernels give the same bits.
#include "omg_grad.h"
#include "omg_kernels.h"

namespace omg {

// four consecutive values at p: two 16-B stores (p 16-B aligned) or four 8-B ones
template <bool W8>
__device__ __forceinline__ void put4(double* p, double v0, double v1, double v2, double v3) {
  if (W8) {
    p[0] = v0;
    p[1] = v1;
    p[2] = v2;
    p[3] = v3;
  } else {
    st2(p, d2{v0, v1});
    st2(p + 2, d2{v2, v3});
  }
}

template <int NC, bool FACE, bool W8>
__global__ void __launch_bounds__(grad_tile_block(NC))
k_boxes_grad_tile(LevelView L, int iv, const BoxRec* __restrict__ recs, DenseGrad G, long long s1, long long s2) {
  typedef GradTile<NC> GT;
  constexpr int PT = GT::PT, PP = GT::PP, IT = GT::IT;
  __shared__ __attribute__((aligned(16))) double T[GT::NT];

  const BoxRec rec = recs[blockIdx.x];
  const int q = GT::quarter();
  GT::stage(T, boxp(L, iv, rec.box));

#pragma unroll
  for (int t = 0; t < IT; t++) {
    int j, k;
    GT::row_of(t, j, k);
    const long long off = rec.off + (long long)(j - 1) * s1 + (long long)(k - 1) * s2 + 4 * q;
    const double* m = T + 4 * q + PT * j + PP * k;   // cell 4q of the row
    const d2 a = ld2(m), b = ld2(m + 2), e = ld2(m + 4);
    if (G.out[0]) {
      const double f = G.f[0];
      if (FACE) {
        put4<W8>(G.out[0] + off, grad_value(b.x, a.y, f), grad_value(b.y, b.x, f), grad_value(e.x, b.y, f),
                 grad_value(e.y, e.x, f));
        if (q == 0) G.out[0][off - 1] = grad_value(a.y, a.x, f);   // the face i = 0
      } else {
        put4<W8>(G.out[0] + off, grad_value(b.x, a.x, f), grad_value(b.y, a.y, f), grad_value(e.x, b.x, f),
                 grad_value(e.y, b.y, f));
      }
    }
#pragma unroll
    for (int d = 1; d < 3; d++) {
      if (!G.out[d]) continue;
      const int step = d == 1 ? PT : PP;
      const double f = G.f[d];
      const d2 ha = ld2(m + step), hb = ld2(m + step + 2), he = ld2(m + step + 4);
      if (FACE) {
        put4<W8>(G.out[d] + off, grad_value(ha.y, a.y, f), grad_value(hb.x, b.x, f), grad_value(hb.y, b.y, f),
                 grad_value(he.x, e.x, f));
        if ((d == 1 ? j : k) == 1) {   // the row j = 0 / the plane k = 0
          const d2 la = ld2(m - step), lb = ld2(m - step + 2), le = ld2(m - step + 4);
          put4<W8>(G.out[d] + (off - (d == 1 ? s1 : s2)), grad_value(a.y, la.y, f), grad_value(b.x, lb.x, f),
                   grad_value(b.y, lb.y, f), grad_value(e.x, le.x, f));
        }
      } else {
        const d2 la = ld2(m - step), lb = ld2(m - step + 2), le = ld2(m - step + 4);
        put4<W8>(G.out[d] + off, grad_value(ha.y, la.y, f), grad_value(hb.x, lb.x, f), grad_value(hb.y, lb.y, f),
                 grad_value(he.x, le.x, f));
      }
    }
  }
}

// Any box size: one point (i,j,k) of the record per thread, 1 .. nc for cell
// centring, 0 .. nc for face centring (component d is defined where the two
// other indices are >= 1).
template <bool FACE>
__global__ void __launch_bounds__(256)
k_boxes_grad_cell(LevelView L, int iv, const BoxRec* recs, int bpc, DenseGrad G, long long s1, long long s2) {
  const BoxRec rec = recs[blockIdx.x / bpc];
  const int nc = L.nc, lo = FACE ? 0 : 1, n = nc + 1 - lo, total = n * n * n;
  const double* box = boxp(L, iv, rec.box);
  for (int t = (blockIdx.x % bpc) * 256 + threadIdx.x; t < total; t += bpc * 256) {
    const int i = t % n + lo, j = (t / n) % n + lo, k = t / (n * n) + lo;
    const long long off = rec.off + (i - 1) + (long long)(j - 1) * s1 + (long long)(k - 1) * s2;
    if (FACE) {
      if (G.out[0] && j && k)
        G.out[0][off] = grad_value(box[off_cell(L, i + 1, j, k)], box[off_cell(L, i, j, k)], G.f[0]);
      if (G.out[1] && i && k)
        G.out[1][off] = grad_value(box[off_cell(L, i, j + 1, k)], box[off_cell(L, i, j, k)], G.f[1]);
      if (G.out[2] && i && j)
        G.out[2][off] = grad_value(box[off_cell(L, i, j, k + 1)], box[off_cell(L, i, j, k)], G.f[2]);
    } else {
      if (G.out[0]) G.out[0][off] = grad_value(box[off_cell(L, i + 1, j, k)], box[off_cell(L, i - 1, j, k)], G.f[0]);
      if (G.out[1]) G.out[1][off] = grad_value(box[off_cell(L, i, j + 1, k)], box[off_cell(L, i, j - 1, k)], G.f[1]);
      if (G.out[2]) G.out[2][off] = grad_value(box[off_cell(L, i, j, k + 1)], box[off_cell(L, i, j, k - 1)], G.f[2]);
    }
  }
}

template <int NC>
static void launch_grad_tile_nc(const LevelView& L, int iv, const BoxRec* recs, int n, const DenseGrad& G,
                                long long s1, long long s2, bool face, bool w8, hipStream_t st) {
  constexpr int BS = grad_tile_block(NC);
  if (face) {
    if (w8) k_boxes_grad_tile<NC, true, true><<<n, BS, 0, st>>>(L, iv, recs, G, s1, s2);
    else k_boxes_grad_tile<NC, true, false><<<n, BS, 0, st>>>(L, iv, recs, G, s1, s2);
  } else {
    if (w8) k_boxes_grad_tile<NC, false, true><<<n, BS, 0, st>>>(L, iv, recs, G, s1, s2);
    else k_boxes_grad_tile<NC, false, false><<<n, BS, 0, st>>>(L, iv, recs, G, s1, s2);
  }
}

void launch_boxes_grad_tile(const LevelView& L, int iv, const BoxRec* recs, int n, const DenseGrad& G, long long s1,
                            long long s2, bool face, bool w8, hipStream_t st) {
  if (n <= 0) return;
  if (L.nc == 16) launch_grad_tile_nc<16>(L, iv, recs, n, G, s1, s2, face, w8, st);
  else launch_grad_tile_nc<8>(L, iv, recs, n, G, s1, s2, face, w8, st);
}

void launch_boxes_grad_cell(const LevelView& L, int iv, const BoxRec* recs, int n, const DenseGrad& G, long long s1,
                            long long s2, bool face, hipStream_t st) {
  if (n <= 0) return;
  const long long m = L.nc + (face ? 1 : 0);
  const int bpc = cell_bpc(m * m * m);
  const unsigned grid = (unsigned)((long long)n * bpc);
  if (face) k_boxes_grad_cell<true><<<grid, 256, 0, st>>>(L, iv, recs, bpc, G, s1, s2);
  else k_boxes_grad_cell<false><<<grid, 256, 0, st>>>(L, iv, recs, bpc, G, s1, s2);
}

}  // namespace omg
