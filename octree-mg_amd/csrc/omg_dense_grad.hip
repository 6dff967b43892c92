// omg_dense_grad.hip — omg_get_dense_grad: the central differences of a
// variable over the stored box and its six ghost faces,
//     g_d(i,j,k) = (cc(+1 in d) - cc(-1 in d)) * f_d,   f_d = 0.5*scale/dr_d,
// written as up to three dense windows [z][y][x] that share the clip records
// of omg_get_dense (DenseClip).  One subtraction and one multiplication per
// value (grad_value, shared by both kernels; the library builds with
// -ffp-contract=off).  Edge and corner ghosts are never needed.
//
// Tile kernel (box sizes 16 and 8, the row conditions of k_dense_row).  One
// workgroup per record stages the stored box in LDS (GradTile, omg_grad.h:
// the layout, the loads before the one barrier, the bank argument and
// tile_row16).  Then a lane owns the cells i = 4q+1 .. 4q+4 of a row (j, k):
// the x component reads the row's cells 4q .. 4q+5 as three 16-B LDS reads,
// the y and z components the same three pairs of rows j-1, j+1 / k-1, k+1,
// and every component goes out as two 16-B stores.  A skipped component is a
// wave-uniform branch.
#include "omg_grad.h"
#include "omg_kernels.h"

namespace omg {

template <int NC>
__global__ void __launch_bounds__(grad_tile_block(NC))
k_dense_grad_tile(LevelView L, int iv, const DenseClip* __restrict__ clips, DenseGrad G, long long s1, long long s2) {
  typedef GradTile<NC> GT;
  constexpr int PT = GT::PT, PP = GT::PP, IT = GT::IT;
  __shared__ __attribute__((aligned(16))) double T[GT::NT];

  const DenseClip c = clips[blockIdx.x];
  const int q = GT::quarter();
  GT::stage(T, boxp(L, iv, c.box));

  const bool whole = c.j0 == 1 && c.j1 == NC && c.k0 == 1 && c.k1 == NC;
#pragma unroll
  for (int t = 0; t < IT; t++) {
    int j, k;
    GT::row_of(t, j, k);
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
