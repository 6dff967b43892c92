// omg_boxes_flux.hip — omg_get_boxes_flux: omg_get_boxes_grad's values, each
// component optionally weighted by a coefficient variable and optionally
// added to what the caller's pool holds.  With g = grad_value(hi, lo, f_d), the
// gradient's value of an element (omg_boxes_grad.hip: the same elements, the
// same f_d, the same bits),
//   no coefficient      v = g
//   face-centred        v = c * g,  c = ((2 * a_lo) * a_hi) / (a_lo + a_hi): the
//                       harmonic mean of the coefficient in the face's two
//                       cells, the weight of the operators with a cell
//                       coefficient (aop_value, omg_device.h), evaluated left
//                       to right; at the faces 0 and nc along d it reads the
//                       coefficient's face ghosts as they stand
//   cell-centred        v = a(i,j,k) * g
//   accumulate          out[d][o] = out[d][o] + v, else out[d][o] = v.
// flux_value holds the arithmetic and every kernel here calls it; the library
// builds with -ffp-contract=off, so every operation is rounded once.  Every
// store is a plain C++ (vector) store.
//
// Tile kernel (box sizes 16 and 8).  The variable is staged and read exactly
// as k_boxes_grad_tile does (GradTile::stage, rows by tile_row16, the same
// 16-B LDS reads: its bank argument holds unchanged).  The coefficient is not
// staged: a second tile of 46.7 KB at 16^3 does not fit beside the first in
// the 64 KiB a workgroup may hold statically, and three distinct coefficients
// fit in no case.  A lane loads the coefficient of its four cells of a row
// straight from the colour-split stored box, as two 16-B loads (coef_row4:
// cells 4q+1, 4q+3 of one colour and 4q+2, 4q+4 of the other; a ghost row of
// a y or z face is split the same way), and the cells 0 and 4q+5 of the x
// direction as 8-B loads.  No LDS and no new LDS read pattern is added; the
// loads of a workgroup cover whole 64-B lines of the stored box.
// Accumulating, the four elements of a put4 are loaded first, by two 16-B
// loads, or four 8-B ones under W8.
//
// Per-cell kernel: k_boxes_grad_cell's structure, any box size.  Both kernels
// give the same bits.
#include "omg_grad.h"
#include "omg_kernels.h"

namespace omg {

// the one place the arithmetic lives.  a_lo, a_hi: the coefficient in the two
// cells of a face (FACE), or a_lo the cell's own; coef = false: no weight
template <bool FACE>
__device__ __forceinline__ double flux_value(double hi, double lo, double f, bool coef, double a_lo, double a_hi) {
  const double g = grad_value(hi, lo, f);
  if (!coef) return g;
  const double c = FACE ? ((2.0 * a_lo) * a_hi) / (a_lo + a_hi) : a_lo;
  return c * g;
}

template <bool ACC>
__device__ __forceinline__ void flux_put(double* p, double v) {
  *p = ACC ? *p + v : v;
}

// four consecutive values at p: put4's stores, after loads of the same width
template <bool W8, bool ACC>
__device__ __forceinline__ void flux_put4(double* p, double v0, double v1, double v2, double v3) {
  if (!ACC) {
    if (W8) {
      p[0] = v0;
      p[1] = v1;
      p[2] = v2;
      p[3] = v3;
    } else {
      st2(p, d2{v0, v1});
      st2(p + 2, d2{v2, v3});
    }
  } else if (W8) {
    const double o0 = p[0], o1 = p[1], o2 = p[2], o3 = p[3];
    p[0] = o0 + v0;
    p[1] = o1 + v1;
    p[2] = o2 + v2;
    p[3] = o3 + v3;
  } else {
    const d2 a = ld2(p), b = ld2(p + 2);
    st2(p, d2{a.x + v0, a.y + v1});
    st2(p + 2, d2{b.x + v2, b.y + v3});
  }
}

struct D4 {
  double c[4];
};

// The cells 4q+1 .. 4q+4 of row (j, k) of a stored box, 0 <= j, k <= NC+1 and
// not both on a ghost layer: two 16-B loads, of the cells 4q+1, 4q+3 and of
// the cells 4q+2, 4q+4 (interior rows: GradTile::stage's loads; a ghost row of
// face nb: the colour halves of that face, tangential (i, the other index)).
template <int NC>
__device__ __forceinline__ D4 coef_row4(const double* __restrict__ box, int q, int j, int k) {
  typedef Tl<NC> TL;
  int o, half, e;   // offset of the colour-0 pair, distance of the colour halves, colour of cell 4q+1
  if (j == 0 || j == NC + 1) {
    o = 2 * TL::HV + (j ? 3 : 2) * TL::FS + 2 * q + TL::H * (k - 1);
    half = TL::FH;
    e = (j + 1 + k) & 1;
  } else if (k == 0 || k == NC + 1) {
    o = 2 * TL::HV + (k ? 5 : 4) * TL::FS + 2 * q + TL::H * (j - 1);
    half = TL::FH;
    e = (k + 1 + j) & 1;
  } else {
    o = 2 * q + TL::H * ((j - 1) + NC * (k - 1));
    half = TL::HV;
    e = (1 + j + k) & 1;
  }
  const d2 u = ld2(box + e * half + o), v = ld2(box + (e ^ 1) * half + o);
  return D4{{u.x, v.x, u.y, v.y}};
}

template <int NC, bool FACE, bool W8, bool ACC>
__global__ void __launch_bounds__(grad_tile_block(NC))
k_boxes_flux_tile(LevelView L, int iv, const BoxRec* __restrict__ recs, DenseGrad G, FluxCoef K, long long s1,
                  long long s2) {
  typedef GradTile<NC> GT;
  typedef Tl<NC> TL;
  constexpr int PT = GT::PT, PP = GT::PP, IT = GT::IT;
  __shared__ __attribute__((aligned(16))) double T[GT::NT];

  const BoxRec rec = recs[blockIdx.x];
  const int q = GT::quarter();
  GT::stage(T, boxp(L, iv, rec.box));
  const double* A[3];
#pragma unroll
  for (int d = 0; d < 3; d++) A[d] = K.iv[d] ? boxp(L, K.iv[d], rec.box) : nullptr;

#pragma unroll
  for (int t = 0; t < IT; t++) {
    int j, k;
    GT::row_of(t, j, k);
    const long long off = rec.off + (long long)(j - 1) * s1 + (long long)(k - 1) * s2 + 4 * q;
    const double* m = T + 4 * q + PT * j + PP * k;   // cell 4q of the row
    const d2 a = ld2(m), b = ld2(m + 2), e = ld2(m + 4);
    if (G.out[0]) {
      const double f = G.f[0];
      const bool w = A[0] != nullptr;
      D4 c{};
      if (w) c = coef_row4<NC>(A[0], q, j, k);
      if (FACE) {
        const double cn = w ? A[0][TL::ocell(4 * q + 5, j, k)] : 0.0;
        flux_put4<W8, ACC>(G.out[0] + off, flux_value<true>(b.x, a.y, f, w, c.c[0], c.c[1]),
                           flux_value<true>(b.y, b.x, f, w, c.c[1], c.c[2]),
                           flux_value<true>(e.x, b.y, f, w, c.c[2], c.c[3]),
                           flux_value<true>(e.y, e.x, f, w, c.c[3], cn));
        if (q == 0) {   // the face i = 0
          const double c0 = w ? A[0][TL::ocell(0, j, k)] : 0.0;
          flux_put<ACC>(G.out[0] + off - 1, flux_value<true>(a.y, a.x, f, w, c0, c.c[0]));
        }
      } else {
        flux_put4<W8, ACC>(G.out[0] + off, flux_value<false>(b.x, a.x, f, w, c.c[0], 0.0),
                           flux_value<false>(b.y, a.y, f, w, c.c[1], 0.0),
                           flux_value<false>(e.x, b.x, f, w, c.c[2], 0.0),
                           flux_value<false>(e.y, b.y, f, w, c.c[3], 0.0));
      }
    }
#pragma unroll
    for (int d = 1; d < 3; d++) {
      if (!G.out[d]) continue;
      const int step = d == 1 ? PT : PP;
      const double f = G.f[d];
      const bool w = A[d] != nullptr;
      D4 c{}, ch{};
      if (w) c = coef_row4<NC>(A[d], q, j, k);
      const d2 ha = ld2(m + step), hb = ld2(m + step + 2), he = ld2(m + step + 4);
      if (FACE) {
        if (w) ch = d == 1 ? coef_row4<NC>(A[d], q, j + 1, k) : coef_row4<NC>(A[d], q, j, k + 1);
        flux_put4<W8, ACC>(G.out[d] + off, flux_value<true>(ha.y, a.y, f, w, c.c[0], ch.c[0]),
                           flux_value<true>(hb.x, b.x, f, w, c.c[1], ch.c[1]),
                           flux_value<true>(hb.y, b.y, f, w, c.c[2], ch.c[2]),
                           flux_value<true>(he.x, e.x, f, w, c.c[3], ch.c[3]));
        if ((d == 1 ? j : k) == 1) {   // the row j = 0 / the plane k = 0
          const d2 la = ld2(m - step), lb = ld2(m - step + 2), le = ld2(m - step + 4);
          D4 cl{};
          if (w) cl = d == 1 ? coef_row4<NC>(A[d], q, 0, k) : coef_row4<NC>(A[d], q, j, 0);
          flux_put4<W8, ACC>(G.out[d] + (off - (d == 1 ? s1 : s2)), flux_value<true>(a.y, la.y, f, w, cl.c[0], c.c[0]),
                             flux_value<true>(b.x, lb.x, f, w, cl.c[1], c.c[1]),
                             flux_value<true>(b.y, lb.y, f, w, cl.c[2], c.c[2]),
                             flux_value<true>(e.x, le.x, f, w, cl.c[3], c.c[3]));
        }
      } else {
        const d2 la = ld2(m - step), lb = ld2(m - step + 2), le = ld2(m - step + 4);
        flux_put4<W8, ACC>(G.out[d] + off, flux_value<false>(ha.y, la.y, f, w, c.c[0], 0.0),
                           flux_value<false>(hb.x, lb.x, f, w, c.c[1], 0.0),
                           flux_value<false>(hb.y, lb.y, f, w, c.c[2], 0.0),
                           flux_value<false>(he.x, le.x, f, w, c.c[3], 0.0));
      }
    }
  }
}

// Any box size: one point (i,j,k) of the record per thread, as
// k_boxes_grad_cell hands them out.
template <bool FACE, bool ACC>
__global__ void __launch_bounds__(256)
k_boxes_flux_cell(LevelView L, int iv, const BoxRec* recs, int bpc, DenseGrad G, FluxCoef K, long long s1,
                  long long s2) {
  const BoxRec rec = recs[blockIdx.x / bpc];
  const int nc = L.nc, lo = FACE ? 0 : 1, n = nc + 1 - lo, total = n * n * n;
  const double* box = boxp(L, iv, rec.box);
  const double* A[3];
#pragma unroll
  for (int d = 0; d < 3; d++) A[d] = K.iv[d] ? boxp(L, K.iv[d], rec.box) : nullptr;
  for (int t = (blockIdx.x % bpc) * 256 + threadIdx.x; t < total; t += bpc * 256) {
    const int i = t % n + lo, j = (t / n) % n + lo, k = t / (n * n) + lo;
    const long long off = rec.off + (i - 1) + (long long)(j - 1) * s1 + (long long)(k - 1) * s2;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      if (!G.out[d]) continue;
      const int di = d == 0, dj = d == 1, dk = d == 2;
      const bool w = A[d] != nullptr;
      if (FACE) {
        // (component d is defined where the two other indices are >= 1)
        if (!((i || di) && (j || dj) && (k || dk))) continue;
        const int o0 = off_cell(L, i, j, k), o1 = off_cell(L, i + di, j + dj, k + dk);
        flux_put<ACC>(G.out[d] + off,
                      flux_value<true>(box[o1], box[o0], G.f[d], w, w ? A[d][o0] : 0.0, w ? A[d][o1] : 0.0));
      } else {
        const double hi = box[off_cell(L, i + di, j + dj, k + dk)], lw = box[off_cell(L, i - di, j - dj, k - dk)];
        flux_put<ACC>(G.out[d] + off, flux_value<false>(hi, lw, G.f[d], w, w ? A[d][off_int(L, i, j, k)] : 0.0, 0.0));
      }
    }
  }
}

template <int NC, bool FACE, bool W8>
static void launch_flux_tile_acc(const LevelView& L, int iv, const BoxRec* recs, int n, const DenseGrad& G,
                                 const FluxCoef& K, long long s1, long long s2, bool acc, hipStream_t st) {
  constexpr int BS = grad_tile_block(NC);
  if (acc) k_boxes_flux_tile<NC, FACE, W8, true><<<n, BS, 0, st>>>(L, iv, recs, G, K, s1, s2);
  else k_boxes_flux_tile<NC, FACE, W8, false><<<n, BS, 0, st>>>(L, iv, recs, G, K, s1, s2);
}

template <int NC>
static void launch_flux_tile_nc(const LevelView& L, int iv, const BoxRec* recs, int n, const DenseGrad& G,
                                const FluxCoef& K, long long s1, long long s2, bool face, bool w8, bool acc,
                                hipStream_t st) {
  if (face) {
    if (w8) launch_flux_tile_acc<NC, true, true>(L, iv, recs, n, G, K, s1, s2, acc, st);
    else launch_flux_tile_acc<NC, true, false>(L, iv, recs, n, G, K, s1, s2, acc, st);
  } else {
    if (w8) launch_flux_tile_acc<NC, false, true>(L, iv, recs, n, G, K, s1, s2, acc, st);
    else launch_flux_tile_acc<NC, false, false>(L, iv, recs, n, G, K, s1, s2, acc, st);
  }
}

void launch_boxes_flux_tile(const LevelView& L, int iv, const BoxRec* recs, int n, const DenseGrad& G,
                            const FluxCoef& K, long long s1, long long s2, bool face, bool w8, bool acc,
                            hipStream_t st) {
  if (n <= 0) return;
  if (L.nc == 16) launch_flux_tile_nc<16>(L, iv, recs, n, G, K, s1, s2, face, w8, acc, st);
  else launch_flux_tile_nc<8>(L, iv, recs, n, G, K, s1, s2, face, w8, acc, st);
}

void launch_boxes_flux_cell(const LevelView& L, int iv, const BoxRec* recs, int n, const DenseGrad& G,
                            const FluxCoef& K, long long s1, long long s2, bool face, bool acc, hipStream_t st) {
  if (n <= 0) return;
  const long long m = L.nc + (face ? 1 : 0);
  const int bpc = cell_bpc(m * m * m);
  const unsigned grid = (unsigned)((long long)n * bpc);
  if (face) {
    if (acc) k_boxes_flux_cell<true, true><<<grid, 256, 0, st>>>(L, iv, recs, bpc, G, K, s1, s2);
    else k_boxes_flux_cell<true, false><<<grid, 256, 0, st>>>(L, iv, recs, bpc, G, K, s1, s2);
  } else {
    if (acc) k_boxes_flux_cell<false, true><<<grid, 256, 0, st>>>(L, iv, recs, bpc, G, K, s1, s2);
    else k_boxes_flux_cell<false, false><<<grid, 256, 0, st>>>(L, iv, recs, bpc, G, K, s1, s2);
  }
}

}  // namespace omg
