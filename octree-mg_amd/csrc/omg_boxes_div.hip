// omg_boxes_div.hip — omg_put_boxes_div: the divergence of a vector field
// whose components lie as blocks in up to three pools of the caller's device
// memory, written into variable iv of a list of boxes on any levels.  With
// o = rec.off + (i-1) + (j-1)*s1 + (k-1)*s2 (the slot of cell (i,j,k) of a
// record's block, as omg_boxes.hip) and e_d the step 1, s1, s2 along d,
//   cell-centred  t_d = (V_d[o + e_d] - V_d[o - e_d]) * f_d,  f_d = 0.5*scale/dr_d;
//   face-centred  t_d = (V_d[o] - V_d[o - e_d]) * f_d,        f_d = scale/dr_d,
//                 V_d[o] the value on the face between the cells i and i+1
//                 along d: the layout omg_get_boxes_grad writes;
// and cell (i,j,k), 1 <= i,j,k <= nc, becomes the sum of the t_d of the
// non-null pools in the order x, y, z: (t_x + t_y) + t_z, one term alone is
// itself (div_value below: every kernel here calls it; the library builds
// with -ffp-contract=off).  Of a pool only these elements are read: the
// interior and, along d, the index 0 (both centrings) and nc+1 (cells).  The
// pools are read-only; the face-ghost slots of the stored box are not written.
//
// Tile kernel (box sizes 16 and 8).  One workgroup per record, no LDS: a lane
// owns the cells i = 4q+1 .. 4q+4 of a row (j, k) per pass, rows in their
// natural order.  It reads the pools from global memory, y and z as four
// values of the rows j-1 (, j+1) / k-1 (, k+1) and of its own row (faces), x
// as the values 4q .. 4q+5 (cells) or 4q .. 4q+4 (faces) of its own row:
// 16-B loads of the aligned pairs (4q+1, 4q+2), (4q+3, 4q+4) and 8-B loads of
// the odd ends when every base, box_off and stride is even, the parity rule
// of omg_boxes.hip with a = 0 for every row; 8-B loads throughout (W8)
// otherwise.  Its four sums are two same-colour pairs of the stored box, the
// cells 4q+1, 4q+3 and 4q+2, 4q+4 (the two 16-B loads of GradTile::stage,
// omg_grad.h, turned round): two 16-B stores, and the lanes of a wave, which
// hold 16 / 32 consecutive rows, write 1 KiB of consecutive addresses in each
// colour half.  All loads of all passes of a lane are issued before its
// first store.
//
// Per-cell kernel: any box size, through off_int (off_cell's interior part),
// `bpc` workgroups per record.  It measured faster than or equal to the tile
// kernel at every list length, so the routing sends every list
// to it and the tile kernel runs under OMG_BOXES_TILE=1 only.  Both kernels
// give the same bits.
#include "omg_grad.h"
#include "omg_kernels.h"

namespace omg {

// the one place the arithmetic lives: every kernel gives the same bits.
// tx, ty, tz: the terms (hi - lo) * f of the components that are present.
__device__ __forceinline__ double div_value(bool hx, bool hy, bool hz, double tx, double ty, double tz) {
  if (hx) {
    if (hy) return hz ? (tx + ty) + tz : tx + ty;
    return hz ? tx + tz : tx;
  }
  if (hy) return hz ? ty + tz : ty;
  return tz;
}

// four consecutive values at p: two 16-B loads (p 16-B aligned) or four 8-B ones
template <bool W8>
__device__ __forceinline__ void get4(const double* p, double* v) {
  if (W8) {
    v[0] = p[0];
    v[1] = p[1];
    v[2] = p[2];
    v[3] = p[3];
  } else {
    const d2 a = ld2(p), b = ld2(p + 2);
    v[0] = a.x;
    v[1] = a.y;
    v[2] = b.x;
    v[3] = b.y;
  }
}

template <int NC, bool FACE, bool W8>
__global__ void __launch_bounds__(grad_tile_block(NC))
k_boxes_div_tile(LevelView L, int iv, const BoxRec* __restrict__ recs, BoxDiv G, long long s1, long long s2) {
  typedef Tl<NC> TL;
  constexpr int LPR = NC / 4, BS = grad_tile_block(NC), RPP = BS / LPR, IT = NC * NC / RPP;
  const BoxRec rec = recs[blockIdx.x];
  double* __restrict__ box = boxp(L, iv, rec.box);
  const int q = threadIdx.x % LPR;
  const bool hx = G.in[0] != nullptr, hy = G.in[1] != nullptr, hz = G.in[2] != nullptr;

  // every load first: lo[d] the four lower values, hi[d] the four upper ones
  // (x: xs holds the values 4q .. 4q+5 of the row, the last unused for faces)
  double xs[IT][6], lo[IT][2][4], hi[IT][2][4];
#pragma unroll
  for (int t = 0; t < IT; t++) {
    const int r = threadIdx.x / LPR + t * RPP, j = r % NC, k = r / NC;   // (0-based)
    const long long off = rec.off + (long long)j * s1 + (long long)k * s2 + 4 * q;
    if (hx) {
      const double* p = G.in[0] + off;
      xs[t][0] = p[-1];
      get4<W8>(p, &xs[t][1]);
      if (!FACE) xs[t][5] = p[4];
    }
#pragma unroll
    for (int d = 1; d < 3; d++) {
      if (!G.in[d]) continue;
      const long long step = d == 1 ? s1 : s2;
      const double* p = G.in[d] + off;
      get4<W8>(p - step, lo[t][d - 1]);
      get4<W8>(FACE ? p : p + step, hi[t][d - 1]);
    }
  }
#pragma unroll
  for (int t = 0; t < IT; t++) {
    const int r = threadIdx.x / LPR + t * RPP, j = r % NC, k = r / NC;
    double v[4];
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const double tx = hx ? grad_value(xs[t][FACE ? a + 1 : a + 2], xs[t][a], G.f[0]) : 0.0;
      const double ty = hy ? grad_value(hi[t][0][a], lo[t][0][a], G.f[1]) : 0.0;
      const double tz = hz ? grad_value(hi[t][1][a], lo[t][1][a], G.f[2]) : 0.0;
      v[a] = div_value(hx, hy, hz, tx, ty, tz);
    }
    // cells 4q+1 and 4q+3 have the colour (1 + j1 + k1) & 1 = (j + k + 1) & 1
    const int o = 2 * q + TL::H * (j + NC * k), ea = (1 + j + k) & 1;
    st2(box + ea * TL::HV + o, d2{v[0], v[2]});
    st2(box + (ea ^ 1) * TL::HV + o, d2{v[1], v[3]});
  }
}

// Any box size: one interior cell (i,j,k) of the record per thread.
template <bool FACE>
__global__ void __launch_bounds__(256)
k_boxes_div_cell(LevelView L, int iv, const BoxRec* recs, int bpc, BoxDiv G, long long s1, long long s2) {
  const BoxRec rec = recs[blockIdx.x / bpc];
  const int nc = L.nc, total = nc * nc * nc;
  double* box = boxp(L, iv, rec.box);
  const bool hx = G.in[0] != nullptr, hy = G.in[1] != nullptr, hz = G.in[2] != nullptr;
  for (int t = (blockIdx.x % bpc) * 256 + threadIdx.x; t < total; t += bpc * 256) {
    const int i = t % nc + 1, j = (t / nc) % nc + 1, k = t / (nc * nc) + 1;
    const long long off = rec.off + (i - 1) + (long long)(j - 1) * s1 + (long long)(k - 1) * s2;
    double tm[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int d = 0; d < 3; d++) {
      if (!G.in[d]) continue;
      const long long step = d == 0 ? 1 : d == 1 ? s1 : s2;
      const double* p = G.in[d] + off;
      tm[d] = grad_value(FACE ? p[0] : p[step], p[-step], G.f[d]);
    }
    box[off_int(L, i, j, k)] = div_value(hx, hy, hz, tm[0], tm[1], tm[2]);
  }
}

template <int NC>
static void launch_div_tile_nc(const LevelView& L, int iv, const BoxRec* recs, int n, const BoxDiv& G, long long s1,
                               long long s2, bool face, bool w8, hipStream_t st) {
  constexpr int BS = grad_tile_block(NC);
  if (face) {
    if (w8) k_boxes_div_tile<NC, true, true><<<n, BS, 0, st>>>(L, iv, recs, G, s1, s2);
    else k_boxes_div_tile<NC, true, false><<<n, BS, 0, st>>>(L, iv, recs, G, s1, s2);
  } else {
    if (w8) k_boxes_div_tile<NC, false, true><<<n, BS, 0, st>>>(L, iv, recs, G, s1, s2);
    else k_boxes_div_tile<NC, false, false><<<n, BS, 0, st>>>(L, iv, recs, G, s1, s2);
  }
}

void launch_boxes_div_tile(const LevelView& L, int iv, const BoxRec* recs, int n, const BoxDiv& G, long long s1,
                           long long s2, bool face, bool w8, hipStream_t st) {
  if (n <= 0) return;
  if (L.nc == 16) launch_div_tile_nc<16>(L, iv, recs, n, G, s1, s2, face, w8, st);
  else launch_div_tile_nc<8>(L, iv, recs, n, G, s1, s2, face, w8, st);
}

void launch_boxes_div_cell(const LevelView& L, int iv, const BoxRec* recs, int n, const BoxDiv& G, long long s1,
                           long long s2, bool face, hipStream_t st) {
  if (n <= 0) return;
  const int bpc = cell_bpc((long long)L.nc * L.nc * L.nc);
  const unsigned grid = (unsigned)((long long)n * bpc);
  if (face) k_boxes_div_cell<true><<<grid, 256, 0, st>>>(L, iv, recs, bpc, G, s1, s2);
  else k_boxes_div_cell<false><<<grid, 256, 0, st>>>(L, iv, recs, bpc, G, s1, s2);
}

}  // namespace omg
