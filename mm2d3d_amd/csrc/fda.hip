// Fourier domain adaptation of the source images (Yang & Soatto, CVPR 2020): the amplitudes of the (2b+1) x (2b+1) lowest
// frequencies of a source image are replaced by a target image's, the source's phases stay; include/mm2d3d.h has the definition.
// Only that band changes, so the result is the source image plus a band-limited correction and no FFT is needed: the partial
// forward DFT and the partial inverse are separable and are taken directly, for any H and W.  A real image's spectrum is
// Hermitian, F[-ky, -kx] = conj(F[ky, kx]), and so is the correction's: only the column frequencies kx in [0, b] are computed.
//   mm_fda_transfer  k_fda_rows: a workgroup takes up to 32 rows of one source or target image-channel.  First their row DFT onto
//                    kx = 0 .. b: a thread owns one kx and FOUR rows (one twiddle read serves four sums), the rows pass through LDS
//                    in chunks of 128 columns (coalesced reads, pitch 129: the row groups of a wave meet distinct banks), x
//                    ascending.  Then, from LDS, these rows' share of the column DFT: a thread per (ky, kx), y ascending,
//                    written as P[image-channel][row tile][ky][kx].  The row spectra never reach memory.
//                    k_fda_finish: one workgroup per (source image, channel).  A thread per (ky, kx) totals both operands'
//                    shares, row tiles ascending; the DC term moved to pixel units where mean / std are given; the amplitude swap
//                    dF = F_src (|F_trg| / |F_src| - 1), or |F_trg| where F_src is exactly 0; sum |dF|^2 over the band (Parseval:
//                    the image-channel's share of mse, in a fixed tree).
//                    k_fda_apply: a workgroup takes eight rows.  First their inverse column transform, a thread per (y, kx):
//                    G[y, kx] = sum_ky dF[ky, kx] e^{+2 pi i ky y / H}, ky ascending, scaled by 1 / HW (kx = 0) or 2 / HW (kx > 0,
//                    which stands for -kx too) - on one workgroup per image-channel this stage alone took 70 us, spread over
//                    the apply pass's workgroups it is hidden.  Then out = src + G[y, 0].re + sum_{kx = 1 .. b} Re(G[y, kx]
//                    e^{+2 pi i kx x / W}), a thread a column of the eight rows: coalesced fp32 reads and writes, kx ascending.
//                    The first workgroup of an image adds its C shares of mse, c ascending.
// Every sum and every twiddle factor is fp64.  Phases are reduced in integers - (k x) mod W, (k y) mod H, kept by adding and
// wrapping - before the table of cos, sin(2 pi r / n), r in [0, n / 2], that each workgroup fills in LDS with sincospi (no
// argument reduction of a large angle anywhere); r > n / 2 reads the mirrored entry.  No atomics of any kind, no workgroup waits
// for another, no host read: the same bits on every call.  Three launches whatever the sizes.
#include "common.h"
#include "rows.h"

namespace {
constexpr int MAXN = 2048;          // H and W: the half table of the larger one holds MAXN / 2 + 1 entries
constexpr int MAXB = 32;            // band
constexpr int MAXC = 4;             // channels
constexpr int TABN = MAXN / 2 + 1;  // 16.4 KB of LDS
constexpr int NT = 256;             // threads of k_fda_rows and k_fda_apply
constexpr int XC = 128;             // columns per staged chunk of k_fda_rows
constexpr int TP = XC + 1;          // ... and its pitch
constexpr int RG = 4;               // rows per thread of k_fda_rows
constexpr int MAXG = 8;             // ... and row groups per workgroup: at most 32 rows
constexpr int STAGE = (MAXG * RG * TP * 4 + 15) / 16;  // double2 words of its staging buffer: a pixel chunk, or NT row spectra of RG rows
constexpr int AR = 8;               // rows per workgroup of k_fda_apply
constexpr int FT = ROWS_FT;         // threads of k_fda_finish
constexpr int MAXIMG = 1 << 20;     // Bs and Bt: the grids stay far below 2^31

// tab[r] = cos, sin(2 pi r / n) for r in [0, n / 2]
template <int NTH>
__device__ __forceinline__ void fill_table(double2* tab, int n) {
  for (int r = threadIdx.x; r <= n / 2; r += NTH) {
    double s, c;
    sincospi((double)(2 * r) / (double)n, &s, &c);
    tab[r] = make_double2(c, s);
  }
}
// cos, sin(2 pi r / n) for r in [0, n)
__device__ __forceinline__ double2 twiddle(const double2* tab, int r, int n) {
  const bool up = 2 * r > n;
  double2 t = tab[up ? n - r : r];
  if (up) t.y = -t.y;
  return t;
}

// P[ic][tile][ky + b][kx] = sum over the tile's rows y of e^{-2 pi i ky y / H} sum_x img[ic][y][x] e^{-2 pi i kx x / W};
// image-channels of src first, then trg's; a tile is G * RG rows
__global__ __launch_bounds__(NT) void k_fda_rows(const float* __restrict__ src, const float* __restrict__ trg, int ns, int H, int W, int b,
                                                  int G, double2* __restrict__ P) {
  __shared__ double2 tabw[TABN], tabh[TABN];
  __shared__ double2 stage[STAGE];  // the pixel chunk [G * RG][TP] as floats, then the row spectra [G * RG][nk]
  float* tile = (float*)stage;
  const int tid = (int)threadIdx.x, ic = (int)blockIdx.x;
  const float* img = ic < ns ? src + (int64_t)ic * H * W : trg + (int64_t)(ic - ns) * H * W;
  const int y0 = (int)blockIdx.y * G * RG;
  const int rows = H - y0 < G * RG ? H - y0 : G * RG;
  const int nk = b + 1, nj = 2 * b + 1, nout = nj * nk;
  fill_table<NT>(tabw, W);
  fill_table<NT>(tabh, H);
  const int g = tid / nk, kx = tid - g * nk;  // a thread owns one kx and RG rows: one twiddle read serves RG sums
  const bool live = g < G;
  double ar[RG], ai[RG];
#pragma unroll
  for (int j = 0; j < RG; j++) ar[j] = 0.0, ai[j] = 0.0;
  int idx = 0;  // (kx x) mod W
  for (int x0 = 0; x0 < W; x0 += XC) {
    const int nc = W - x0 < XC ? W - x0 : XC;
    __syncthreads();  // the tables are filled; the chunk before has been summed
    for (int e = tid; e < G * RG * XC; e += NT) {
      const int r = e / XC, c = e - r * XC;
      // every load is issued, from a clamped address: a load under a condition would be waited for one by one
      const float v = img[(int64_t)(y0 + r < H ? y0 + r : H - 1) * W + (x0 + c < W ? x0 + c : W - 1)];
      tile[r * TP + c] = r < rows && c < nc ? v : 0.f;
    }
    __syncthreads();
    if (live) {
      const float* a = tile + g * RG * TP;
#pragma unroll 2
      for (int c = 0; c < nc; c++) {  // x ascending: the order is part of the result bits
        const double2 t = twiddle(tabw, idx, W);
#pragma unroll
        for (int j = 0; j < RG; j++) {
          const double v = (double)a[j * TP + c];
          ar[j] += v * t.x;
          ai[j] -= v * t.y;
        }
        idx += kx;
        if (idx >= W) idx -= W;
      }
    }
  }
  __syncthreads();  // the last chunk has been read
  if (live) {
#pragma unroll
    for (int j = 0; j < RG; j++) stage[(g * RG + j) * nk + kx] = make_double2(ar[j], ai[j]);  // rows beyond the image: zeros, never read
  }
  __syncthreads();
  double2* Po = P + ((int64_t)ic * gridDim.y + blockIdx.y) * nout;
  for (int o = tid; o < nout; o += NT) {
    const int j = o / nk, k = o - j * nk, ky = j - b;
    const int step = ky < 0 ? ky + H : ky;
    int id = (int)(((int64_t)step * y0) % H);  // (ky y) mod H
    double fr = 0.0, fi = 0.0;
#pragma unroll 2
    for (int r = 0; r < rows; r++) {  // y ascending
      const double2 t = twiddle(tabh, id, H), p = stage[r * nk + k];
      fr += p.x * t.x + p.y * t.y;
      fi += p.y * t.x - p.x * t.y;
      id += step;
      if (id >= H) id -= H;
    }
    Po[o] = make_double2(fr, fi);
  }
}

// dF[sc][ky + b][kx] of the source image-channel sc = blockIdx.x, and its share sum |dF|^2 / (HW)^2 of mse
__global__ __launch_bounds__(FT) void k_fda_finish(const double2* __restrict__ P, int T, int Bs, int Bt, int C, int H, int W, int b,
                                                   const float* __restrict__ mean, const float* __restrict__ std,
                                                   double2* __restrict__ dF, double* __restrict__ msep) {
  __shared__ double red[FT];
  const int tid = (int)threadIdx.x, sc = (int)blockIdx.x;
  const int i = sc / C, c = sc - i * C;
  const int nk = b + 1, nout = (2 * b + 1) * nk;
  const double2* Ps = P + (int64_t)sc * T * nout;
  const double2* Pt = P + ((int64_t)Bs * C + (int64_t)(i % Bt) * C + c) * T * nout;  // source image i takes target image i mod Bt
  const double hw = (double)H * (double)W;
  double e2 = 0.0;
  for (int o = tid; o < nout; o += FT) {
    const int kx = o % nk;
    double sr = 0.0, si = 0.0, tr = 0.0, ti = 0.0;
    for (int t = 0; t < T; t++) {  // row tiles ascending
      const double2 p = Ps[(int64_t)t * nout + o], q = Pt[(int64_t)t * nout + o];
      sr += p.x, si += p.y, tr += q.x, ti += q.y;
    }
    double sd = 1.0;
    if (mean && o == b * nk) {  // the DC term of (pixel - mean) / std, in pixel units: every other term scales by 1 / std on both sides
      sd = (double)std[c];
      const double m = (double)mean[c] * hw;
      sr = sd * sr + m, si = sd * si, tr = sd * tr + m, ti = sd * ti;
    }
    const double at = hypot(tr, ti);
    double dr, di;
    if (sr == 0.0 && si == 0.0) {  // no phase to keep: angle(0) = 0
      dr = at, di = 0.0;
    } else {
      const double f = at / hypot(sr, si) - 1.0;
      dr = sr * f, di = si * f;
    }
    dr /= sd, di /= sd;
    dF[(int64_t)sc * nout + o] = make_double2(dr, di);
    e2 += (kx == 0 ? 1.0 : 2.0) * (dr * dr + di * di);  // kx > 0 stands for -kx too
  }
  const double tot = block_sum<FT>(e2, red);
  if (tid == 0) msep[sc] = tot / (hw * hw);
}

// rows [y0, y0 + AR) of the source image-channel sc = blockIdx.x
__global__ __launch_bounds__(NT) void k_fda_apply(const float* __restrict__ src, const double2* __restrict__ dF,
                                                   const double* __restrict__ msep, int C, int H, int W, int b, float* __restrict__ out,
                                                   float* __restrict__ mse) {
  __shared__ double2 tab[TABN];
  __shared__ double2 tw[AR * (2 * MAXB + 1)];  // [row][ky + b] = cos, sin(2 pi ky y / H)
  __shared__ double2 g[AR * (MAXB + 1)];       // [row][kx]
  const int tid = (int)threadIdx.x, sc = (int)blockIdx.x;
  const int y0 = (int)blockIdx.y * AR;
  const int rows = H - y0 < AR ? H - y0 : AR;
  const int nk = b + 1, nj = 2 * b + 1;
  fill_table<NT>(tab, W);
  for (int e = tid; e < rows * nj; e += NT) {  // the few column twiddles of these rows, as the tables hold them
    const int r = e / nj, ky = e - r * nj - b;
    const int idx = (int)(((int64_t)(ky < 0 ? ky + H : ky) * (y0 + r)) % H);  // (ky y) mod H
    const bool up = 2 * idx > H;
    double s, c;
    sincospi((double)(2 * (up ? H - idx : idx)) / (double)H, &s, &c);
    tw[e] = make_double2(c, up ? -s : s);
  }
  if (blockIdx.y == 0 && tid == 0 && sc % C == 0) {
    double s = 0.0;
    for (int c = 0; c < C; c++) s += msep[sc + c];  // c ascending
    mse[sc / C] = (float)(s / (double)C);
  }
  __syncthreads();
  const double inv = 1.0 / ((double)H * (double)W);
  const double2* d = dF + (int64_t)sc * nj * nk;
  for (int e = tid; e < AR * nk; e += NT) {  // the inverse column transform of these rows
    const int r = e / nk, kx = e - r * nk;
    double gr = 0.0, gi = 0.0;
    if (r < rows) {
#pragma unroll 4
      for (int j = 0; j < nj; j++) {  // ky ascending
        const double2 t = tw[r * nj + j], f = d[j * nk + kx];
        gr += f.x * t.x - f.y * t.y;
        gi += f.x * t.y + f.y * t.x;
      }
    }
    const double s = kx == 0 ? inv : 2.0 * inv;  // kx > 0 stands for -kx too
    g[e] = make_double2(gr * s, gi * s);
  }
  __syncthreads();
  const int64_t base = ((int64_t)sc * H + y0) * W;
  for (int x = tid; x < W; x += NT) {
    double acc[AR];
#pragma unroll
    for (int r = 0; r < AR; r++) acc[r] = g[r * nk].x;
    int idx = 0;  // (kx x) mod W
    for (int kx = 1; kx < nk; kx++) {  // kx ascending
      idx += x;
      if (idx >= W) idx -= W;
      const double2 t = twiddle(tab, idx, W);
#pragma unroll
      for (int r = 0; r < AR; r++) {
        const double2 a = g[r * nk + kx];
        acc[r] += a.x * t.x - a.y * t.y;
      }
    }
    float v[AR];
#pragma unroll
    for (int r = 0; r < AR; r++) v[r] = src[base + (int64_t)(r < rows ? r : rows - 1) * W + x];  // every load is issued (k_fda_rows)
#pragma unroll
    for (int r = 0; r < AR; r++)
      if (r < rows) out[base + (int64_t)r * W + x] = (float)((double)v[r] + acc[r]);
  }
}

struct FdaWs {
  double2 *P, *dF;
  double* msep;
  int groups, T;  // row groups per workgroup and row tiles of k_fda_rows
  size_t bytes;
};
// P [(Bs + Bt) C][T][2 b + 1][b + 1], dF [Bs C][2 b + 1][b + 1], msep [Bs C]
FdaWs fda_ws(void* ws, int Bs, int Bt, int C, int H, int band) {
  const int G = NT / (band + 1) < MAXG ? NT / (band + 1) : MAXG;  // 7 at band 32, else 8
  const int T = (int)mm_cdiv(H, G * RG);
  const size_t p = mm_align((size_t)(Bs + Bt) * C * T * (2 * band + 1) * (band + 1) * sizeof(double2));
  const size_t g = mm_align((size_t)Bs * C * (2 * band + 1) * (band + 1) * sizeof(double2)), m = mm_align((size_t)Bs * C * sizeof(double));
  char* q = (char*)ws;
  return {(double2*)q, (double2*)(q + p), (double*)(q + p + g), G, T, p + g + m};
}

bool fda_sizes_ok(int Bs, int Bt, int C, int H, int W, int band) {
  return Bs >= 1 && Bt >= 1 && Bs <= MAXIMG && Bt <= MAXIMG && C >= 1 && C <= MAXC && H >= 1 && W >= 1 && H <= MAXN && W <= MAXN &&
         band >= 0 && band <= MAXB && 2 * band + 1 <= (H < W ? H : W);
}
}  // namespace

extern "C" {

size_t mm_fda_ws_bytes(int Bs, int Bt, int C, int H, int W, int band) {
  if (!fda_sizes_ok(Bs, Bt, C, H, W, band)) return 0;
  return fda_ws(nullptr, Bs, Bt, C, H, band).bytes;
}

int mm_fda_transfer(const float* src, int Bs, const float* trg, int Bt, int C, int H, int W, int band, const float* mean, const float* std,
                    float* out, float* mse, void* ws, size_t ws_bytes, hipStream_t s) {
  static_assert(NT / (MAXB + 1) >= 1 && STAGE >= NT * RG, "k_fda_rows: a thread per (row group, kx), its RG row spectra staged");
  MM_CHECK_ARG(Bs >= 1 && Bt >= 1 && H >= 1 && W >= 1, "fda_transfer: Bs, Bt, H and W must be at least 1");
  MM_CHECK_ARG(Bs <= MAXIMG && Bt <= MAXIMG, "fda_transfer: Bs and Bt may be at most 2^20");
  MM_CHECK_ARG(C >= 1 && C <= MAXC, "fda_transfer: C must lie in [1, 4]");
  MM_CHECK_ARG(H <= MAXN && W <= MAXN, "fda_transfer: H and W may be at most 2048, what the twiddle tables hold");
  MM_CHECK_ARG(band >= 0 && band <= MAXB, "fda_transfer: band must lie in [0, 32]");
  MM_CHECK_ARG(2 * band + 1 <= (H < W ? H : W), "fda_transfer: 2 * band + 1 must not exceed min(H, W)");
  MM_CHECK_ARG(src && trg && out && mse, "fda_transfer: null src, trg, out or mse");
  MM_CHECK_ARG((mean == nullptr) == (std == nullptr), "fda_transfer: mean and std must be both null or both set");
  MM_CHECK_ARG(ws && ws_bytes >= mm_fda_ws_bytes(Bs, Bt, C, H, W, band), "fda_transfer: workspace missing or too small");
  const FdaWs w = fda_ws(ws, Bs, Bt, C, H, band);
  hipLaunchKernelGGL(k_fda_rows, dim3((unsigned)((Bs + Bt) * C), (unsigned)w.T), dim3(NT), 0, s, src, trg, Bs * C, H, W, band, w.groups, w.P);
  MM_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_fda_finish, dim3((unsigned)(Bs * C)), dim3(FT), 0, s, (const double2*)w.P, w.T, Bs, Bt, C, H, W, band, mean, std, w.dF,
                     w.msep);
  MM_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_fda_apply, dim3((unsigned)(Bs * C), (unsigned)mm_cdiv(H, AR)), dim3(NT), 0, s, src, (const double2*)w.dF,
                     (const double*)w.msep, C, H, W, band, out, mse);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"
