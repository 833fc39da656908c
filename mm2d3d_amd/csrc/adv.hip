// Adversarial alignment in the output space (AdaptSegNet, Tsai et al., CVPR 2018; AdvEnt, Vu et al., CVPR 2019) with a point-wise
// discriminator on the rows [0, P) (source) and [P, N) (target) of a logit matrix x [N, C]; include/mm2d3d.h has the definition.
//   mm_adv_fwd  k_adv_count: a capped grid walks the 128-row tiles (stage_rows of rows.h) and counts the finite rows of each domain
//               (wave_count, block_count).  The row pass needs n_s and n_t BEFORE it can write a row of gx or add a row to the
//               weight gradient - both carry 1 / n - and every row of gx is written once, so the count is a launch of its own.
//               k_adv_rows<H>: a capped grid walks the tiles again.  Each workgroup totals the count partials (sum_partial, a wave
//               per domain).  The parameters stay in global memory: every index into them is uniform over the workgroup, so they
//               arrive by scalar loads through the constant cache and enter the multiply-adds as scalar operands.  (Staged into
//               LDS, every multiply-add had an LDS broadcast read beside it and the 18.7 KB of parameters left room for one
//               two-wave workgroup per CU: 3.72 ms for the 558,080 rows of the benchmark at H = 64, C = 6, in a kernel trace; this
//               way the whole call with its backward and D's optimiser step takes 1.44 ms.)
//               Per tile:
//                 1. a lane owns a row: softmax or self-information u (row_lse) into the tile U, layer 1 in H registers
//                    and into the tile A, layer 2 unit by unit into the tile B, the logit a, the row's
//                    softplus terms, and g = dloss_D / da into gd[row].  An uncounted row leaves zeros in U, A and B and g = 0.
//                 2. the threads share the H x H entries of dW2 as register blocks of H/16 x H/8: an fp32 sum over the tile's rows
//                    ascending of delta2[r][j] * h1[r][k], delta2 = g w3_j lrelu'(h2) formed from B on the fly, then added to the
//                    thread's fp64 accumulators, which are carried across the workgroup's tiles.  Threads [0, H) also own a
//                    column of db2 and dw3, thread 0 db3.
//                 3. the lane again: e2 = da/dz2 from its row of B, e1 = da/dz1 = (W2T e2) lrelu'(h1) in H registers; after a
//                    barrier e1 replaces the row of B; a target row goes on to da/du = W1T e1 and through the input transform and
//                    writes gx over its row of the x tile, any other row writes zeros there.
//                 4. dW1 (H C entries, up to H/4 per thread) and db1 from gd, B and U as in 2; the x tile leaves through
//                    unstage_rows.
//               At the end the workgroup writes its slab: the parameter gradient and three fp64 softplus sums (block_sum), and
//               its two "correct" counts.
//               k_adv_final: 64 quantities per workgroup, four threads each over the slabs in a fixed interleave, joined in a fixed
//               order; the last workgroup totals the loss sums and the counts (sum_partial) and writes stats, count and correct.
//   mm_adv_bwd  k_adv_scale: dx = grad_out[0] * gx + 0 over every row.
// LDS of k_adv_rows: two [128][C | 1] tiles (7.2 KB at C = 6, 33.8 KB at C = 32), two [128][H + 1] tiles (66.6 KB at H = 64; the
// first is [128][C | 1] where that is wider) and gd: 74.2 KB at H = 64, C = 6 - two workgroups, four waves, per CU -, 100.9 KB at
// the limits, 25.1 KB at H = 16, C = 6.  Products and a tile's partial sums are fp32, everything across tiles and workgroups is fp64 in a fixed
// order.  No atomics of any kind, no grid barrier, no workgroup waits for another, no host read: bit-stable run to run.
#include "common.h"
#include "pointpred.h"
#include "rows.h"

namespace {
constexpr int PT = 128;           // rows per tile = threads per workgroup
constexpr int MAXC = MM_PRED_MAXC;
constexpr int ADV_MAX_WG = 512;   // two workgroups per CU of 256; a slab is up to 50.7 KB: half the grid of the other statistics passes
constexpr int MODE_SOFTMAX = 0, MODE_SELFINFO = 1;
constexpr float SLOPE = 0.2f;
constexpr int FQ = 64, FPARTS = 4;  // the finish: quantities per workgroup, threads per quantity
constexpr int NSCAL = 3;            // fp64 scalars behind a slab's gradient: sum_src softplus(a), sum_trg softplus(-a), sum_trg softplus(a)

__host__ __device__ constexpr bool adv_h_ok(int H) { return H == 16 || H == 32 || H == 64; }
__host__ __device__ constexpr int adv_params(int C, int H) { return H * C + H * H + 3 * H + 1; }
// where the parts lie in the flat parameter buffer: W1 [H][C], b1 [H], W2 [H][H], b2 [H], w3 [H], b3
struct AdvOff { int W1, b1, W2, b2, w3, b3; };
__host__ __device__ inline AdvOff adv_off(int C, int H) {
  AdvOff o;
  o.W1 = 0, o.b1 = H * C, o.W2 = o.b1 + H, o.b2 = o.W2 + H * H, o.w3 = o.b2 + H, o.b3 = o.w3 + H;
  return o;
}
// the pitch of the tile A: a row holds h1 [H] and later the C products p_c v_c of the input transform; odd either way
__host__ __device__ constexpr int adv_pitch_a(int C, int H) { return H + 1 > (C | 1) ? H + 1 : (C | 1); }
__host__ __device__ constexpr size_t adv_lds_floats(int C, int H) {
  return 2 * (size_t)PT * (C | 1) + (size_t)PT * adv_pitch_a(C, H) + (size_t)PT * (H + 1) + PT;
}

struct AdvWs { double* psum /*[ADV_MAX_WG][np + NSCAL]*/; long long* pcnt /*[ADV_MAX_WG][2]*/; long long* pcor /*[ADV_MAX_WG][2]*/; size_t bytes; };
inline AdvWs adv_ws(void* ws, int C, int H) {
  const size_t a = mm_align((size_t)ADV_MAX_WG * (adv_params(C, H) + NSCAL) * sizeof(double));
  const size_t b = mm_align((size_t)ADV_MAX_WG * 2 * sizeof(long long));
  return {(double*)ws, (long long*)((char*)ws + a), (long long*)((char*)ws + a + b), a + 2 * b};
}

__device__ __forceinline__ float lrelu(float z) { return z > 0.f ? z : SLOPE * z; }

__global__ __launch_bounds__(PT) void k_adv_count(const float* __restrict__ x, int ld, int64_t N, int64_t P, int C,
                                                   long long* __restrict__ pcnt /*[grid][2]*/) {
  extern __shared__ float tile[];  // [PT][pitch]
  __shared__ unsigned wcnt[2 * PT / 64];
  const int pitch = C | 1;
  const int64_t nt = (N + PT - 1) / PT;
  unsigned wn[2] = {0, 0};  // per wave: every lane holds the wave's counts (N * C < 2^31: below 2^30 rows)
  for (int64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const RowTile tl = row_tile<PT>(t, N);
    __syncthreads();  // the previous tile has been read
    stage_rows<PT>(tile, x + tl.row0 * ld, ld, tl.rows, C, pitch);
    __syncthreads();
    const bool ok = (int)threadIdx.x < tl.rows && row_finite(tile + threadIdx.x * pitch, C);
    const bool trg = tl.row0 + threadIdx.x >= P;
    wn[0] += wave_count(ok && !trg);
    wn[1] += wave_count(ok && trg);
  }
  const long long n = block_count<PT>(wn, wcnt);
  if (threadIdx.x < 2) pcnt[blockIdx.x * 2 + threadIdx.x] = n;
}

template <int H>
__global__ __launch_bounds__(PT) void k_adv_rows(const float* __restrict__ x, int ld, int64_t N, int64_t P, int C, int mode,
                                                  const float* __restrict__ params, const long long* __restrict__ pcnt, int nbc,
                                                  double* __restrict__ psum, long long* __restrict__ pcor, float* __restrict__ gx,
                                                  int ld_g) {
  static_assert(H % 16 == 0 && H <= PT, "a thread owns an H/16 x H/8 block of dW2 and threads [0, H) a bias column");
  constexpr int HP = H + 1;              // odd pitch: the lanes' rows fall on distinct banks
  constexpr int JB = H / 16, KB = H / 8;  // the block of dW2 a thread owns: 16 x 8 blocks = PT threads
  constexpr int NQ1 = H * MAXC / PT;      // entries of dW1 per thread at C = 32
  extern __shared__ float lds[];
  __shared__ double red[PT];
  __shared__ unsigned wcnt[2 * PT / 64];
  __shared__ long long cnt[2];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pc = C | 1, np = adv_params(C, H);
  const AdvOff o = adv_off(C, H);
  // read where they lie: every index below is uniform over the workgroup, so these are scalar loads (file comment)
  const float* __restrict__ par = params;
  float* X = lds;
  float* U = X + PT * pc;
  float* A = U + PT * pc;
  const int ap = adv_pitch_a(C, H);
  float* B = A + PT * ap;
  float* gd = B + PT * HP;
  {  // PT / 64 = 2 waves, a domain each
    const long long s = sum_partial(pcnt, nbc, 2, wave, lane);
    if (lane == 0) cnt[wave] = s;
  }
  __syncthreads();
  const long long n_s = cnt[0], n_t = cnt[1];
  const float ks = n_s > 0 ? (float)(0.5 / (double)n_s) : 0.f, kt = n_t > 0 ? (float)(0.5 / (double)n_t) : 0.f;
  const float kg = n_t > 0 ? (float)(1.0 / (double)n_t) : 0.f;
  const float inv_lnC = 1.f / logf((float)C);

  // what this thread owns of the gradient
  const int j0 = (tid / 8) * JB, k0 = (tid % 8) * KB;
  float w3r[JB], w3s[JB];
#pragma unroll
  for (int jj = 0; jj < JB; jj++) w3r[jj] = par[o.w3 + j0 + jj], w3s[jj] = SLOPE * w3r[jj];
  const float w3c = tid < H ? par[o.w3 + tid] : 0.f, w3cs = SLOPE * w3c;  // the bias column's
  double accW2[JB][KB], accW1[NQ1], accb1 = 0.0, accb2 = 0.0, accw3 = 0.0, accb3 = 0.0;
  int offB[NQ1], offU[NQ1];
  const int nq1 = (H * C + PT - 1) / PT;
#pragma unroll
  for (int jj = 0; jj < JB; jj++)
#pragma unroll
    for (int kk = 0; kk < KB; kk++) accW2[jj][kk] = 0.0;
#pragma unroll
  for (int q = 0; q < NQ1; q++) {
    const int e = tid + q * PT;
    const int k = e < H * C ? e / C : 0, c = e < H * C ? e - k * C : 0;
    accW1[q] = 0.0, offB[q] = k, offU[q] = c;
  }
  double l_src = 0.0, l_trg = 0.0, l_gen = 0.0;  // this lane's rows
  unsigned wc[2] = {0, 0};

  const int64_t ntiles = (N + PT - 1) / PT;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const RowTile tl = row_tile<PT>(t, N);
    __syncthreads();  // the previous tile's sums have been taken and its x tile has left
    stage_rows<PT>(X, x + tl.row0 * ld, ld, tl.rows, C, pc);
    __syncthreads();

    // ---- 1. the lane's row: input transform, the two hidden layers, the logit
    float* xr = X + tid * pc;
    float* ur = U + tid * pc;
    float* ar = A + tid * ap;
    float* br = B + tid * HP;
    const bool trg = tl.row0 + tid >= P;
    bool counted = false;
    float a = 0.f, g = 0.f, gG = 0.f, m = 0.f, inv = 0.f, logs = 0.f;
    if (tid < tl.rows) {
      counted = row_finite(xr, C);
      if (counted) {
        const RowLse r = row_lse(xr, C);
        m = r.m, inv = 1.f / r.s, logs = logf(r.s);
        for (int c = 0; c < C; c++) {
          const float d = xr[c] - m, p = expf(d) * inv;
          ur[c] = mode == MODE_SOFTMAX ? p : (p > 0.f ? -p * (d - logs) * inv_lnC : 0.f);
        }
        float h1[H];
#pragma unroll
        for (int j = 0; j < H; j++) h1[j] = par[o.b1 + j];
        for (int c = 0; c < C; c++) {
          const float uc = ur[c];
#pragma unroll
          for (int j = 0; j < H; j++) h1[j] = fmaf(par[o.W1 + j * C + c], uc, h1[j]);
        }
#pragma unroll
        for (int j = 0; j < H; j++) h1[j] = lrelu(h1[j]), ar[j] = h1[j];
        a = par[o.b3];
#pragma unroll 2
        for (int j = 0; j < H; j++) {
          float z = par[o.b2 + j];
          const float* w = par + o.W2 + j * H;
#pragma unroll
          for (int k = 0; k < H; k++) z = fmaf(w[k], h1[k], z);
          z = lrelu(z);
          br[j] = z;
          a = fmaf(par[o.w3 + j], z, a);
        }
        // softplus(+-a) = max(+-a, 0) + log1p(exp(-|a|)); sigmoid(+-a) from the same exponential
        const float e = expf(-fabsf(a)), l1p = log1pf(e), hi = 1.f / (1.f + e), lo = e / (1.f + e);
        const float sp_pos = fmaxf(a, 0.f) + l1p, sp_neg = fmaxf(-a, 0.f) + l1p;
        const float sig_pos = a >= 0.f ? hi : lo, sig_neg = a >= 0.f ? lo : hi;
        if (trg) {
          l_trg += (double)sp_neg, l_gen += (double)sp_pos;
          g = -kt * sig_neg, gG = kg * sig_pos;
        } else {
          l_src += (double)sp_pos;
          g = ks * sig_pos;
        }
      } else {  // adds +0 to every sum
        for (int c = 0; c < C; c++) ur[c] = 0.f;
#pragma unroll
        for (int j = 0; j < H; j++) ar[j] = 0.f, br[j] = 0.f;
      }
    }
    gd[tid] = g;
    wc[0] += wave_count(counted && !trg && a <= 0.f);
    wc[1] += wave_count(counted && trg && a > 0.f);
    __syncthreads();

    // ---- 2. dW2 += delta2 h1T over the tile's rows ascending; db2, dw3, db3
    {
      float acc[JB][KB];
#pragma unroll
      for (int jj = 0; jj < JB; jj++)
#pragma unroll
        for (int kk = 0; kk < KB; kk++) acc[jj][kk] = 0.f;
      for (int r = 0; r < tl.rows; r++) {
        const float gr = gd[r];
        const float* Br = B + r * HP + j0;
        const float* Ar = A + r * ap + k0;
        float d2[JB], hk[KB];
#pragma unroll
        for (int jj = 0; jj < JB; jj++) d2[jj] = gr * (Br[jj] > 0.f ? w3r[jj] : w3s[jj]);
#pragma unroll
        for (int kk = 0; kk < KB; kk++) hk[kk] = Ar[kk];
#pragma unroll
        for (int jj = 0; jj < JB; jj++)
#pragma unroll
          for (int kk = 0; kk < KB; kk++) acc[jj][kk] = fmaf(d2[jj], hk[kk], acc[jj][kk]);
      }
#pragma unroll
      for (int jj = 0; jj < JB; jj++)
#pragma unroll
        for (int kk = 0; kk < KB; kk++) accW2[jj][kk] += (double)acc[jj][kk];
      if (tid < H) {
        float sb2 = 0.f, sw3 = 0.f, sb3 = 0.f;
        for (int r = 0; r < tl.rows; r++) {
          const float gr = gd[r], hb = B[r * HP + tid];
          sb2 += gr * (hb > 0.f ? w3c : w3cs);
          sw3 = fmaf(gr, hb, sw3);
          sb3 += gr;
        }
        accb2 += (double)sb2, accw3 += (double)sw3, accb3 += (double)sb3;
      }
    }

    // ---- 3. the lane's row again: e1 = da/dz1, then da/du and the input transform for a target row
    float e1[H];
    if (counted) {
#pragma unroll
      for (int k = 0; k < H; k++) e1[k] = 0.f;
#pragma unroll 2
      for (int j = 0; j < H; j++) {
        const float w3j = par[o.w3 + j];
        const float e2 = br[j] > 0.f ? w3j : SLOPE * w3j;
        const float* w = par + o.W2 + j * H;
#pragma unroll
        for (int k = 0; k < H; k++) e1[k] = fmaf(w[k], e2, e1[k]);
      }
#pragma unroll
      for (int k = 0; k < H; k++) e1[k] = ar[k] > 0.f ? e1[k] : SLOPE * e1[k];
    }
    __syncthreads();  // everybody has read A and B
    if (tid < tl.rows) {
      if (counted) {
#pragma unroll
        for (int k = 0; k < H; k++) br[k] = e1[k];
      }
      if (counted && trg) {
        // dL/dx_k = w_k - p_k sum_c w_c, w_c = p_c v_c (0 where p_c = 0), v_c = dL/du_c times the transform's own derivative
        float sum = 0.f;
        for (int c = 0; c < C; c++) {
          float v = 0.f;
#pragma unroll
          for (int k = 0; k < H; k++) v = fmaf(par[o.W1 + k * C + c], e1[k], v);
          const float d = xr[c] - m, p = expf(d) * inv;
          if (mode == MODE_SELFINFO) v *= -((d - logs) + 1.f) * inv_lnC;
          const float w = p > 0.f ? p * v : 0.f;
          ar[c] = w;  // the row of A is free, and wide enough (adv_pitch_a)
          sum += w;
        }
        for (int c = 0; c < C; c++) {
          const float p = expf(xr[c] - m) * inv;
          xr[c] = gG * (ar[c] - p * sum) + 0.f;  // + 0: a zero gradient is +0 whatever the signs
        }
      } else {
        for (int c = 0; c < C; c++) xr[c] = 0.f;
      }
    }
    __syncthreads();

    // ---- 4. dW1 += delta1 uT, db1; the gradient rows leave
    {
      float acc[NQ1];
#pragma unroll
      for (int q = 0; q < NQ1; q++) acc[q] = 0.f;
      for (int r = 0; r < tl.rows; r++) {
        const float gr = gd[r];
        const float* Br = B + r * HP;
        const float* Ur = U + r * pc;
#pragma unroll
        for (int q = 0; q < NQ1; q++)
          if (q < nq1) acc[q] = fmaf(gr * Br[offB[q]], Ur[offU[q]], acc[q]);
      }
#pragma unroll
      for (int q = 0; q < NQ1; q++) accW1[q] += (double)acc[q];
      if (tid < H) {
        float sb1 = 0.f;
        for (int r = 0; r < tl.rows; r++) sb1 += gd[r] * B[r * HP + tid];
        accb1 += (double)sb1;
      }
    }
    unstage_rows<PT>(gx + tl.row0 * ld_g, ld_g, X, tl.rows, C, pc);
  }

  // ---- the workgroup's slab
  double* out = psum + (int64_t)blockIdx.x * (np + NSCAL);
#pragma unroll
  for (int q = 0; q < NQ1; q++)
    if (tid + q * PT < H * C) out[o.W1 + tid + q * PT] = accW1[q];
#pragma unroll
  for (int jj = 0; jj < JB; jj++)
#pragma unroll
    for (int kk = 0; kk < KB; kk++) out[o.W2 + (j0 + jj) * H + k0 + kk] = accW2[jj][kk];
  if (tid < H) out[o.b1 + tid] = accb1, out[o.b2 + tid] = accb2, out[o.w3 + tid] = accw3;
  if (tid == 0) out[o.b3] = accb3;
  const double s0 = block_sum<PT>(l_src, red);
  const double s1 = block_sum<PT>(l_trg, red);
  const double s2 = block_sum<PT>(l_gen, red);
  if (tid == 0) out[np] = s0, out[np + 1] = s1, out[np + 2] = s2;
  const long long nc = block_count<PT>(wc, wcnt);
  if (tid < 2) pcor[blockIdx.x * 2 + tid] = nc;
}

// dparams[np] = the slabs' totals; the last workgroup: stats[2] = loss_D, loss_G; count[2]; correct[2]
__global__ __launch_bounds__(FQ * FPARTS) void k_adv_final(const double* __restrict__ psum, int nb, int np, const long long* __restrict__ pcnt,
                                                           int nbc, const long long* __restrict__ pcor, float* __restrict__ dparams,
                                                           float* __restrict__ stats, int64_t* __restrict__ count,
                                                           int64_t* __restrict__ correct) {
  __shared__ double part[FPARTS][FQ];
  __shared__ double tot[NSCAL];
  __shared__ long long itot[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, K = np + NSCAL;
  if (blockIdx.x + 1 < gridDim.x) {
    const int q = blockIdx.x * FQ + lane;  // consecutive lanes on consecutive quantities of a slab
    double s = 0.0;
    if (q < np)
      for (int i = wave; i < nb; i += FPARTS) s += psum[(int64_t)i * K + q];  // slabs ascending: the order is part of the result bits
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && q < np) dparams[q] = (float)(((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]);
    return;
  }
  for (int q = wave; q < NSCAL + 4; q += FPARTS) {  // uniform per wave
    if (q < NSCAL) {
      const double v = sum_partial(psum, nb, K, np + q, lane);
      if (lane == 0) tot[q] = v;
    } else {
      const int k = q - NSCAL;
      const long long v = k < 2 ? sum_partial(pcnt, nbc, 2, k, lane) : sum_partial(pcor, nb, 2, k - 2, lane);
      if (lane == 0) itot[k] = v;
    }
  }
  __syncthreads();
  if (tid == 0) {
    const long long n_s = itot[0], n_t = itot[1];
    const double ds = n_s > 0 ? 0.5 * tot[0] / (double)n_s : 0.0, dt = n_t > 0 ? 0.5 * tot[1] / (double)n_t : 0.0;
    stats[0] = (float)(ds + dt);
    stats[1] = (float)(n_t > 0 ? tot[2] / (double)n_t : 0.0);
    count[0] = (int64_t)n_s, count[1] = (int64_t)n_t;
    correct[0] = (int64_t)itot[2], correct[1] = (int64_t)itot[3];
  }
}

__global__ __launch_bounds__(256) void k_adv_scale(const float* __restrict__ gx, int ld_g, int64_t total, int C,
                                                    const float* __restrict__ gout, float* __restrict__ dx, int ld_d) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t r = e / C;
  const int c = (int)(e - r * C);
  dx[r * ld_d + c] = gout[0] * gx[r * ld_g + c] + 0.f;  // + 0: a zero gradient stays +0 under a negative grad_out
}

template <int H>
int adv_launch_rows(int nb, size_t lds, hipStream_t s, const float* x, int ld, int64_t N, int64_t P, int C, int mode, const float* params,
                    const long long* pcnt, int nbc, double* psum, long long* pcor, float* gx, int ld_g) {
  static unsigned once = 0;  // per-device bit: see mm_attr_todo (common.h)
  if (mm_attr_todo(&once)) {
    MM_HIP(hipFuncSetAttribute((const void*)k_adv_rows<H>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(adv_lds_floats(MAXC, H) * sizeof(float))));
    mm_attr_done(&once);
  }
  hipLaunchKernelGGL(k_adv_rows<H>, dim3(nb), dim3(PT), lds, s, x, ld, N, P, C, mode, params, pcnt, nbc, psum, pcor, gx, ld_g);
  MM_LAUNCH_CHECK();
  return MM_OK;
}
}  // namespace

extern "C" {

int64_t mm_adv_param_count(int C, int H) {
  if (C < 2 || C > MAXC || !adv_h_ok(H)) return 0;
  return adv_params(C, H);
}

size_t mm_adv_ws_bytes(int C, int H) {
  if (C < 2 || C > MAXC || !adv_h_ok(H)) return 0;
  return adv_ws(nullptr, C, H).bytes;
}

int mm_adv_fwd(const float* x, int ld, int64_t N, int64_t P, int C, int H, int mode, const float* params, float* stats, int64_t* count,
               int64_t* correct, float* dparams, float* gx, int ld_gx, void* ws, size_t ws_bytes, hipStream_t s) {
  MM_CHECK_ARG(C >= 2 && C <= MAXC, "adv_fwd: C must lie in [2, 32]");
  MM_CHECK_ARG(adv_h_ok(H), "adv_fwd: H must be 16, 32 or 64");
  MM_CHECK_ARG(ld >= C && ld_gx >= C, "adv_fwd: row pitch below C");
  MM_CHECK_ARG(N >= 0 && P >= 0 && P <= N, "adv_fwd: the first target row must lie in [0, N]");
  MM_CHECK_ARG(N <= (((int64_t)1 << 31) - 1) / C, "adv_fwd: N * C must stay below 2^31");
  MM_CHECK_ARG(mode == MODE_SOFTMAX || mode == MODE_SELFINFO, "adv_fwd: mode must be 0 (softmax) or 1 (selfinfo)");
  MM_CHECK_ARG((x && gx) || N == 0, "adv_fwd: null x or gx");
  MM_CHECK_ARG(params && stats && count && correct && dparams, "adv_fwd: null params, stats, count, correct or dparams");
  MM_CHECK_ARG(ws && ws_bytes >= mm_adv_ws_bytes(C, H), "adv_fwd: workspace missing or too small");
  static_assert(adv_lds_floats(MAXC, 64) * sizeof(float) <= 160 * 1024, "the tiles and the parameters fit a CU's LDS");
  const AdvWs w = adv_ws(ws, C, H);
  const int np = adv_params(C, H);
  const int64_t nt = mm_cdiv(N, PT);
  const int nb = (int)(nt > ADV_MAX_WG ? ADV_MAX_WG : nt);  // workgroups of the count pass and of the row pass
  if (nb > 0) {
    hipLaunchKernelGGL(k_adv_count, dim3(nb), dim3(PT), (size_t)PT * (C | 1) * sizeof(float), s, x, ld, N, P, C, w.pcnt);
    MM_LAUNCH_CHECK();
    const size_t lds = adv_lds_floats(C, H) * sizeof(float);
    int rc = MM_OK;
    if (H == 16) rc = adv_launch_rows<16>(nb, lds, s, x, ld, N, P, C, mode, params, w.pcnt, nb, w.psum, w.pcor, gx, ld_gx);
    else if (H == 32) rc = adv_launch_rows<32>(nb, lds, s, x, ld, N, P, C, mode, params, w.pcnt, nb, w.psum, w.pcor, gx, ld_gx);
    else rc = adv_launch_rows<64>(nb, lds, s, x, ld, N, P, C, mode, params, w.pcnt, nb, w.psum, w.pcor, gx, ld_gx);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_adv_final, dim3((unsigned)mm_cdiv(np, FQ) + 1), dim3(FQ * FPARTS), 0, s, (const double*)w.psum, nb, np,
                     (const long long*)w.pcnt, nb, (const long long*)w.pcor, dparams, stats, count, correct);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_adv_bwd(const float* gx, int ld_gx, int64_t N, int C, const float* grad_out, float* dx, int ld_dx, hipStream_t s) {
  MM_CHECK_ARG(C >= 2 && C <= MAXC, "adv_bwd: C must lie in [2, 32]");
  MM_CHECK_ARG(ld_gx >= C && ld_dx >= C, "adv_bwd: row pitch below C");
  MM_CHECK_ARG(N >= 0 && N <= (((int64_t)1 << 31) - 1) / C, "adv_bwd: N must lie in [0, 2^31 / C)");
  MM_CHECK_ARG(grad_out, "adv_bwd: null grad_out");
  MM_CHECK_ARG((gx && dx) || N == 0, "adv_bwd: null gx or dx");
  if (N == 0) return MM_OK;
  const int64_t total = N * C;
  hipLaunchKernelGGL(k_adv_scale, dim3((unsigned)mm_cdiv(total, 256)), dim3(256), 0, s, gx, ld_gx, total, C, grad_out, dx, ld_dx);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"
