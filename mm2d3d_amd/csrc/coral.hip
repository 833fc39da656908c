// Correlation alignment (Deep CORAL, Sun & Saenko, ECCV-W 2016; Deep LogCORAL, Morerio et al., ICLR 2018) of the rows [0, P) and
// [P, N) of a row matrix x [N, d]; include/mm2d3d.h has the definition.
//   mm_coral_fwd  k_coral_stats: a capped grid walks the 128-row tiles of the source rows, then those of the target rows (a tile never
//                 straddles P), staged through LDS (stage_rows of rows.h); a lane zeroes its row in the tile when it is not counted.
//                 Then the threads share the segment's K = d + d (d + 1) / 2 quantities - d column sums and the upper triangle of
//                 sum x xT - one fp64 accumulator each (up to KQ = 5 per thread at d = 32), rows ascending, carried across the
//                 workgroup's tiles; the product of two fp32 values is exact in fp64.  All lanes of a wave read one row of the
//                 tile at a time: at most d <= 32 distinct words of a pitch-(d | 1) row, which fall on distinct banks.  Row counts
//                 are ballots (wave_count, block_count).
//                 k_coral_final: one workgroup of ROWS_FT threads totals the partials (sum_partial: a wave per quantity), forms
//                 means and covariances in fp64 and, in log mode, diagonalises both d x d matrices at once (threads [0, 512) the
//                 source's, [512, 1024) the target's) with a cyclic Jacobi iteration in the round-robin order: the d / 2 rotations of a
//                 step touch disjoint index pairs and are applied together, d - 1 steps make a sweep, the order is fixed.  Then
//                 the matrix logarithms, the loss and the Daleckii-Krein gradient matrices as five small products.
//   mm_coral_bwd  k_coral_bwd: one 128-row tile per workgroup, staged the same way, both gradient matrices in LDS; a lane forms
//                 grad_out * (x_i - m_a) * aux_a for its row in registers (DP = 8, 16 or 32 columns, chosen by d on the host)
//                 and writes it over the row; the tile leaves through unstage_rows.
// No atomics of any kind, no grid barrier, no workgroup waits for another: bit-stable run to run.
#include "common.h"
#include "pointpred.h"
#include "rows.h"

namespace {
constexpr int PT = 128;  // rows per tile = threads per workgroup
constexpr int MAXD = MM_PRED_MAXC;
constexpr int KMAX = MAXD + MAXD * (MAXD + 1) / 2;  // 560 quantities per segment at d = 32
constexpr int KQ = (KMAX + PT - 1) / PT;            // ... at most 5 per thread
constexpr int LP = MAXD + 1;                        // pitch of the fp64 matrices of the finish: odd, so that a column walk meets distinct banks
constexpr int HALF = ROWS_FT / 2;                   // threads per matrix in the finish
constexpr int MAX_SWEEPS = 30;
constexpr int MODE_PLAIN = 0, MODE_LOG = 1;

__host__ __device__ inline int coral_K(int d) { return d + d * (d + 1) / 2; }
// where sum x_j x_k (j <= k) lies among a segment's K quantities: behind the d column sums, the upper triangle row by row
__device__ __forceinline__ int tri_index(int d, int j, int k) { return d + j * d - j * (j - 1) / 2 + (k - j); }

__global__ __launch_bounds__(PT) void k_coral_stats(const float* __restrict__ x, int ld, int64_t N, int64_t P, int d,
                                                     double* __restrict__ psum /*[grid][2][K]*/, long long* __restrict__ pcnt /*[grid][2]*/) {
  extern __shared__ float tile[];  // [PT][pitch]
  __shared__ unsigned wcnt[PT / 64];
  const int pitch = d | 1, K = coral_K(d);
  // quantity threadIdx.x + q * PT of this thread: the sum of column cj[q] (one[q]) or of the products of columns cj[q], ck[q]
  int cj[KQ], ck[KQ], nq = 0;
  bool one[KQ];
#pragma unroll
  for (int q = 0; q < KQ; q++) {
    const int idx = (int)threadIdx.x + q * PT;
    cj[q] = 0, ck[q] = 0, one[q] = true;
    if (idx < K) {
      nq = q + 1;
      if (idx < d) {
        cj[q] = ck[q] = idx;
      } else {
        one[q] = false;
        int r = idx - d, j = 0;
        while (r >= d - j) r -= d - j, j++;
        cj[q] = j, ck[q] = j + r;
      }
    }
  }
  const int64_t ts = (P + PT - 1) / PT;  // tiles of the source rows
  for (int seg = 0; seg < 2; seg++) {
    const int64_t first = seg ? P : 0, end = seg ? N : P;
    const int64_t nt = (end - first + PT - 1) / PT;
    // the target's tiles go on where the source's ended, so that the grid shares ts + nt tiles evenly
    const int64_t t0 = seg ? (int64_t)((blockIdx.x + gridDim.x - (unsigned)(ts % gridDim.x)) % gridDim.x) : (int64_t)blockIdx.x;
    double acc[KQ];
#pragma unroll
    for (int q = 0; q < KQ; q++) acc[q] = 0.0;
    unsigned wn[1] = {0};  // per wave: every lane holds the wave's count (N * d < 2^31: below 2^30 rows)
    for (int64_t t = t0; t < nt; t += gridDim.x) {
      const RowTile tl = row_tile<PT>(t, end, first);
      __syncthreads();  // the previous tile's sums have been taken
      stage_rows<PT>(tile, x + tl.row0 * ld, ld, tl.rows, d, pitch);
      __syncthreads();
      bool counted = false;
      if ((int)threadIdx.x < tl.rows) {
        float* a = tile + threadIdx.x * pitch;
        counted = row_finite(a, d);
        if (!counted)
          for (int c = 0; c < d; c++) a[c] = 0.f;  // adds +0 to every sum
      }
      wn[0] += wave_count(counted);
      __syncthreads();
      if (nq > 0) {
        for (int r = 0; r < tl.rows; r++) {  // rows ascending: the order is part of the result bits
          const float* a = tile + r * pitch;
#pragma unroll
          for (int q = 0; q < KQ; q++)
            if (q < nq) acc[q] += (double)a[cj[q]] * (one[q] ? 1.0 : (double)a[ck[q]]);
        }
      }
    }
    double* out = psum + ((int64_t)blockIdx.x * 2 + seg) * K;
#pragma unroll
    for (int q = 0; q < KQ; q++)
      if (q < nq) out[threadIdx.x + q * PT] = acc[q];
    __syncthreads();  // the count words of the segment before have been read
    const long long n = block_count<PT>(wn, wcnt);
    if (threadIdx.x == 0) pcnt[blockIdx.x * 2 + seg] = n;
  }
}

// (log a - log b) / (a - b) for a, b > 0 without cancellation: log1p(t) / (t lo), t = (hi - lo) / lo >= 0; its series where t is tiny
__device__ __forceinline__ double log_divided_difference(double a, double b) {
  const double lo = a < b ? a : b, hi = a < b ? b : a;
  const double t = (hi - lo) / lo;
  const double f = t < 1e-5 ? 1.0 - t * (0.5 - t * (1.0 / 3.0 - 0.25 * t)) : log1p(t) / t;
  return f / lo;
}

// out = A B, d x d matrices of pitch LP, over one matrix's HALF threads
__device__ __forceinline__ void small_product(double* __restrict__ out, const double* A, const double* B, int d, int t) {
  for (int e = t; e < d * d; e += HALF) {
    const int j = e / d, k = e - j * d;
    double s = 0.0;
    for (int i = 0; i < d; i++) s += A[j * LP + i] * B[i * LP + k];
    out[j * LP + k] = s;
  }
}

// loss[1]; count[2] = n_s, n_t; mean[2][d]; cov[2][d][d]; aux = mean_s[d], mean_t[d], what their fp32 rounding left of the fp64 means
// [2][d], then the two d x d matrices 2 / (n_a - 1) * G_a
__global__ __launch_bounds__(ROWS_FT) void k_coral_final(const double* __restrict__ psum, const long long* __restrict__ pcnt, int nb, int d,
                                                        int mode, double eps, float* __restrict__ loss, int64_t* __restrict__ count,
                                                        float* __restrict__ mean, float* __restrict__ cov, float* __restrict__ aux) {
  __shared__ double tot[2 * KMAX];
  __shared__ double Ab[2][2][MAXD * LP];  // [matrix][ping-pong]
  __shared__ double Vb[2][MAXD * LP];
  __shared__ double lam[2][MAXD], llam[2][MAXD];
  __shared__ double rc[2][MAXD], rs[2][MAXD], rd[2][MAXD];  // per index of a step: cos, -+sin, the change of its diagonal element
  __shared__ int rp[2][MAXD];                               // ... and the index it is rotated with
  __shared__ unsigned char raised[2][MAXD];
  __shared__ long long cnt[2];
  __shared__ int rotated[2];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = coral_K(d), dd = d * d;
  for (int q = wave; q < 2 * K + 2; q += ROWS_FT / 64) {  // uniform per wave
    if (q < 2 * K) {
      const double v = sum_partial(psum, nb, 2 * K, q, lane);
      if (lane == 0) tot[q] = v;
    } else {
      const long long s = sum_partial(pcnt, nb, 2, q - 2 * K, lane);
      if (lane == 0) cnt[q - 2 * K] = s;
    }
  }
  if (tid < 2) rotated[tid] = 0;
  __syncthreads();
  const long long n0 = cnt[0], n1 = cnt[1];
  if (tid < 2 * d) {
    const int a = tid / d, j = tid - a * d;
    const long long n = a ? n1 : n0;
    const double m = n > 0 ? tot[a * K + j] / (double)n : 0.0;
    const float hi = (float)m;
    mean[tid] = hi;
    aux[tid] = hi;
    aux[2 * d + tid] = (float)(m - (double)hi);  // the mean to 48 bits: the centred row of the backward then rounds once
  }
  if (tid < 2) count[tid] = (int64_t)(tid ? n1 : n0);
  for (int e = tid; e < 2 * dd; e += ROWS_FT) {
    const int a = e / dd, r = e - a * dd, j = r / d, k = r - j * d;
    const long long n = a ? n1 : n0;
    const double* T = tot + a * K;
    double c = 0.0;
    if (n >= 2) c = (T[tri_index(d, j < k ? j : k, j < k ? k : j)] - T[j] * T[k] / (double)n) / (double)(n - 1);
    Ab[a][0][j * LP + k] = c;
    cov[e] = (float)c;
  }
  __syncthreads();
  float* gm = aux + 4 * d;  // the two gradient matrices
  const double inv_d2 = 1.0 / (double)dd;
  if (n0 < 2 || n1 < 2) {  // uniform: a segment without a covariance - loss 0, a zero gradient
    for (int e = tid; e < 2 * dd; e += ROWS_FT) gm[e] = 0.f;
    if (tid == 0) loss[0] = 0.f;
    return;
  }
  const double k0 = 2.0 / (double)(n0 - 1), k1 = 2.0 / (double)(n1 - 1);
  if (mode == MODE_PLAIN) {
    for (int e = tid; e < dd; e += ROWS_FT) {
      const int j = e / d, k = e - j * d;
      const double D = Ab[0][0][j * LP + k] - Ab[1][0][j * LP + k];
      Ab[0][1][j * LP + k] = D;
      gm[e] = (float)(k0 * 0.5 * inv_d2 * D);
      gm[dd + e] = (float)(-k1 * 0.5 * inv_d2 * D);
    }
    __syncthreads();
    if (wave == 0) {
      double s = 0.0;
      for (int e = lane; e < dd; e += 64) {
        const double D = Ab[0][1][(e / d) * LP + e % d];
        s += D * D;
      }
      s = wave_sum(s);
      if (lane == 0) loss[0] = (float)(0.25 * inv_d2 * s);
    }
    return;
  }

  // ---- log mode: C_a + eps I = V diag(lam) VT by cyclic Jacobi, both matrices at once
  const int h = tid / HALF, t = tid - h * HALF;
  double* V = Vb[h];
  for (int e = t; e < dd; e += HALF) {
    const int j = e / d, k = e - j * d;
    if (j == k) Ab[h][0][j * LP + k] += eps;
    V[j * LP + k] = j == k ? 1.0 : 0.0;
  }
  __syncthreads();
  const int de = d + (d & 1), m = de / 2;  // an odd d plays with a bye
  const double tol = (double)d * 2.220446049250313e-16;
  int cur = 0;
  for (int sweep = 0; sweep < MAX_SWEEPS; sweep++) {
    for (int step = 0; step < de - 1; step++) {
      const double* A = Ab[h][cur];
      if (t < m) {  // the round-robin pairing: index de - 1 stays, the others go round
        const int ia = t == 0 ? de - 1 : (step + t) % (de - 1), ib = t == 0 ? step : (step + de - 1 - t) % (de - 1);
        const int p = ia < ib ? ia : ib, q = ia < ib ? ib : ia;
        if (q < d) {
          const double app = A[p * LP + p], aqq = A[q * LP + q], apq = A[p * LP + q];
          double c = 1.0, s = 0.0, tt = 0.0;
          if (fabs(apq) > tol * sqrt(fabs(app * aqq))) {
            const double theta = (aqq - app) / (2.0 * apq);
            tt = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
            c = 1.0 / sqrt(tt * tt + 1.0);
            s = tt * c;
            if (s != 0.0) rotated[sweep & 1] = 1;
          }
          rc[h][p] = c, rs[h][p] = -s, rd[h][p] = -tt * apq, rp[h][p] = q;
          rc[h][q] = c, rs[h][q] = s, rd[h][q] = tt * apq, rp[h][q] = p;
        } else if (p < d) {
          rc[h][p] = 1.0, rs[h][p] = 0.0, rd[h][p] = 0.0, rp[h][p] = p;
        }
      }
      __syncthreads();
      if (tid == 0 && step == 0) rotated[(sweep + 1) & 1] = 0;  // everybody is past the test of the sweep before
      double* B = Ab[h][cur ^ 1];
      for (int e = t; e < dd; e += HALF) {
        const int k = e / d, l = e - k * d;
        const int pk = rp[h][k], pl = rp[h][l];
        const double ckk = rc[h][k], sk = rs[h][k], cl = rc[h][l], sl = rs[h][l];
        if (l < pl) {  // the two columns of a pair of V, by the thread of the lower one
          const double vl = V[k * LP + l], vp = V[k * LP + pl];
          V[k * LP + l] = cl * vl + sl * vp;
          V[k * LP + pl] = rc[h][pl] * vp + rs[h][pl] * vl;
        }
        if (k <= l) {  // JT A J: the upper triangle, mirrored
          double o;
          if (k == l) {
            o = A[k * LP + k] + rd[h][k];
          } else if (l == pk && sk != 0.0) {
            o = 0.0;  // the pivot of a rotation
          } else {
            const double r0 = cl * A[k * LP + l] + sl * A[k * LP + pl], r1 = cl * A[pk * LP + l] + sl * A[pk * LP + pl];
            o = ckk * r0 + sk * r1;
          }
          B[k * LP + l] = o;
          B[l * LP + k] = o;
        }
      }
      cur ^= 1;
      __syncthreads();
    }
    if (!rotated[sweep & 1]) break;  // uniform: no pair of either matrix was above the threshold
  }
  if (t < d) {
    const double l = Ab[h][cur][t * LP + t];
    raised[h][t] = l < eps;  // rounding pushed an eigenvalue of C + eps I below eps
    lam[h][t] = l < eps ? eps : l;
    llam[h][t] = log(l < eps ? eps : l);
  }
  __syncthreads();
  double *B0 = Ab[0][cur], *Bh = Ab[h][cur], *Lh = Ab[h][cur ^ 1];
  for (int e = t; e < dd; e += HALF) {  // log(C_a + eps I) = V diag(log lam) VT
    const int j = e / d, k = e - j * d;
    if (j <= k) {
      double s = 0.0;
      for (int i = 0; i < d; i++) s += V[j * LP + i] * llam[h][i] * V[k * LP + i];
      Lh[j * LP + k] = s;
      Lh[k * LP + j] = s;
    }
  }
  __syncthreads();
  for (int e = tid; e < dd; e += ROWS_FT) {
    const int j = e / d, k = e - j * d;
    B0[j * LP + k] = Ab[0][cur ^ 1][j * LP + k] - Ab[1][cur ^ 1][j * LP + k];  // Delta
  }
  __syncthreads();
  if (wave == 0) {
    double s = 0.0;
    for (int e = lane; e < dd; e += 64) {
      const double D = B0[(e / d) * LP + e % d];
      s += D * D;
    }
    s = wave_sum(s);
    if (lane == 0) loss[0] = (float)(inv_d2 * s);
  }
  small_product(Lh, B0, V, d, t);  // Delta V
  __syncthreads();
  for (int e = t; e < dd; e += HALF) {  // (VT Delta V) o K
    const int j = e / d, k = e - j * d;
    double s = 0.0;
    for (int i = 0; i < d; i++) s += V[i * LP + j] * Lh[i * LP + k];
    const double kk = j == k ? (raised[h][j] ? 0.0 : 1.0 / lam[h][j]) : log_divided_difference(lam[h][j], lam[h][k]);
    Bh[j * LP + k] = s * kk;
  }
  __syncthreads();
  small_product(Lh, V, Bh, d, t);  // V M
  __syncthreads();
  const double scale = (h ? -k1 : k0) * 2.0 * inv_d2;
  for (int e = t; e < dd; e += HALF) {  // ... VT
    const int j = e / d, k = e - j * d;
    double s = 0.0;
    for (int i = 0; i < d; i++) s += Lh[j * LP + i] * V[k * LP + i];
    gm[h * dd + e] = (float)(scale * s);
  }
}

// dx_i = grad_out * (x_i - m_a) * aux_a for a counted row of segment a, +0 for any other
template <int DP>
__global__ __launch_bounds__(PT) void k_coral_bwd(const float* __restrict__ x, int ld, int64_t N, int64_t P, int d,
                                                   const float* __restrict__ aux, const float* __restrict__ gout, float* __restrict__ dx,
                                                   int ld_d) {
  extern __shared__ float tile[];  // [PT][pitch]
  __shared__ float G[2][DP * DP];  // zero beyond d
  __shared__ float mu[2][DP], mu_lo[2][DP];
  const int pitch = d | 1, dd = d * d;
  const RowTile t = row_tile<PT>(blockIdx.x, N);
  for (int e = threadIdx.x; e < 2 * DP * DP; e += PT) {
    const int a = e / (DP * DP), r = e - a * DP * DP, j = r / DP, k = r - j * DP;
    G[a][r] = j < d && k < d ? aux[4 * d + a * dd + j * d + k] : 0.f;
  }
  if ((int)threadIdx.x < 2 * DP) {
    const int a = threadIdx.x / DP, j = threadIdx.x - a * DP;
    mu[a][j] = j < d ? aux[a * d + j] : 0.f;
    mu_lo[a][j] = j < d ? aux[2 * d + a * d + j] : 0.f;
  }
  stage_rows<PT>(tile, x + t.row0 * ld, ld, t.rows, d, pitch);
  __syncthreads();
  if ((int)threadIdx.x < t.rows) {
    float* a = tile + threadIdx.x * pitch;
    if (row_finite(a, d)) {
      const int seg = t.row0 + threadIdx.x >= P;
      const float *Gs = G[seg], *ms = mu[seg], *ml = mu_lo[seg];
      const float g = gout[0];
      float o[DP];
#pragma unroll
      for (int k = 0; k < DP; k++) o[k] = 0.f;
#pragma unroll 1
      for (int j = 0; j < d; j++) {
        const float c = (a[j] - ms[j]) - ml[j];
#pragma unroll
        for (int k = 0; k < DP; k++) o[k] = fmaf(c, Gs[j * DP + k], o[k]);
      }
#pragma unroll
      for (int k = 0; k < DP; k++)
        if (k < d) a[k] = g * o[k] + 0.f;  // + 0: a zero gradient is +0 whatever the signs
    } else {
      for (int c = 0; c < d; c++) a[c] = 0.f;
    }
  }
  __syncthreads();
  unstage_rows<PT>(dx + t.row0 * ld_d, ld_d, tile, t.rows, d, pitch);
}

int coral_check(const char* who, const float* x, int ld, int64_t N, int64_t P, int d) {
  MM_CHECK_ARG(d >= 2 && d <= MAXD, "%s: d must lie in [2, 32]", who);
  MM_CHECK_ARG(ld >= d, "%s: row pitch below d", who);
  MM_CHECK_ARG(N >= 0 && P >= 0 && P <= N, "%s: the first target row must lie in [0, N]", who);
  MM_CHECK_ARG(N <= (((int64_t)1 << 31) - 1) / d, "%s: N * d must stay below 2^31", who);
  MM_CHECK_ARG(x || N == 0, "%s: null x", who);
  return MM_OK;
}
}  // namespace

extern "C" {

size_t mm_coral_ws_bytes(int d) {
  if (d < 2 || d > MAXD) return 0;
  return stats_ws(nullptr, 2 * coral_K(d), 2).bytes;
}

int mm_coral_fwd(const float* x, int ld, int64_t N, int64_t P, int d, int mode, float eps, float* loss, int64_t* count, float* mean,
                 float* cov, float* aux, void* ws, size_t ws_bytes, hipStream_t s) {
  static_assert(2 * MAXD <= ROWS_FT && MAXD * MAXD <= ROWS_FT && MAXD / 2 <= HALF, "the finish gives a thread an element");
  if (int rc = coral_check("coral_fwd", x, ld, N, P, d)) return rc;
  MM_CHECK_ARG(mode == MODE_PLAIN || mode == MODE_LOG, "coral_fwd: mode must be 0 (plain) or 1 (log)");
  MM_CHECK_ARG(eps > 0.f && eps <= ROWS_F32_MAX, "coral_fwd: eps must be finite and > 0");
  MM_CHECK_ARG(loss && count && mean && cov && aux, "coral_fwd: null loss, count, mean, cov or aux");
  MM_CHECK_ARG(ws && ws_bytes >= mm_coral_ws_bytes(d), "coral_fwd: workspace missing or too small");
  const StatsWs w = stats_ws(ws, 2 * coral_K(d), 2);
  const int64_t nt = mm_cdiv(P, PT) + mm_cdiv(N - P, PT);
  const int nb = (int)(nt > ROWS_MAX_WG ? ROWS_MAX_WG : nt);
  if (nb > 0) {
    const size_t lds = (size_t)PT * (d | 1) * sizeof(float);  // <= 16.9 KB
    hipLaunchKernelGGL(k_coral_stats, dim3(nb), dim3(PT), lds, s, x, ld, N, P, d, w.psum, w.pcnt);
    MM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_coral_final, dim3(1), dim3(ROWS_FT), 0, s, (const double*)w.psum, (const long long*)w.pcnt, nb, d, mode, (double)eps,
                     loss, count, mean, cov, aux);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_coral_bwd(const float* x, int ld, int64_t N, int64_t P, int d, const float* aux, const float* grad_out, float* dx, int ld_dx,
                 hipStream_t s) {
  if (int rc = coral_check("coral_bwd", x, ld, N, P, d)) return rc;
  MM_CHECK_ARG(ld_dx >= d, "coral_bwd: gradient row pitch below d");
  MM_CHECK_ARG(aux && grad_out, "coral_bwd: null aux or grad_out");
  MM_CHECK_ARG(dx || N == 0, "coral_bwd: null dx");
  if (N == 0) return MM_OK;
  const size_t lds = (size_t)PT * (d | 1) * sizeof(float);  // <= 16.9 KB
  const dim3 grid((unsigned)mm_cdiv(N, PT));
  if (d <= 8) hipLaunchKernelGGL(k_coral_bwd<8>, grid, dim3(PT), lds, s, x, ld, N, P, d, aux, grad_out, dx, ld_dx);
  else if (d <= 16) hipLaunchKernelGGL(k_coral_bwd<16>, grid, dim3(PT), lds, s, x, ld, N, P, d, aux, grad_out, dx, ld_dx);
  else hipLaunchKernelGGL(k_coral_bwd<32>, grid, dim3(PT), lds, s, x, ld, N, P, d, aux, grad_out, dx, ld_dx);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"
