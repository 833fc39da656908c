// Target-domain entropy and diversity (MinEnt, Vu et al. CVPR 2019; the diversity term of information maximisation, SHOT, Liang et
// al. ICML 2020) of the rows [P, N) of per-point logits [N, C]; include/mm2d3d.h has the definition.
//   mm_im_fwd   k_im_stats: a capped grid walks the 128-row tiles of the target rows, staged through LDS (stage_rows of rows.h).  A
//               lane that kept 1 + C accumulators indexed by a runtime c would spill them, so each lane writes its row's softmax back
//               INTO the staged tile (zeros for a row that is not counted) and its entropy into ent[]; then thread j sums column j
//               over the tile's rows in ascending order into ONE fp64 accumulator that it carries across the workgroup's tiles
//               (col_sum of rows.h).  Row counts are ballots, integers throughout (wave_count, block_count).
//               k_im_final: one workgroup of ROWS_FT threads sums the <= ROWS_MAX_WG partials per quantity (sum_partial
//               of rows.h: a wave per quantity, sixteen waves share the 1 + C sums and the count) and writes the two
//               losses, the class mass, the count and what the backward reads.
//               The walk, the finish and the workspace (stats_ws) are those of k_pl_stats / k_pl_update (pselab.hip).
//   mm_im_bwd   k_im_bwd: one 128-row tile per workgroup, staged the same way; each lane forms its gradient row in place, the
//               workgroup writes the tile out with consecutive lanes on consecutive addresses (unstage_rows).  Tiles of head rows
//               alone write zeros.
// No atomics of any kind, no grid barrier, no workgroup waits for another: bit-stable run to run.
#include "common.h"
#include "pointpred.h"
#include "rows.h"

namespace {
constexpr int PT = 128;  // rows per tile = threads per workgroup
constexpr int MAXC = MM_PRED_MAXC;

__global__ __launch_bounds__(PT) void k_im_stats(const float* __restrict__ logits, int ld, int64_t N, int64_t P, int C,
                                                  double* __restrict__ psum /*[grid][C + 1]*/, long long* __restrict__ pcnt /*[grid]*/) {
  extern __shared__ float tile[];  // [PT][pitch], then ent [PT]
  __shared__ unsigned wcnt[PT / 64];
  const int pitch = C | 1;
  float* ent = tile + PT * pitch;
  const int K = C + 1, j = (int)threadIdx.x;  // the column this thread sums (threads < K): C masses, then the entropy
  double acc = 0.0;
  unsigned wn[1] = {0};  // per wave: every lane holds the wave's count (N * C < 2^31: below 2^30 rows)
  const int64_t T = N - P;
  const unsigned ntiles = (unsigned)((T + PT - 1) / PT);
  for (unsigned t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const RowTile tl = row_tile<PT>(t, N, P);
    __syncthreads();  // the previous tile's columns have been summed
    stage_rows<PT>(tile, logits + tl.row0 * ld, ld, tl.rows, C, pitch);
    __syncthreads();
    bool counted = false;
    if ((int)threadIdx.x < tl.rows) {
      float* a = tile + threadIdx.x * pitch;
      counted = row_finite(a, C);
      const RowLse r = row_lse(a, C);
      const float ls = logf(r.s);
      float h = 0.f;
#pragma unroll 1
      for (int c = 0; c < C; c++) {
        const float d = a[c] - r.m, p = expf(d) / r.s;
        if (p > 0.f) h -= p * (d - ls);  // p == 0: the limit 0 * log 0 = 0 (d may be -inf for logits 2^128 apart)
        a[c] = counted ? p : 0.f;
      }
      ent[threadIdx.x] = counted ? h : 0.f;
    }
    wn[0] += wave_count(counted);
    __syncthreads();
    if (j < K) {
      if (j == C) col_sum(acc, ent, 1, tl.rows);
      else col_sum(acc, tile + j, pitch, tl.rows);
    }
  }
  if (j < K) psum[(int64_t)blockIdx.x * K + j] = acc;
  const long long n = block_count<PT>(wn, wcnt);
  if (threadIdx.x == 0) pcnt[blockIdx.x] = n;
}

// stats[2] = ent, div; mass[C]; count[1] = n; aux[C + 1] = g_c = ln(mass_c / pi_c) (0 where mass_c == 0), then 1 / (n ln C)
// (0 when n == 0): what k_im_bwd reads.  prior == NULL: pi_c = 1 / C.
__global__ __launch_bounds__(ROWS_FT) void k_im_final(const double* __restrict__ psum, const long long* __restrict__ pcnt, int nb, int C,
                                                     const float* __restrict__ prior, float* __restrict__ stats, float* __restrict__ mass,
                                                     int64_t* __restrict__ count, float* __restrict__ aux) {
  __shared__ double tot[MAXC + 1];
  __shared__ double term[MAXC];
  __shared__ long long cnt;
  const int K = C + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int q = wave; q < K + 1; q += ROWS_FT / 64) {  // uniform per wave
    if (q < K) {
      const double v = sum_partial(psum, nb, K, q, lane);
      if (lane == 0) tot[q] = v;
    } else {
      const long long s = sum_partial(pcnt, nb, 1, 0, lane);
      if (lane == 0) cnt = s;
    }
  }
  __syncthreads();
  const long long n = cnt;
  const double lnC = log((double)C);
  const double scale = n > 0 ? 1.0 / ((double)n * lnC) : 0.0;
  if ((int)threadIdx.x < C) {
    const double m = n > 0 ? tot[threadIdx.x] / (double)n : 0.0;
    const double lp = prior ? log((double)prior[threadIdx.x]) : -lnC;
    const double g = m > 0.0 ? log(m) - lp : 0.0;
    term[threadIdx.x] = m * g;
    mass[threadIdx.x] = (float)m;
    aux[threadIdx.x] = (float)g;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double d = 0.0;
    for (int c = 0; c < C; c++) d += term[c];  // ascending: a fixed order
    d /= lnC;
    stats[0] = (float)(tot[C] * scale);
    stats[1] = (float)(d > 0.0 ? d : 0.0);  // a KL divergence: rounding may leave -1e-17 where it is 0
    count[0] = (int64_t)n;
    aux[C] = (float)scale;
  }
}

// d ent / dx_k = -p_k (log p_k + H) / (n ln C);  d div / dx_k = p_k (g_k - sum_c p_c g_c) / (n ln C)
__global__ __launch_bounds__(PT) void k_im_bwd(const float* __restrict__ logits, int ld, int64_t N, int64_t P, int C,
                                                const float* __restrict__ aux, const float* __restrict__ gout, float* __restrict__ dl,
                                                int ld_d) {
  extern __shared__ float tile[];  // [PT][pitch]
  __shared__ float gs[MAXC + 1];
  const int pitch = C | 1;
  const RowTile t = row_tile<PT>(blockIdx.x, N);
  float* out = dl + t.row0 * ld_d;
  if (t.row0 + t.rows <= P) {  // uniform: head rows alone
    unstage_rows<PT, true>(out, ld_d, tile, t.rows, C, pitch);
    return;
  }
  if ((int)threadIdx.x <= C) gs[threadIdx.x] = aux[threadIdx.x];
  stage_rows<PT>(tile, logits + t.row0 * ld, ld, t.rows, C, pitch);
  __syncthreads();
  if ((int)threadIdx.x < t.rows) {
    float* a = tile + threadIdx.x * pitch;
    const bool counted = t.row0 + threadIdx.x >= P && row_finite(a, C);
    if (counted) {
      const float scale = gs[C], g0 = gout[0], g1 = gout[1];
      const RowLse r = row_lse(a, C);
      const float ls = logf(r.s);
      float h = 0.f, dot = 0.f;
#pragma unroll 1
      for (int c = 0; c < C; c++) {
        const float d = a[c] - r.m, p = expf(d) / r.s;
        if (p > 0.f) h -= p * (d - ls);
        dot += p * gs[c];
      }
#pragma unroll 1
      for (int c = 0; c < C; c++) {
        const float d = a[c] - r.m, p = expf(d) / r.s;
        const float de = p > 0.f ? -p * ((d - ls) + h) * scale : 0.f;
        const float dd = p * (gs[c] - dot) * scale;
        a[c] = g0 * de + g1 * dd;
      }
    } else {
      for (int c = 0; c < C; c++) a[c] = 0.f;
    }
  }
  __syncthreads();
  unstage_rows<PT>(out, ld_d, tile, t.rows, C, pitch);
}

int im_check(const char* who, const float* logits, int ld, int64_t N, int64_t P, int C) {
  MM_CHECK_ARG(C >= 2 && C <= MAXC, "%s: C must lie in [2, 32]", who);
  MM_CHECK_ARG(ld >= C, "%s: row pitch below C", who);
  MM_CHECK_ARG(N >= 0 && P >= 0 && P <= N, "%s: the first target row must lie in [0, N]", who);
  MM_CHECK_ARG(N <= (((int64_t)1 << 31) - 1) / C, "%s: N * C must stay below 2^31", who);
  MM_CHECK_ARG(logits || N == P, "%s: null logits", who);
  return MM_OK;
}
}  // namespace

extern "C" {

size_t mm_im_ws_bytes() { return stats_ws(nullptr, MAXC + 1, 1).bytes; }

int mm_im_fwd(const float* logits, int ld, int64_t N, int64_t P, int C, const float* prior, float* stats, float* mass, int64_t* count,
              float* aux, void* ws, size_t ws_bytes, hipStream_t s) {
  static_assert(MAXC + 1 <= PT && MAXC + 2 <= ROWS_FT, "one thread per column");
  if (int rc = im_check("im_fwd", logits, ld, N, P, C)) return rc;
  MM_CHECK_ARG(stats && mass && count && aux, "im_fwd: null stats, mass, count or aux");
  MM_CHECK_ARG(ws && ws_bytes >= mm_im_ws_bytes(), "im_fwd: workspace missing or too small");
  const StatsWs w = stats_ws(ws, MAXC + 1, 1);
  const int64_t nt = mm_cdiv(N - P, PT);
  const int nb = (int)(nt > ROWS_MAX_WG ? ROWS_MAX_WG : nt);
  if (nb > 0) {
    const size_t lds = ((size_t)PT * (C | 1) + PT) * sizeof(float);  // <= 17.4 KB
    hipLaunchKernelGGL(k_im_stats, dim3(nb), dim3(PT), lds, s, logits, ld, N, P, C, w.psum, w.pcnt);
    MM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_im_final, dim3(1), dim3(ROWS_FT), 0, s, (const double*)w.psum, (const long long*)w.pcnt, nb, C, prior, stats, mass,
                     count, aux);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_im_bwd(const float* logits, int ld, int64_t N, int64_t P, int C, const float* aux, const float* grad_out, float* dlogits,
              int ld_d, hipStream_t s) {
  if (int rc = im_check("im_bwd", logits, ld, N, P, C)) return rc;
  MM_CHECK_ARG(ld_d >= C, "im_bwd: gradient row pitch below C");
  MM_CHECK_ARG(aux && grad_out, "im_bwd: null aux or grad_out");
  MM_CHECK_ARG(dlogits || N == 0, "im_bwd: null dlogits");
  if (N == 0) return MM_OK;
  const size_t lds = (size_t)PT * (C | 1) * sizeof(float);  // <= 16.9 KB
  hipLaunchKernelGGL(k_im_bwd, dim3((unsigned)mm_cdiv(N, PT)), dim3(PT), lds, s, logits, ld, N, P, C, aux, grad_out, dlogits, ld_d);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"
