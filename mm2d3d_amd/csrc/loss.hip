// Row-wise losses over per-point logits [N, C]:
//   weighted cross entropy, ignore_index, weighted-mean reduction   (/root/reference/lib/losses.py:55-68)
//   cross-modal KL( softmax(target) || softmax(pred) ).sum(1).mean() (/root/reference/.../train.py:157-184)
// plus the evaluation's confusion matrices.  (The 2D->3D lifting is in lift.hip, the optimiser updates and the loss-scale kernels
// are in optim.hip.)
// Block partial sums are fp64 and combined in a fixed order: bit-stable run to run.
#include "common.h"
#include "pointpred.h"
#include "rows.h"

namespace {
constexpr int T = 256;
constexpr int MAX_PART = 1024;
constexpr int MAXC = MM_PRED_MAXC;

// ---- hard-label cross entropy over NSEG segments of the rows: rows [0, P) against (labels0, weight0) and, with NSEG = 2, rows
// [P, N) against (labels1, weight1), each segment its own weighted mean.  The joined [source | target] pass keeps a head's logits
// in ONE tensor; NSEG = 2 reads it once per direction and writes its gradient once (no slice gradients to zero-fill, copy and
// add).  NSEG = 1 (mm_ce_*: P = N, labels required) is the same code with `tail` a compile-time false: over one labelled segment
// the two agree bit for bit.  NSEG = 2: a NULL labels pointer = an unlabelled segment.
// RW (mm_ce2_*_w): row_w[N - P] scales the tail rows' terms of the loss and their gradient rows, not the weight sum.  A compile-time
// flag, as CLS below: without it the kernels are the kernels they were.
// partial[b] = (sum w*nll, sum w) per segment
template <int NSEG, bool RW = false>
__global__ __launch_bounds__(T) void k_ce_fwd(const float* __restrict__ logits, int ld, int64_t N, int64_t P, int C,
                                               const int64_t* __restrict__ labels0, const float* __restrict__ weight0,
                                               const int64_t* __restrict__ labels1, const float* __restrict__ weight1, int64_t ignore,
                                               const float* __restrict__ row_w, double* __restrict__ partial) {
  static_assert(!RW || NSEG == 2, "row weights belong to the tail");
  __shared__ double red[T];
  double sl[NSEG] = {}, sw[NSEG] = {};
  for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < N; i += (int64_t)gridDim.x * T) {
    const bool tail = NSEG == 2 && i >= P;
    const int64_t* labels = tail ? labels1 : labels0;
    if (NSEG == 2 && !labels) continue;
    int64_t y = labels[tail ? i - P : i];
    if (!label_counted(y, ignore, C)) continue;
    const float* weight = tail ? weight1 : weight0;
    const float* x = logits + i * ld;
    const RowLse r = row_lse(x, C);
    float nll = (r.m + logf(r.s)) - x[y];
    float w = weight ? weight[y] : 1.f;
    if (tail) {
      sl[NSEG - 1] += (double)(RW ? row_w[i - P] * (w * nll) : w * nll);  // x * 1.0f is exact: all-one row weights change no bit
      sw[NSEG - 1] += (double)w;
    } else {
      sl[0] += (double)(w * nll);
      sw[0] += (double)w;
    }
  }
  double* o = partial + 2 * NSEG * (int64_t)blockIdx.x;
#pragma unroll
  for (int s = 0; s < NSEG; s++) {
    double a = block_sum<T>(sl[s], red);
    double b = block_sum<T>(sw[s], red);
    if (threadIdx.x == 0) o[2 * s] = a, o[2 * s + 1] = b;
  }
}

// out[2 * s] = loss (0/0 = nan, as torch does when every label is ignored), out[2 * s + 1] = sum_w of segment s.  NSEG = 2 only:
// labelled: bit s = segment s has labels; zero_if_empty: bit s = a segment whose weights sum to 0 reports loss 0 instead of 0/0
template <int NSEG>
__global__ __launch_bounds__(64) void k_ce_finalize(const double* __restrict__ partial, int nb, int labelled, int zero_if_empty,
                                                     float* __restrict__ out /*[2 * NSEG]*/) {
  double v[2 * NSEG];
  sum_partials<2 * NSEG>(partial, nb, threadIdx.x, v);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < NSEG; s++) {
      double a = v[2 * s], b = v[2 * s + 1];
      bool zero = NSEG == 2 && (!((labelled >> s) & 1) || (((zero_if_empty >> s) & 1) && b == 0.0));
      out[2 * s] = zero ? 0.f : (float)(a / b);
      out[2 * s + 1] = (float)b;
    }
  }
}

// every row written once: segment s: gout[s] * w[y] / sum_w_s * (softmax - onehot), RW: times row_w of a tail row; ignored and
// unlabelled rows: zeros
template <int NSEG, bool RW = false>
__global__ __launch_bounds__(T) void k_ce_bwd(const float* __restrict__ logits, int ld, int64_t N, int64_t P, int C,
                                               const int64_t* __restrict__ labels0, const float* __restrict__ weight0,
                                               const int64_t* __restrict__ labels1, const float* __restrict__ weight1, int64_t ignore,
                                               const float* __restrict__ row_w, const float* __restrict__ stats,
                                               const float* __restrict__ gout, float* __restrict__ dlogits, int ld_d) {
  int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
  if (i >= N) return;
  const bool tail = NSEG == 2 && i >= P;
  const int64_t* labels = tail ? labels1 : labels0;
  const bool labelled = NSEG == 1 || labels;
  int64_t y = labelled ? labels[tail ? i - P : i] : ignore;
  float* d = dlogits + i * ld_d;
  if (!labelled || !label_counted(y, ignore, C)) {
    for (int c = 0; c < C; c++) d[c] = 0.f;
    return;
  }
  const float* weight = tail ? weight1 : weight0;
  const float* x = logits + i * ld;
  const RowLse r = row_lse(x, C);
  float k = gout[tail] * (weight ? weight[y] : 1.f) / stats[2 * tail + 1];
  if (RW && tail) k *= row_w[i - P];
  ce_grad_row(d, x, C, r.m, 1.f / r.s, k, (int)y);
}

// ---- two-segment cross entropy with a SOFT tail (mean-teacher targets): rows [0, P) as k_ce_*<2> against (labels0, weight0), rows
// [P, N) against the distribution q of the teacher logits ta (and tb: the ensemble), softened by the temperature, kept or not by
// the row's confidence at temperature 1 - pa / pe of mm_point_predict, the value mm_teacher_labels judges the row by.
// Staging: a workgroup is ONE wave and owns tiles of ST rows; the [rows, C] blocks of the (up to three) matrices go through LDS
// (stage_rows of rows.h, rows pitched to C | 1 words).  3 x 64 x 33 words = 25,344 bytes at C = 32: six workgroups per CU by
// LDS.  Sums: per lane fp64 over its rows in ascending order, a fixed shuffle tree per workgroup, then k_ce2s_finalize over the
// workgroups' partials in a fixed order; the kept count is an integer carried in fp64 (exact below 2^53).  No atomics of any kind.
constexpr int ST = 64;          // rows per tile = lanes of the one wave
constexpr int S_MAX_PART = 2048;

// The softened teacher distribution of one teacher row t (tm = its maximum): q_c = soft_e(c) / sum_c soft_e(c), the sum
// ascending in c.  The forward and the backward form q from this one expression.
__device__ __forceinline__ float soft_e(const float* t, int c, float tm, float inv_t) { return expf((t[c] - tm) * inv_t); }

// sum_c q_c * v_c over one teacher row, v_c = lse - x_c
__device__ inline float soft_dot(const float* t, float tm, float inv_t, const float* x, float lse, int C) {
  float s = 0.f, n = 0.f;
  for (int c = 0; c < C; c++) {
    const float e = soft_e(t, c, tm, inv_t);
    s += e;
    n += e * (lse - x[c]);
  }
  return n / s;
}

// The tile of k_ce2s_*: tile = [HAS_B ? 3 : 2][ST][pitch] holds the logits rows and, for the tail rows [h, rows) alone, the teacher
// rows (row0 + r - P) at the same r; h = tile_head(P, row0, rows).  The caller synchronises.
template <bool HAS_B>
__device__ __forceinline__ void stage_ce2s(float* tile, const RowTile& t, int h, int64_t P, int C, int pitch,
                                           const float* __restrict__ logits, int ld, const float* __restrict__ ta, int ld_a,
                                           const float* __restrict__ tb, int ld_b) {
  stage_rows<ST>(tile, logits + t.row0 * ld, ld, t.rows, C, pitch);
  if (h < t.rows) {
    const int64_t t0 = t.row0 + h - P;
    stage_rows<ST>(tile + (ST + h) * pitch, ta + t0 * ld_a, ld_a, t.rows - h, C, pitch);
    if (HAS_B) stage_rows<ST>(tile + (2 * ST + h) * pitch, tb + t0 * ld_b, ld_b, t.rows - h, C, pitch);
  }
}

// partial[b] = (sum w*nll, sum w) of the head, (sum of the kept rows' soft cross entropies, kept rows) of the tail.  RW
// (mm_ce2s_*_w): row_w[N - P] scales a kept row's term and its gradient row, not the count K.
template <bool HAS_B, bool CLS, bool RW>
__global__ __launch_bounds__(ST) void k_ce2s_fwd(const float* __restrict__ logits, int ld, int64_t N, int64_t P, int C,
                                                  const int64_t* __restrict__ labels0, const float* __restrict__ weight0, int64_t ignore,
                                                  const float* __restrict__ ta, int ld_a, const float* __restrict__ tb, int ld_b,
                                                  float inv_t, float thr, const float* __restrict__ thr_cls,
                                                  const float* __restrict__ row_w, double* __restrict__ partial) {
  extern __shared__ float tile[];  // [HAS_B ? 3 : 2][ST][pitch]
  const int pitch = C | 1;
  float* sx = tile;
  float* sa = tile + ST * pitch;
  float* sb = tile + 2 * ST * pitch;  // never touched without HAS_B
  double sl0 = 0.0, sw0 = 0.0, sl1 = 0.0;
  long long k1 = 0;
  const int64_t ntiles = (N + ST - 1) / ST;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const RowTile tl = row_tile<ST>(t, N);
    const int64_t row0 = tl.row0;
    const int rows = tl.rows, h = tile_head(P, row0, rows);
    __syncthreads();  // the previous tile's rows have been read
    stage_ce2s<HAS_B>(tile, tl, h, P, C, pitch, logits, ld, ta, ld_a, tb, ld_b);
    __syncthreads();
    const int r = threadIdx.x;
    const float* x = sx + r * pitch;
    if (r < h) {
      const int64_t y = labels0 ? labels0[row0 + r] : ignore;
      if (labels0 && label_counted(y, ignore, C)) {
        const RowLse l = row_lse(x, C);
        const float nll = (l.m + logf(l.s)) - x[y];
        const float w = weight0 ? weight0[y] : 1.f;
        sl0 += (double)(w * nll);
        sw0 += (double)w;
      }
    } else if (r < rows) {
      const float* a = sa + r * pitch;
      const float* b = sb + r * pitch;
      const MMPointPred pr = mm_point_predict<HAS_B>(a, b, C);
      // CLS (mm_ce2s_*_cls): the threshold of the row's own class.  A NaN confidence (or the ensemble's -1 of a non-finite row)
      // is never kept
      if ((HAS_B ? pr.pe : pr.pa) >= (CLS ? thr_cls[HAS_B ? pr.ie : pr.ia] : thr)) {
        const RowLse l = row_lse(x, C);
        const float lse = l.m + logf(l.s);
        float v = soft_dot(a, a[pr.ia], inv_t, x, lse, C);
        if (HAS_B) v = 0.5f * (v + soft_dot(b, b[pr.ib], inv_t, x, lse, C));
        sl1 += (double)(RW ? row_w[row0 + r - P] * v : v);
        k1 += 1;
      }
    }
  }
  const double a0 = wave_sum(sl0), b0 = wave_sum(sw0), a1 = wave_sum(sl1), b1 = wave_sum((double)k1);
  if (threadIdx.x == 0) {
    double* o = partial + 4 * (int64_t)blockIdx.x;
    o[0] = a0, o[1] = b0, o[2] = a1, o[3] = b1;
  }
}

// head: a / b (0/0 = nan, as k_ce_finalize) or 0 when unlabelled; tail: the mean over the K kept rows, 0 when K == 0
__global__ __launch_bounds__(64) void k_ce2s_finalize(const double* __restrict__ partial, int nb, int head_labelled,
                                                       float* __restrict__ out /*[4]: loss0, sum_w0, loss1, K*/,
                                                       int64_t* __restrict__ kept) {
  double v[4];
  sum_partials<4>(partial, nb, threadIdx.x, v);
  if (threadIdx.x == 0) {
    out[0] = head_labelled ? (float)(v[0] / v[1]) : 0.f;
    out[1] = (float)v[1];
    out[2] = v[3] > 0.0 ? (float)(v[2] / v[3]) : 0.f;
    out[3] = (float)v[3];
    if (kept) kept[0] = (int64_t)v[3];  // integer-valued partials: exact
  }
}

// One tile per workgroup, every row written once: the gradient rows are formed in place in the staged logits tile and leave it
// with consecutive lanes on consecutive addresses.  Head: gout[0] * w[y] / sum_w * (softmax - onehot), as k_ce_bwd; kept tail
// rows: gout[1] / K * (softmax - q), RW: times row_w of the row, q recomputed from the teacher rows; every other row: zeros.
template <bool HAS_B, bool CLS, bool RW>
__global__ __launch_bounds__(ST) void k_ce2s_bwd(const float* __restrict__ logits, int ld, int64_t N, int64_t P, int C,
                                                  const int64_t* __restrict__ labels0, const float* __restrict__ weight0, int64_t ignore,
                                                  const float* __restrict__ ta, int ld_a, const float* __restrict__ tb, int ld_b,
                                                  float inv_t, float thr, const float* __restrict__ thr_cls,
                                                  const float* __restrict__ row_w, const float* __restrict__ stats,
                                                  const float* __restrict__ gout, float* __restrict__ dlogits, int ld_d) {
  extern __shared__ float tile[];  // [HAS_B ? 3 : 2][ST][pitch]
  const int pitch = C | 1;
  float* sx = tile;
  float* sa = tile + ST * pitch;
  float* sb = tile + 2 * ST * pitch;
  const RowTile tl = row_tile<ST>(blockIdx.x, N);
  const int64_t row0 = tl.row0;
  const int rows = tl.rows, h = tile_head(P, row0, rows);
  stage_ce2s<HAS_B>(tile, tl, h, P, C, pitch, logits, ld, ta, ld_a, tb, ld_b);
  __syncthreads();
  const int r = threadIdx.x;
  if (r < rows) {
    float* x = sx + r * pitch;
    bool live;
    int y = -1;
    float k = 0.f;
    MMPointPred pr;
    const float* a = sa + r * pitch;
    const float* b = sb + r * pitch;
    if (r < h) {
      const int64_t yl = labels0 ? labels0[row0 + r] : ignore;
      live = labels0 && label_counted(yl, ignore, C);
      if (live) {
        y = (int)yl;
        k = gout[0] * (weight0 ? weight0[y] : 1.f) / stats[1];
      }
    } else {
      pr = mm_point_predict<HAS_B>(a, b, C);
      live = (HAS_B ? pr.pe : pr.pa) >= (CLS ? thr_cls[HAS_B ? pr.ie : pr.ia] : thr);
      if (live) k = RW ? gout[1] / stats[3] * row_w[row0 + r - P] : gout[1] / stats[3];
    }
    if (!live) {
      for (int c = 0; c < C; c++) x[c] = 0.f;
    } else {
      const RowLse l = row_lse(x, C);
      const float m = l.m, inv = 1.f / l.s;
      if (r < h) {
        ce_grad_row(x, x, C, m, inv, k, y);
      } else {
        const float ma = a[pr.ia];
        float za = 0.f, zb = 1.f, mb = 0.f;
        for (int c = 0; c < C; c++) za += soft_e(a, c, ma, inv_t);
        if (HAS_B) {
          mb = b[pr.ib], zb = 0.f;
          for (int c = 0; c < C; c++) zb += soft_e(b, c, mb, inv_t);
        }
        for (int c = 0; c < C; c++) {
          float q = soft_e(a, c, ma, inv_t) / za;
          if (HAS_B) q = 0.5f * (q + soft_e(b, c, mb, inv_t) / zb);
          x[c] = k * (expf(x[c] - m) * inv - q);
        }
      }
    }
  }
  __syncthreads();
  unstage_rows<ST>(dlogits + row0 * ld_d, ld_d, sx, rows, C, pitch);
}

// partial[b] = sum_i sum_c q_ic (log q_ic - log p_ic)
__global__ __launch_bounds__(T) void k_kl_fwd(const float* __restrict__ pred, int ld_p, const float* __restrict__ tgt,
                                               int ld_t, int64_t N, int C, double* __restrict__ partial) {
  __shared__ double red[T];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < N; i += (int64_t)gridDim.x * T) {
    const float* p = pred + i * ld_p;
    const float* t = tgt + i * ld_t;
    const RowLse rp = row_lse(p, C), rt = row_lse(t, C);
    float lp = rp.m + logf(rp.s), lt = rt.m + logf(rt.s);
    float r = 0.f;
    for (int c = 0; c < C; c++) {
      float lq = t[c] - lt;
      r += expf(lq) * (lq - (p[c] - lp));
    }
    acc += (double)r;
  }
  double a = block_sum<T>(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = a;
}

__global__ __launch_bounds__(64) void k_kl_finalize(const double* __restrict__ partial, int nb, int64_t N, float* __restrict__ out) {
  double a[1];
  sum_partials<1>(partial, nb, threadIdx.x, a);
  if (threadIdx.x == 0) out[0] = (float)(a[0] / (double)N);
}

// dpred = gscale/N * (softmax(pred) - softmax(tgt))
__global__ __launch_bounds__(T) void k_kl_bwd(const float* __restrict__ pred, int ld_p, const float* __restrict__ tgt,
                                               int ld_t, int64_t N, int C, const float* __restrict__ gout,
                                               float* __restrict__ dpred, int ld_d) {
  int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
  if (i >= N) return;
  const float* p = pred + i * ld_p;
  const float* t = tgt + i * ld_t;
  const RowLse rp = row_lse(p, C), rt = row_lse(t, C);
  float k = gout[0] / (float)N, ip = 1.f / rp.s, it = 1.f / rt.s;
  for (int c = 0; c < C; c++) dpred[i * ld_d + c] = k * (expf(p[c] - rp.m) * ip - expf(t[c] - rt.m) * it);
}

// ---- evaluation (train.py:297-339): argmax of the 2D logits, of the 3D logits and of the softmax average, three
// confusion matrices [target][pred] over the rows whose label != ignore.  Integer counts: order independent.
__global__ __launch_bounds__(T) void k_eval_confusion(const float* __restrict__ l2, int ld2, const float* __restrict__ l3, int ld3,
                                                       const int64_t* __restrict__ labels, int64_t N, int C, int64_t ignore,
                                                       unsigned long long* __restrict__ cm /*[3][C][C]*/) {
  extern __shared__ unsigned int hist[];  // [3][C][C]
  for (int i = threadIdx.x; i < 3 * C * C; i += T) hist[i] = 0u;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < N; i += (int64_t)gridDim.x * T) {
    int64_t y = labels[i];
    if (!label_counted(y, ignore, C)) continue;
    const MMPointPred r = mm_point_predict<true>(l2 + i * ld2, l3 + i * ld3, C);  // pointpred.h: shared with the pseudo-label export
    atomicAdd(&hist[(0 * C + (int)y) * C + r.ia], 1u);
    atomicAdd(&hist[(1 * C + (int)y) * C + r.ib], 1u);
    atomicAdd(&hist[(2 * C + (int)y) * C + r.ie], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * C * C; i += T)
    if (hist[i]) atomicAdd(&cm[i], (unsigned long long)hist[i]);
}
}  // namespace

extern "C" {

size_t mm_loss_ws_bytes() { return mm_align((size_t)MAX_PART * 2 * sizeof(double)) + 256; }

static inline int loss_blocks(int64_t N) {
  int64_t nb = mm_cdiv(N > 0 ? N : 1, (int64_t)T * 4);
  return (int)(nb > MAX_PART ? MAX_PART : nb);
}

// stats[0] = loss, stats[1] = sum of weights of the non-ignored rows
int mm_ce_fwd(const float* logits, int ld, const int64_t* labels, const float* weight, int64_t N, int C, int64_t ignore_index,
              float* stats, void* ws, size_t ws_bytes, hipStream_t s) {
  MM_CHECK_ARG(C > 0 && C <= MAXC && ld >= C, "ce: bad C");
  MM_CHECK_ARG(N >= 0, "ce: negative N");
  MM_CHECK_ARG(stats && ws && ((logits && labels) || N == 0), "ce: null logits, labels, stats or workspace");
  if (ws_bytes < (size_t)MAX_PART * 2 * sizeof(double)) {
    mm_set_error("ce: workspace too small");
    return MM_ERR_WORKSPACE;
  }
  int nb = loss_blocks(N);
  hipLaunchKernelGGL(k_ce_fwd<1>, dim3(nb), dim3(T), 0, s, logits, ld, N, N, C, labels, weight, nullptr, nullptr, ignore_index,
                     nullptr, (double*)ws);
  hipLaunchKernelGGL(k_ce_finalize<1>, dim3(1), dim3(64), 0, s, (const double*)ws, nb, 1, 0, stats);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_ce_bwd(const float* logits, int ld, const int64_t* labels, const float* weight, int64_t N, int C, int64_t ignore_index,
              const float* stats, const float* grad_out, float* dlogits, int ld_d, hipStream_t s) {
  MM_CHECK_ARG(C > 0 && C <= MAXC && ld >= C && ld_d >= C, "ce: bad C");
  MM_CHECK_ARG(N >= 0, "ce: negative N");
  if (N == 0) return MM_OK;
  MM_CHECK_ARG(logits && labels && stats && grad_out && dlogits, "ce: null logits, labels, stats, grad_out or dlogits");
  hipLaunchKernelGGL(k_ce_bwd<1>, dim3((unsigned)mm_cdiv(N, T)), dim3(T), 0, s, logits, ld, N, N, C, labels, weight, nullptr, nullptr,
                     ignore_index, nullptr, stats, grad_out, dlogits, ld_d);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

size_t mm_ce2_ws_bytes() { return mm_align((size_t)MAX_PART * 4 * sizeof(double)) + 256; }

// stats[4] = loss and weight sum of rows [0, P), then of rows [P, N); see include/mm2d3d.h.  row_w != NULL (mm_ce2_*_w): the
// RW kernels; NULL launches the kernels of the plain entry points.
int mm_ce2_fwd_w(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                 const int64_t* labels1, const float* weight1, int64_t ignore_index, int zero_if_empty, const float* row_w, float* stats,
                 void* ws, size_t ws_bytes, hipStream_t s) {
  MM_CHECK_ARG(C > 0 && C <= MAXC && ld >= C, "ce2: bad C");
  MM_CHECK_ARG(N >= 0 && P >= 0 && P <= N, "ce2: the split must lie in [0, N]");
  if (ws_bytes < (size_t)MAX_PART * 4 * sizeof(double)) {
    mm_set_error("ce2: workspace too small");
    return MM_ERR_WORKSPACE;
  }
  int nb = loss_blocks(N);
  if (row_w)
    hipLaunchKernelGGL((k_ce_fwd<2, true>), dim3(nb), dim3(T), 0, s, logits, ld, N, P, C, labels0, weight0, labels1, weight1,
                       ignore_index, row_w, (double*)ws);
  else
    hipLaunchKernelGGL(k_ce_fwd<2>, dim3(nb), dim3(T), 0, s, logits, ld, N, P, C, labels0, weight0, labels1, weight1, ignore_index,
                       row_w, (double*)ws);
  hipLaunchKernelGGL(k_ce_finalize<2>, dim3(1), dim3(64), 0, s, (const double*)ws, nb, (labels0 ? 1 : 0) | (labels1 ? 2 : 0),
                     zero_if_empty, stats);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_ce2_bwd_w(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                 const int64_t* labels1, const float* weight1, int64_t ignore_index, const float* row_w, const float* stats,
                 const float* grad_out, float* dlogits, int ld_d, hipStream_t s) {
  MM_CHECK_ARG(C > 0 && C <= MAXC && ld >= C && ld_d >= C, "ce2: bad C");
  MM_CHECK_ARG(N >= 0 && P >= 0 && P <= N, "ce2: the split must lie in [0, N]");
  if (N == 0) return MM_OK;
  const dim3 grid((unsigned)mm_cdiv(N, T));
  if (row_w)
    hipLaunchKernelGGL((k_ce_bwd<2, true>), grid, dim3(T), 0, s, logits, ld, N, P, C, labels0, weight0, labels1, weight1, ignore_index,
                       row_w, stats, grad_out, dlogits, ld_d);
  else
    hipLaunchKernelGGL(k_ce_bwd<2>, grid, dim3(T), 0, s, logits, ld, N, P, C, labels0, weight0, labels1, weight1, ignore_index, row_w,
                       stats, grad_out, dlogits, ld_d);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_ce2_fwd(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
               const int64_t* labels1, const float* weight1, int64_t ignore_index, int zero_if_empty, float* stats, void* ws,
               size_t ws_bytes, hipStream_t s) {
  return mm_ce2_fwd_w(logits, ld, N, P, C, labels0, weight0, labels1, weight1, ignore_index, zero_if_empty, nullptr, stats, ws, ws_bytes, s);
}

int mm_ce2_bwd(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
               const int64_t* labels1, const float* weight1, int64_t ignore_index, const float* stats, const float* grad_out,
               float* dlogits, int ld_d, hipStream_t s) {
  return mm_ce2_bwd_w(logits, ld, N, P, C, labels0, weight0, labels1, weight1, ignore_index, nullptr, stats, grad_out, dlogits, ld_d, s);
}

size_t mm_ce2s_ws_bytes() { return mm_align((size_t)S_MAX_PART * 4 * sizeof(double)) + 256; }

// thr_cls != NULL (mm_ce2s_*_cls): thr_cls[C] on the device replaces the scalar thr
static int ce2s_check(const float* logits, int ld, int64_t N, int64_t P, int C, const float* ta, int ld_a, const float* tb, int ld_b,
                      float temperature, float thr, const float* thr_cls, bool cls) {
  MM_CHECK_ARG(C > 0 && C <= MAXC && ld >= C, "ce2s: bad C");
  MM_CHECK_ARG(N >= 0 && P >= 0 && P <= N && N <= (int64_t)ST * 0x7fffffff, "ce2s: the split must lie in [0, N]");
  MM_CHECK_ARG(logits || N == 0, "ce2s: null logits");
  MM_CHECK_ARG(ta || (P == N && !tb), "ce2s: tail rows without teacher logits");
  MM_CHECK_ARG((!ta || ld_a >= C) && (!tb || ld_b >= C), "ce2s: teacher row pitch below C");
  MM_CHECK_ARG(temperature > 0.f && temperature <= 3.0e38f, "ce2s: the temperature must be a finite number > 0");
  if (cls)
    MM_CHECK_ARG(thr_cls, "ce2s: null class thresholds");
  else
    MM_CHECK_ARG(thr >= 0.f && thr <= 1.f, "ce2s: the threshold must lie in [0, 1]");
  return MM_OK;
}

// the kernel of (tb != NULL, cls, row_w != NULL): LAUNCH(HAS_B, CLS, RW)
#define MM_CE2S_DISPATCH_B(LAUNCH, CLS, RW) \
  do {                                      \
    if (tb) LAUNCH(true, CLS, RW);          \
    else LAUNCH(false, CLS, RW);            \
  } while (0)
#define MM_CE2S_DISPATCH_C(LAUNCH, RW)                \
  do {                                                \
    if (cls) MM_CE2S_DISPATCH_B(LAUNCH, true, RW);    \
    else MM_CE2S_DISPATCH_B(LAUNCH, false, RW);       \
  } while (0)
#define MM_CE2S_DISPATCH(LAUNCH)                      \
  do {                                                \
    if (row_w) MM_CE2S_DISPATCH_C(LAUNCH, true);      \
    else MM_CE2S_DISPATCH_C(LAUNCH, false);           \
  } while (0)

static int ce2s_fwd(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                    int64_t ignore_index, const float* ta, int ld_a, const float* tb, int ld_b, float temperature, float thr,
                    const float* thr_cls, bool cls, const float* row_w, float* stats, int64_t* kept, void* ws, size_t ws_bytes,
                    hipStream_t s) {
  if (int rc = ce2s_check(logits, ld, N, P, C, ta, ld_a, tb, ld_b, temperature, thr, thr_cls, cls)) return rc;
  MM_CHECK_ARG(stats, "ce2s: null stats");
  if (ws_bytes < (size_t)S_MAX_PART * 4 * sizeof(double)) {
    mm_set_error("ce2s: workspace too small");
    return MM_ERR_WORKSPACE;
  }
  int64_t nt = mm_cdiv(N > 0 ? N : 1, (int64_t)ST);
  const int nb = (int)(nt > S_MAX_PART ? S_MAX_PART : nt);
  const size_t lds = (size_t)(tb ? 3 : 2) * ST * (C | 1) * sizeof(float);
  const float inv_t = 1.f / temperature;
#define MM_CE2S_FWD(HAS_B, CLS, RW)                                                                                                  \
  hipLaunchKernelGGL((k_ce2s_fwd<HAS_B, CLS, RW>), dim3(nb), dim3(ST), lds, s, logits, ld, N, P, C, labels0, weight0, ignore_index, \
                     ta, ld_a, tb, ld_b, inv_t, thr, thr_cls, row_w, (double*)ws)
  MM_CE2S_DISPATCH(MM_CE2S_FWD);
#undef MM_CE2S_FWD
  hipLaunchKernelGGL(k_ce2s_finalize, dim3(1), dim3(64), 0, s, (const double*)ws, nb, labels0 ? 1 : 0, stats, kept);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

static int ce2s_bwd(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                    int64_t ignore_index, const float* ta, int ld_a, const float* tb, int ld_b, float temperature, float thr,
                    const float* thr_cls, bool cls, const float* row_w, const float* stats, const float* grad_out, float* dlogits,
                    int ld_d, hipStream_t s) {
  if (int rc = ce2s_check(logits, ld, N, P, C, ta, ld_a, tb, ld_b, temperature, thr, thr_cls, cls)) return rc;
  MM_CHECK_ARG(ld_d >= C, "ce2s: gradient row pitch below C");
  if (N == 0) return MM_OK;
  MM_CHECK_ARG(stats && grad_out && dlogits, "ce2s: null stats, grad_out or dlogits");
  const unsigned nb = (unsigned)mm_cdiv(N, (int64_t)ST);
  const size_t lds = (size_t)(tb ? 3 : 2) * ST * (C | 1) * sizeof(float);
  const float inv_t = 1.f / temperature;
#define MM_CE2S_BWD(HAS_B, CLS, RW)                                                                                                  \
  hipLaunchKernelGGL((k_ce2s_bwd<HAS_B, CLS, RW>), dim3(nb), dim3(ST), lds, s, logits, ld, N, P, C, labels0, weight0, ignore_index, \
                     ta, ld_a, tb, ld_b, inv_t, thr, thr_cls, row_w, stats, grad_out, dlogits, ld_d)
  MM_CE2S_DISPATCH(MM_CE2S_BWD);
#undef MM_CE2S_BWD
  MM_LAUNCH_CHECK();
  return MM_OK;
}

// stats[4] = head loss, head weight sum, tail loss, kept rows K (as a float); kept[0] = K exactly; see include/mm2d3d.h
int mm_ce2s_fwd(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                int64_t ignore_index, const float* ta, int ld_a, const float* tb, int ld_b, float temperature, float thr, float* stats,
                int64_t* kept, void* ws, size_t ws_bytes, hipStream_t s) {
  return ce2s_fwd(logits, ld, N, P, C, labels0, weight0, ignore_index, ta, ld_a, tb, ld_b, temperature, thr, nullptr, false, nullptr, stats,
                  kept, ws, ws_bytes, s);
}

int mm_ce2s_bwd(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                int64_t ignore_index, const float* ta, int ld_a, const float* tb, int ld_b, float temperature, float thr,
                const float* stats, const float* grad_out, float* dlogits, int ld_d, hipStream_t s) {
  return ce2s_bwd(logits, ld, N, P, C, labels0, weight0, ignore_index, ta, ld_a, tb, ld_b, temperature, thr, nullptr, false, nullptr,
                  stats, grad_out, dlogits, ld_d, s);
}

// the same pair with a threshold per class: a tail row is kept iff its confidence >= thr_cls[its arg-max class]
int mm_ce2s_fwd_cls(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                    int64_t ignore_index, const float* ta, int ld_a, const float* tb, int ld_b, float temperature, const float* thr_cls,
                    float* stats, int64_t* kept, void* ws, size_t ws_bytes, hipStream_t s) {
  return ce2s_fwd(logits, ld, N, P, C, labels0, weight0, ignore_index, ta, ld_a, tb, ld_b, temperature, 0.f, thr_cls, true, nullptr, stats,
                  kept, ws, ws_bytes, s);
}

int mm_ce2s_bwd_cls(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                    int64_t ignore_index, const float* ta, int ld_a, const float* tb, int ld_b, float temperature, const float* thr_cls,
                    const float* stats, const float* grad_out, float* dlogits, int ld_d, hipStream_t s) {
  return ce2s_bwd(logits, ld, N, P, C, labels0, weight0, ignore_index, ta, ld_a, tb, ld_b, temperature, 0.f, thr_cls, true, nullptr,
                  stats, grad_out, dlogits, ld_d, s);
}

// the same pair with row weights of the tail rows: thr_cls != NULL wins over thr; row_w == NULL: the kernels of the entry points above
int mm_ce2s_fwd_w(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                  int64_t ignore_index, const float* ta, int ld_a, const float* tb, int ld_b, float temperature, float thr,
                  const float* thr_cls, const float* row_w, float* stats, int64_t* kept, void* ws, size_t ws_bytes, hipStream_t s) {
  return ce2s_fwd(logits, ld, N, P, C, labels0, weight0, ignore_index, ta, ld_a, tb, ld_b, temperature, thr_cls ? 0.f : thr, thr_cls,
                  thr_cls != nullptr, row_w, stats, kept, ws, ws_bytes, s);
}

int mm_ce2s_bwd_w(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                  int64_t ignore_index, const float* ta, int ld_a, const float* tb, int ld_b, float temperature, float thr,
                  const float* thr_cls, const float* row_w, const float* stats, const float* grad_out, float* dlogits, int ld_d,
                  hipStream_t s) {
  return ce2s_bwd(logits, ld, N, P, C, labels0, weight0, ignore_index, ta, ld_a, tb, ld_b, temperature, thr_cls ? 0.f : thr, thr_cls,
                  thr_cls != nullptr, row_w, stats, grad_out, dlogits, ld_d, s);
}

int mm_kl_fwd(const float* pred, int ld_p, const float* tgt, int ld_t, int64_t N, int C, float* loss, void* ws, size_t ws_bytes,
              hipStream_t s) {
  MM_CHECK_ARG(C > 0 && C <= MAXC && ld_p >= C && ld_t >= C, "kl: bad C");
  MM_CHECK_ARG(N >= 0, "kl: negative N");
  MM_CHECK_ARG(loss && ws && ((pred && tgt) || N == 0), "kl: null pred, tgt, loss or workspace");
  if (ws_bytes < (size_t)MAX_PART * sizeof(double)) {
    mm_set_error("kl: workspace too small");
    return MM_ERR_WORKSPACE;
  }
  int nb = loss_blocks(N);
  hipLaunchKernelGGL(k_kl_fwd, dim3(nb), dim3(T), 0, s, pred, ld_p, tgt, ld_t, N, C, (double*)ws);
  hipLaunchKernelGGL(k_kl_finalize, dim3(1), dim3(64), 0, s, (const double*)ws, nb, N, loss);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_kl_bwd(const float* pred, int ld_p, const float* tgt, int ld_t, int64_t N, int C, const float* grad_out, float* dpred,
              int ld_d, hipStream_t s) {
  MM_CHECK_ARG(C > 0 && C <= MAXC && ld_p >= C && ld_t >= C && ld_d >= C, "kl: bad C");
  MM_CHECK_ARG(N >= 0, "kl: negative N");
  if (N == 0) return MM_OK;
  MM_CHECK_ARG(pred && tgt && grad_out && dpred, "kl: null pred, tgt, grad_out or dpred");
  hipLaunchKernelGGL(k_kl_bwd, dim3((unsigned)mm_cdiv(N, T)), dim3(T), 0, s, pred, ld_p, tgt, ld_t, N, C, grad_out, dpred, ld_d);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

// cm int64 [3][C][C] (2D, 3D, softmax-average ensemble), accumulated (caller zeroes it at the start of an epoch)
int mm_eval_confusion(const float* logits2d, int ld2, const float* logits3d, int ld3, const int64_t* labels, int64_t N, int C,
                      int64_t ignore_index, int64_t* cm, hipStream_t s) {
  MM_CHECK_ARG(C > 0 && C <= MAXC && ld2 >= C && ld3 >= C, "eval_confusion: bad C");
  MM_CHECK_ARG(N >= 0, "eval_confusion: negative N");
  if (N == 0) return MM_OK;
  MM_CHECK_ARG(logits2d && logits3d && labels && cm, "eval_confusion: null logits, labels or cm");
  int nb = (int)mm_cdiv(N, (int64_t)T * 8);
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(k_eval_confusion, dim3(nb), dim3(T), (size_t)3 * C * C * sizeof(unsigned int), s, logits2d, ld2, logits3d, ld3,
                     labels, N, C, ignore_index, (unsigned long long*)cm);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"
