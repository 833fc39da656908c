// Pseudo labels for the self-training round (EXP/train.py:297-339 -> the files lib/dataset/*_dataloader.py read back):
//   mm_pselab_predict   per point: max and argmax of softmax(2D logits), of softmax(3D logits) and of their average
//   mm_teacher_labels   the same per-point expression, written as the int64 training labels of both heads (a mean teacher that
//                       labels the target batch inside the step), with an optional confidence threshold and kept counts
//   mm_teacher_labels_cls  the same launch with one threshold per output and class, read from the device
//   mm_pl_adapt         the self-adaptive per-class thresholds (FreeMatch): running confidence and class mass of both outputs,
//                       kept on the device and updated from every target batch; two launches, no atomics, no host read
//   mm_pl_agree         per row the agreement of the 2D and the 3D prediction, w = exp(-beta * half the Jeffreys divergence of the
//                       two softmaxes): the row weights of the pseudo-label losses; two launches, no atomics, no host read
//   mm_pselab_refine    lib/utils/refine_pseudo_labels.py, exact: per class the lower median of the confidences by a
//                       most-significant-digit radix select (four 8-bit passes over the order-preserving uint32 image of the
//                       floats), threshold min(median, 0.9f), labels below it become ignore_label
// Counts are integers and are summed with integer atomics: the result does not depend on the order of the additions.
// The tile geometry, the staging, the counted rows of a workgroup, the column sums of a staged tile, the one-workgroup finish and
// the workspace of the statistics pass are rows.h's (row_tile, stage_rows, wave_count / block_count, col_sum, sum_partial,
// stats_ws), shared with infomax.hip and loss.hip: the kernels here hold what is particular to each.
#include "common.h"
#include "pointpred.h"
#include "rows.h"

namespace {
constexpr int PT = 128;      // points per workgroup of the prediction kernel
constexpr int T = 256;
constexpr int RADIX = 256;   // 8 bits per pass
constexpr int MAX_BLOCKS = 2048;

// ---- prediction.  The [rows, C] blocks of both logit matrices go through LDS (stage_rows of rows.h: coalesced copies, then each
// lane reads its own row, pitched to an odd number of words): tile = [HAS3 ? 2 : 1][PT][pitch].  The caller synchronises.
template <bool HAS3 = true>
__device__ __forceinline__ void stage_pair(float* tile, const float* __restrict__ l2, int ld2, const float* __restrict__ l3, int ld3,
                                           const RowTile& t, int C, int pitch) {
  stage_rows<PT>(tile, l2 + t.row0 * ld2, ld2, t.rows, C, pitch);
  if (HAS3) stage_rows<PT>(tile + PT * pitch, l3 + t.row0 * ld3, ld3, t.rows, C, pitch);
}

template <bool HAS3>
__global__ __launch_bounds__(PT) void k_pselab_predict(const float* __restrict__ l2, int ld2, const float* __restrict__ l3, int ld3,
                                                        int64_t N, int C, float* __restrict__ p2, uint8_t* __restrict__ y2,
                                                        float* __restrict__ p3, uint8_t* __restrict__ y3, float* __restrict__ pe,
                                                        uint8_t* __restrict__ ye) {
  extern __shared__ float tile[];  // [HAS3 ? 2 : 1][PT][pitch]
  const int pitch = C | 1;
  const RowTile t = row_tile<PT>(blockIdx.x, N);
  float* ta = tile;
  float* tb = tile + PT * pitch;
  stage_pair<HAS3>(tile, l2, ld2, l3, ld3, t, C, pitch);
  __syncthreads();
  if ((int)threadIdx.x >= t.rows) return;
  const MMPointPred r = mm_point_predict<HAS3>(ta + threadIdx.x * pitch, tb + threadIdx.x * pitch, C);
  const int64_t i = t.row0 + threadIdx.x;
  p2[i] = r.pa;
  y2[i] = (uint8_t)r.ia;
  if (HAS3) {
    p3[i] = r.pb;
    y3[i] = (uint8_t)r.ib;
    pe[i] = r.pe;
    ye[i] = (uint8_t)r.ie;
  }
}

// ---- online labels of a mean teacher (mm2d3d_amd/train.py pseudo_label_source="teacher"): the staging and the per-row expression
// of k_pselab_predict, written as the int64 labels cross_entropy_pair reads.  ENS: both outputs take the softmax average.
// thr >= 0: a label whose confidence is not >= thr (a NaN confidence included) becomes `ignore`.  kept[2]: labels that were
// kept, per output - a ballot per wave, the two waves' counts through two words of the tile (its rows are dead by then), one
// 64-bit integer atomic per workgroup and counter.
// CLS (mm_teacher_labels_cls): thr_cls[2][C] on the device replaces thr - output o keeps a row iff p >= thr_cls[o][y].
template <bool ENS, bool CLS>
__global__ __launch_bounds__(PT) void k_teacher_labels(const float* __restrict__ l2, int ld2, const float* __restrict__ l3, int ld3,
                                                        int64_t N, int C, float thr, const float* __restrict__ thr_cls, int64_t ignore,
                                                        int64_t* __restrict__ y2, int64_t* __restrict__ y3, float* __restrict__ p2,
                                                        float* __restrict__ p3, unsigned long long* __restrict__ kept) {
  extern __shared__ float tile[];  // [2][PT][pitch]
  __shared__ float th[CLS ? 2 * MM_PRED_MAXC : 1];
  if (CLS && (int)threadIdx.x < 2 * C) th[threadIdx.x] = thr_cls[threadIdx.x];
  const int pitch = C | 1;
  const RowTile t = row_tile<PT>(blockIdx.x, N);
  float* ta = tile;
  float* tb = tile + PT * pitch;
  stage_pair(tile, l2, ld2, l3, ld3, t, C, pitch);
  __syncthreads();
  bool k2 = false, k3 = false;
  if ((int)threadIdx.x < t.rows) {
    const MMPointPred r = mm_point_predict<true>(ta + threadIdx.x * pitch, tb + threadIdx.x * pitch, C);
    const float pa = ENS ? r.pe : r.pa, pb = ENS ? r.pe : r.pb;
    const int ia = ENS ? r.ie : r.ia, ib = ENS ? r.ie : r.ib;
    k2 = CLS ? pa >= th[ia] : (thr < 0.f || pa >= thr);
    k3 = CLS ? pb >= th[C + ib] : (thr < 0.f || pb >= thr);
    const int64_t i = t.row0 + threadIdx.x;
    y2[i] = k2 ? (int64_t)ia : ignore;
    y3[i] = k3 ? (int64_t)ib : ignore;
    if (p2) p2[i] = pa;
    if (p3) p3[i] = pb;
  }
  if (!kept) return;  // uniform
  const unsigned wn[2] = {wave_count(k2), wave_count(k3)};
  __syncthreads();  // every lane has read its rows
  const long long n = block_count<PT>(wn, (unsigned*)tile);
  if (n) atomicAdd(&kept[threadIdx.x], (unsigned long long)n);  // n != 0: thread 0 or 1
}

// ---- self-adaptive per-class thresholds (mm_pl_adapt; include/mm2d3d.h has the definition).  Per output o the state is tau_o
// and pt_o[c]; a batch contributes mean p and mean q[c] over its counted rows (p >= 0 in float32: the rows threshold 0 keeps).
// k_pl_stats: a capped grid walks the 128-row tiles, staged as in k_teacher_labels.  A lane that kept 2 * (1 + C) accumulators
// indexed by a runtime c would spill them, so each lane writes its row's q values back INTO the staged tile (zeros for a row that
// is not counted) and its confidences into conf[]; then thread (o, j) sums column j of output o over the tile's rows in ascending
// order into ONE fp64 accumulator that it carries across the workgroup's tiles (col_sum of rows.h).  Row counts are ballots,
// integers throughout (wave_count, block_count).
// k_pl_update: one workgroup of ROWS_FT threads sums the <= ROWS_MAX_WG partials per quantity (sum_partial of rows.h:
// a wave per quantity, sixteen waves share the 2 * (1 + C) + 2 quantities), applies the update in place and writes the
// thresholds.  No atomics of any kind.  The walk, the finish and the workspace (stats_ws) are those of infomax.hip.
template <bool ENS>
__global__ __launch_bounds__(PT) void k_pl_stats(const float* __restrict__ l2, int ld2, const float* __restrict__ l3, int ld3, int64_t N,
                                                  int C, double* __restrict__ psum /*[grid][2][1 + C]*/,
                                                  long long* __restrict__ pcnt /*[grid][2]*/) {
  extern __shared__ float tile[];  // [2][PT][pitch], then conf [2][PT]
  __shared__ unsigned wcnt[PT / 64 * 2];
  const int pitch = C | 1;
  float* ta = tile;
  float* tb = tile + PT * pitch;
  float* conf = tile + 2 * PT * pitch;
  const int K = 1 + C;
  const int o = (int)threadIdx.x / K, j = (int)threadIdx.x - o * K;  // the column this thread sums (threads < 2 * K)
  double acc = 0.0;
  unsigned wn[2] = {0, 0};  // per wave: every lane holds the wave's counts (a workgroup sees at most 2^28 rows: mm_pl_adapt)
  const unsigned ntiles = (unsigned)((N + PT - 1) / PT);  // <= 2^31 - 1 (mm_pl_adapt), so t + gridDim.x does not wrap
  for (unsigned t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const RowTile tl = row_tile<PT>(t, N);
    __syncthreads();  // the previous tile's columns have been summed
    stage_pair(tile, l2, ld2, l3, ld3, tl, C, pitch);
    __syncthreads();
    bool k2 = false, k3 = false;
    if ((int)threadIdx.x < tl.rows) {
      float* a = ta + threadIdx.x * pitch;
      float* b = tb + threadIdx.x * pitch;
      const MMPointPred r = mm_point_predict<true>(a, b, C);
      const float pa = ENS ? r.pe : r.pa, pb = ENS ? r.pe : r.pb;
      k2 = pa >= 0.f;  // a NaN confidence, or the ensemble's -1 of a non-finite row, is not counted
      k3 = pb >= 0.f;
      // the per-class values mm_point_predict forms: its maxima are a[ia] / b[ib], its sums run ascending in c
      const float ma = a[r.ia], mb = b[r.ib];
      float sa = 0.f, sb = 0.f;
#pragma unroll 1
      for (int c = 0; c < C; c++) {
        sa += expf(a[c] - ma);
        sb += expf(b[c] - mb);
      }
#pragma unroll 1
      for (int c = 0; c < C; c++) {
        const float qa = expf(a[c] - ma) / sa, qb = expf(b[c] - mb) / sb;
        const float q2 = ENS ? 0.5f * (qa + qb) : qa, q3 = ENS ? q2 : qb;
        a[c] = k2 ? q2 : 0.f;
        b[c] = k3 ? q3 : 0.f;
      }
      conf[threadIdx.x] = k2 ? pa : 0.f;
      conf[PT + threadIdx.x] = k3 ? pb : 0.f;
    }
    wn[0] += wave_count(k2);
    wn[1] += wave_count(k3);
    __syncthreads();
    if ((int)threadIdx.x < 2 * K) {
      if (j == 0) col_sum(acc, conf + o * PT, 1, tl.rows);
      else col_sum(acc, (o ? tb : ta) + (j - 1), pitch, tl.rows);
    }
  }
  if ((int)threadIdx.x < 2 * K) psum[(int64_t)blockIdx.x * 2 * K + threadIdx.x] = acc;
  const long long n = block_count<PT>(wn, wcnt);
  if (threadIdx.x < 2) pcnt[(int64_t)blockIdx.x * 2 + threadIdx.x] = n;
}

// state[2][1 + C] = (tau_o, pt_o[c]), count[2] = updates taken, thr[2][C] = float((pt_o[c] / max_c pt_o[c]) * tau_o) in fp64.
// An output without counted rows keeps its state and its count; its thresholds are written all the same.
__global__ __launch_bounds__(ROWS_FT) void k_pl_update(const double* __restrict__ psum, const long long* __restrict__ pcnt, int nb, int C,
                                                      double momentum, int warmup, double* __restrict__ state,
                                                      int64_t* __restrict__ count, float* __restrict__ thr) {
  __shared__ double tot[2 * (1 + MM_PRED_MAXC)];
  __shared__ long long cnt[2];
  __shared__ double cur[2 * (1 + MM_PRED_MAXC)];
  const int K = 1 + C, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int q = wave; q < 2 * K + 2; q += ROWS_FT / 64) {  // uniform per wave
    if (q < 2 * K) {
      const double v = sum_partial(psum, nb, 2 * K, q, lane);
      if (lane == 0) tot[q] = v;
    } else {
      const long long n = sum_partial(pcnt, nb, 2, q - 2 * K, lane);
      if (lane == 0) cnt[q - 2 * K] = n;
    }
  }
  __syncthreads();
  const int o = (int)threadIdx.x / K, j = (int)threadIdx.x - o * K;
  if ((int)threadIdx.x < 2 * K) {
    const long long n = cnt[o];
    double v = state[threadIdx.x];
    if (n > 0) {
      const int64_t t = count[o];
      double m = momentum;
      if (warmup) {
        const double w = (1.0 + (double)t) / (10.0 + (double)t);
        m = w < m ? w : m;
      }
      v = m * v + (1.0 - m) * (tot[threadIdx.x] / (double)n);
      state[threadIdx.x] = v;
    }
    cur[threadIdx.x] = v;
  }
  __syncthreads();  // every thread has read count[o]
  if ((int)threadIdx.x < 2 * K) {
    if (j == 0) {
      if (cnt[o] > 0) count[o] += 1;
    } else {
      const double* pt = cur + o * K + 1;
      double mx = pt[0];
      for (int c = 1; c < C; c++) mx = pt[c] > mx ? pt[c] : mx;
      thr[o * C + (j - 1)] = (float)((pt[j - 1] / mx) * cur[o * K]);
    }
  }
}

// ---- 2D/3D agreement weights (mm_pl_agree; include/mm2d3d.h has the definition): per row D = half the Jeffreys divergence of the
// two softmaxes and w = exp(-beta * D).  k_pl_agree: a capped grid walks the 128-row tiles, staged as in k_teacher_labels; a lane
// owns a row, writes its w and carries two fp64 sums (w over all its rows, D over its finite rows, rows ascending) across the
// workgroup's tiles; block_sum / block_count finish the workgroup.  k_pl_agree_final: one workgroup, a wave per quantity
// (sum_partial of rows.h).  No atomics of any kind; the walk and the workspace (stats_ws) are those of k_pl_stats.
constexpr int AGREE_FT = 256;  // threads of the finish: three quantities, a wave each

__global__ __launch_bounds__(PT) void k_pl_agree(const float* __restrict__ l2, int ld2, const float* __restrict__ l3, int ld3, int64_t N,
                                                  int C, float beta, float* __restrict__ w, double* __restrict__ psum /*[grid][2]*/,
                                                  long long* __restrict__ pcnt /*[grid]*/) {
  extern __shared__ float tile[];  // [2][PT][pitch]
  __shared__ double red[PT];
  __shared__ unsigned wcnt[PT / 64];
  const int pitch = C | 1;
  double sw = 0.0, sd = 0.0;
  unsigned wn[1] = {0};  // per wave: every lane holds the wave's count (N * C < 2^31: below 2^30 rows)
  const unsigned ntiles = (unsigned)((N + PT - 1) / PT);
  for (unsigned t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const RowTile tl = row_tile<PT>(t, N);
    __syncthreads();  // the previous tile's rows have been read
    stage_pair(tile, l2, ld2, l3, ld3, tl, C, pitch);
    __syncthreads();
    bool finite = false;
    if ((int)threadIdx.x < tl.rows) {
      const float* a = tile + threadIdx.x * pitch;
      const float* b = tile + (PT + threadIdx.x) * pitch;
      finite = row_finite(a, C) && row_finite(b, C);
      float wi = 0.f;
      if (finite) {
        const RowLse ra = row_lse(a, C), rb = row_lse(b, C);
        const float la = ra.m + logf(ra.s), lb = rb.m + logf(rb.s);
        float d = 0.f;
#pragma unroll 1
        for (int c = 0; c < C; c++) {
          const float dp = expf(a[c] - ra.m) / ra.s - expf(b[c] - rb.m) / rb.s;
          if (dp != 0.f) d += dp * ((a[c] - la) - (b[c] - lb));  // dp == 0: the limit 0 (a log ratio may be infinite for logits 2^128 apart)
        }
        d = fmaxf(0.5f * d, 0.f);  // every term is >= 0 up to rounding
        wi = expf(-beta * d);
        sw += (double)wi;
        sd += (double)d;
      }
      w[tl.row0 + threadIdx.x] = wi;
    }
    wn[0] += wave_count(finite);
  }
  const double a = block_sum<PT>(sw, red), b = block_sum<PT>(sd, red);
  if (threadIdx.x == 0) psum[2 * (int64_t)blockIdx.x] = a, psum[2 * (int64_t)blockIdx.x + 1] = b;
  const long long n = block_count<PT>(wn, wcnt);
  if (threadIdx.x == 0) pcnt[blockIdx.x] = n;
}

// stats[0] = sum w / N (0 when N == 0), stats[1] = sum D / n over the n finite rows (0 when n == 0), finite[0] = n
__global__ __launch_bounds__(AGREE_FT) void k_pl_agree_final(const double* __restrict__ psum, const long long* __restrict__ pcnt, int nb,
                                                             int64_t N, float* __restrict__ stats, int64_t* __restrict__ finite) {
  __shared__ double tot[2];
  __shared__ long long cnt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave < 2) {  // uniform per wave
    const double v = sum_partial(psum, nb, 2, wave, lane);
    if (lane == 0) tot[wave] = v;
  } else if (wave == 2) {
    const long long n = sum_partial(pcnt, nb, 1, 0, lane);
    if (lane == 0) cnt = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    stats[0] = N > 0 ? (float)(tot[0] / (double)N) : 0.f;
    stats[1] = cnt > 0 ? (float)(tot[1] / (double)cnt) : 0.f;
    if (finite) finite[0] = (int64_t)cnt;
  }
}

// ---- refinement
// ascending order of finite floats = ascending order of these keys (-0.0 sorts right below +0.0; the threshold is applied by a
// float comparison, to which the two zeros are equal, as they are to numpy's and torch's sort)
__device__ inline unsigned f2key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float key2f(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// pass p (0 .. 3) counts byte 3 - p of the keys whose higher bytes equal the class's prefix chosen so far
__global__ __launch_bounds__(T) void k_refine_hist(const float* __restrict__ probs, const int64_t* __restrict__ labels, int64_t N, int C,
                                                    int pass, const unsigned* __restrict__ prefix,
                                                    unsigned long long* __restrict__ ghist /*[C][RADIX]*/) {
  extern __shared__ unsigned lds[];  // [C][RADIX] counts, [C] prefixes
  unsigned* pre = lds + C * RADIX;
  for (int i = threadIdx.x; i < C * RADIX; i += T) lds[i] = 0u;
  if ((int)threadIdx.x < C) pre[threadIdx.x] = pass ? prefix[threadIdx.x] : 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const int64_t stride = (int64_t)gridDim.x * T;
  for (int64_t i0 = (int64_t)blockIdx.x * T + threadIdx.x; i0 < N; i0 += 4 * stride) {
    // four independent (probability, label) loads in flight per lane
    float p[4];
    int64_t y[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int64_t i = i0 + j * stride;
      y[j] = i < N ? labels[i] : (int64_t)-1;
      p[j] = i < N ? probs[i] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (y[j] < 0 || y[j] >= C) continue;
      const unsigned k = f2key(p[j]);
      // (k >> shift) >> 8: the bytes above this pass's (a shift by 32 is not defined)
      if (pass && ((k >> shift) >> 8) != pre[y[j]]) continue;
      atomicAdd(&lds[(int)y[j] * RADIX + ((k >> shift) & 255u)], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * RADIX; i += T)
    if (lds[i]) atomicAdd(&ghist[i], (unsigned long long)lds[i]);
}

// one workgroup: per class, the bucket that holds the remaining rank; zeroes the table for the next pass.
// pass 0 also turns the class's count n into the rank (n - 1) / 2 of its lower median; pass 3 writes the threshold.
__global__ __launch_bounds__(RADIX) void k_refine_select(unsigned long long* __restrict__ ghist, int C, int pass,
                                                          unsigned long long* __restrict__ rank, unsigned* __restrict__ prefix,
                                                          float* __restrict__ thr) {
  __shared__ unsigned long long scan[RADIX];
  const int t = threadIdx.x;
  for (int c = 0; c < C; c++) {
    const unsigned long long v = ghist[c * RADIX + t];
    ghist[c * RADIX + t] = 0ull;
    const unsigned long long want0 = pass ? rank[c] : 0ull;
    const unsigned pre0 = pass ? prefix[c] : 0u;
    __syncthreads();  // the previous class's readers of scan[] are done
    scan[t] = v;
    __syncthreads();
    for (int d = 1; d < RADIX; d <<= 1) {  // inclusive scan
      const unsigned long long add = t >= d ? scan[t - d] : 0ull;
      __syncthreads();
      scan[t] += add;
      __syncthreads();
    }
    const unsigned long long incl = scan[t], total = scan[RADIX - 1], excl = incl - v;
    if (total == 0ull) {  // the class does not occur, in any pass (for a class that occurs, later passes count a bucket that holds the rank)
      if (t == 0) {
        rank[c] = 0ull;
        prefix[c] = 0u;
        thr[c] = -INFINITY;  // nothing is below it
      }
      continue;  // uniform
    }
    const unsigned long long want = pass ? want0 : (total - 1ull) / 2ull;
    if (v > 0ull && excl <= want && want < incl) {  // exactly one thread
      const unsigned key = (pre0 << 8) | (unsigned)t;
      rank[c] = want - excl;
      prefix[c] = key;
      if (pass == 3) thr[c] = fminf(key2f(key), 0.9f);
    }
  }
}

__global__ __launch_bounds__(T) void k_refine_apply(const float* __restrict__ probs, const int64_t* __restrict__ labels, int64_t N, int C,
                                                     int64_t ignore, const float* __restrict__ thr, int64_t* __restrict__ out) {
  __shared__ float th[MM_PRED_MAXC];
  if ((int)threadIdx.x < C) th[threadIdx.x] = thr[threadIdx.x];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < N; i += (int64_t)gridDim.x * T) {
    const int64_t y = labels[i];
    out[i] = (y >= 0 && y < C && probs[i] < th[y]) ? ignore : y;
  }
}

struct RefineWs {
  unsigned long long* hist;
  unsigned long long* rank;
  unsigned* prefix;
  float* thr;
  size_t bytes;
};
inline RefineWs refine_ws(void* ws, int C) {
  RefineWs w;
  char* p = (char*)ws;
  size_t off = 0;
  w.hist = (unsigned long long*)(p + off), off += mm_align((size_t)C * RADIX * sizeof(unsigned long long));
  w.rank = (unsigned long long*)(p + off), off += mm_align((size_t)C * sizeof(unsigned long long));
  w.prefix = (unsigned*)(p + off), off += mm_align((size_t)C * sizeof(unsigned));
  w.thr = (float*)(p + off), off += mm_align((size_t)C * sizeof(float));
  w.bytes = off;
  return w;
}
}  // namespace

extern "C" {

int mm_pselab_predict(const float* logits2d, int ld2, const float* logits3d, int ld3, int64_t N, int C, float* probs_2d,
                      uint8_t* label_2d, float* probs_3d, uint8_t* label_3d, float* probs_ensemble, uint8_t* label_ensemble,
                      hipStream_t s) {
  MM_CHECK_ARG(C > 0 && C <= MM_PRED_MAXC, "pselab_predict: bad C");
  MM_CHECK_ARG(N >= 0 && N <= (int64_t)PT * 0x7fffffff, "pselab_predict: bad N");
  if (N == 0) return MM_OK;
  MM_CHECK_ARG(logits2d && ld2 >= C && probs_2d && label_2d, "pselab_predict: bad 2D arguments");
  const bool has3 = logits3d != nullptr;
  MM_CHECK_ARG(!has3 || (ld3 >= C && probs_3d && label_3d && probs_ensemble && label_ensemble), "pselab_predict: bad 3D arguments");
  const dim3 grid((unsigned)mm_cdiv(N, PT));
  const size_t lds = (size_t)(has3 ? 2 : 1) * PT * (C | 1) * sizeof(float);  // <= 33 KB
  if (has3)
    hipLaunchKernelGGL(k_pselab_predict<true>, grid, dim3(PT), lds, s, logits2d, ld2, logits3d, ld3, N, C, probs_2d, label_2d, probs_3d,
                       label_3d, probs_ensemble, label_ensemble);
  else
    hipLaunchKernelGGL(k_pselab_predict<false>, grid, dim3(PT), lds, s, logits2d, ld2, logits3d, ld3, N, C, probs_2d, label_2d, probs_3d,
                       label_3d, probs_ensemble, label_ensemble);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

// thr_cls == NULL: the scalar thr; else one threshold per output and class (who: the entry point's name in error texts)
static int teacher_labels(const char* who, const float* logits2d, int ld2, const float* logits3d, int ld3, int64_t N, int C,
                          int ensemble, float thr, const float* thr_cls, bool cls, int64_t ignore_label, int64_t* label_2d,
                          int64_t* label_3d, float* prob_2d, float* prob_3d, unsigned long long* kept, hipStream_t s) {
  static_assert(PT % 64 == 0, "k_teacher_labels counts per 64-lane wave");
  MM_CHECK_ARG(C > 0 && C <= MM_PRED_MAXC, "%s: bad C", who);
  MM_CHECK_ARG(N >= 0 && N <= (int64_t)PT * 0x7fffffff, "%s: bad N", who);
  if (N == 0) return MM_OK;
  MM_CHECK_ARG(logits2d && logits3d, "%s: null logits", who);
  MM_CHECK_ARG(label_2d && label_3d, "%s: null labels", who);
  MM_CHECK_ARG(!cls || thr_cls, "%s: null class thresholds", who);
  MM_CHECK_ARG(ld2 >= C && ld3 >= C, "%s: row pitch below C", who);
  if (kept) MM_HIP(hipMemsetAsync(kept, 0, 2 * sizeof(unsigned long long), s));
  const dim3 grid((unsigned)mm_cdiv(N, PT));
  const size_t lds = (size_t)2 * PT * (C | 1) * sizeof(float);  // <= 33 KB
#define MM_TL_LAUNCH(ENS, CLS)                                                                                                   \
  hipLaunchKernelGGL((k_teacher_labels<ENS, CLS>), grid, dim3(PT), lds, s, logits2d, ld2, logits3d, ld3, N, C, thr, thr_cls,     \
                     ignore_label, label_2d, label_3d, prob_2d, prob_3d, kept)
  if (cls) {
    if (ensemble) MM_TL_LAUNCH(true, true);
    else MM_TL_LAUNCH(false, true);
  } else {
    if (ensemble) MM_TL_LAUNCH(true, false);
    else MM_TL_LAUNCH(false, false);
  }
#undef MM_TL_LAUNCH
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_teacher_labels(const float* logits2d, int ld2, const float* logits3d, int ld3, int64_t N, int C, int ensemble, float thr,
                      int64_t ignore_label, int64_t* label_2d, int64_t* label_3d, float* prob_2d, float* prob_3d,
                      unsigned long long* kept, hipStream_t s) {
  return teacher_labels("teacher_labels", logits2d, ld2, logits3d, ld3, N, C, ensemble, thr, nullptr, false, ignore_label, label_2d,
                        label_3d, prob_2d, prob_3d, kept, s);
}

int mm_teacher_labels_cls(const float* logits2d, int ld2, const float* logits3d, int ld3, int64_t N, int C, int ensemble,
                          const float* thr_cls, int64_t ignore_label, int64_t* label_2d, int64_t* label_3d, float* prob_2d,
                          float* prob_3d, unsigned long long* kept, hipStream_t s) {
  return teacher_labels("teacher_labels_cls", logits2d, ld2, logits3d, ld3, N, C, ensemble, 0.f, thr_cls, true, ignore_label, label_2d,
                        label_3d, prob_2d, prob_3d, kept, s);
}

size_t mm_pl_adapt_ws_bytes() { return stats_ws(nullptr, 2 * (1 + MM_PRED_MAXC), 2).bytes; }

int mm_pl_adapt(const float* logits2d, int ld2, const float* logits3d, int ld3, int64_t N, int C, int ensemble, double momentum,
                int warmup, double* state, int64_t* count, float* thr, void* ws, size_t ws_bytes, hipStream_t s) {
  static_assert(2 * (1 + MM_PRED_MAXC) <= PT && 2 * (1 + MM_PRED_MAXC) <= ROWS_FT, "one thread per (output, quantity)");
  MM_CHECK_ARG(C > 0 && C <= MM_PRED_MAXC, "pl_adapt: bad C");
  MM_CHECK_ARG(N >= 0 && N <= (int64_t)PT * 0x7fffffff, "pl_adapt: bad N");
  MM_CHECK_ARG(momentum >= 0.0 && momentum < 1.0, "pl_adapt: the momentum must lie in [0, 1)");
  MM_CHECK_ARG(state && count && thr, "pl_adapt: null state, count or thr");
  MM_CHECK_ARG(N == 0 || (logits2d && logits3d), "pl_adapt: null logits");
  MM_CHECK_ARG(N == 0 || (ld2 >= C && ld3 >= C), "pl_adapt: row pitch below C");
  MM_CHECK_ARG(ws && ws_bytes >= mm_pl_adapt_ws_bytes(), "pl_adapt: workspace missing or too small");
  const StatsWs w = stats_ws(ws, 2 * (1 + MM_PRED_MAXC), 2);
  const int64_t nt = mm_cdiv(N, PT);
  const int nb = (int)(nt > ROWS_MAX_WG ? ROWS_MAX_WG : nt);
  if (nb > 0) {
    const size_t lds = ((size_t)2 * PT * (C | 1) + 2 * PT) * sizeof(float);  // <= 34 KB
    if (ensemble)
      hipLaunchKernelGGL(k_pl_stats<true>, dim3(nb), dim3(PT), lds, s, logits2d, ld2, logits3d, ld3, N, C, w.psum, w.pcnt);
    else
      hipLaunchKernelGGL(k_pl_stats<false>, dim3(nb), dim3(PT), lds, s, logits2d, ld2, logits3d, ld3, N, C, w.psum, w.pcnt);
    MM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_pl_update, dim3(1), dim3(ROWS_FT), 0, s, (const double*)w.psum, (const long long*)w.pcnt, nb, C, momentum,
                     warmup ? 1 : 0, state, count, thr);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

size_t mm_pl_agree_ws_bytes() { return stats_ws(nullptr, 2, 1).bytes; }

int mm_pl_agree(const float* logits2d, int ld2, const float* logits3d, int ld3, int64_t N, int C, float beta, float* w, float* stats,
                int64_t* finite, void* ws, size_t ws_bytes, hipStream_t s) {
  MM_CHECK_ARG(C >= 2 && C <= MM_PRED_MAXC, "pl_agree: C must lie in [2, 32]");
  MM_CHECK_ARG(ld2 >= C && ld3 >= C, "pl_agree: row pitch below C");
  MM_CHECK_ARG(beta > 0.f && beta <= 3.0e38f, "pl_agree: beta must be a finite number > 0");
  MM_CHECK_ARG(N >= 0 && N <= (((int64_t)1 << 31) - 1) / C, "pl_agree: N * C must stay below 2^31");
  MM_CHECK_ARG(N == 0 || (logits2d && logits3d && w), "pl_agree: null logits or w");
  MM_CHECK_ARG(stats, "pl_agree: null stats");
  MM_CHECK_ARG(ws && ws_bytes >= mm_pl_agree_ws_bytes(), "pl_agree: workspace missing or too small");
  const StatsWs p = stats_ws(ws, 2, 1);
  const int64_t nt = mm_cdiv(N, PT);
  const int nb = (int)(nt > ROWS_MAX_WG ? ROWS_MAX_WG : nt);
  if (nb > 0) {
    const size_t lds = (size_t)2 * PT * (C | 1) * sizeof(float);  // <= 33 KB
    hipLaunchKernelGGL(k_pl_agree, dim3(nb), dim3(PT), lds, s, logits2d, ld2, logits3d, ld3, N, C, beta, w, p.psum, p.pcnt);
    MM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_pl_agree_final, dim3(1), dim3(AGREE_FT), 0, s, (const double*)p.psum, (const long long*)p.pcnt, nb, N, stats, finite);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

size_t mm_pselab_refine_ws_bytes(int C) {
  if (C <= 0 || C > MM_PRED_MAXC) return 0;
  return refine_ws(nullptr, C).bytes;
}

int mm_pselab_refine(const float* probs, const int64_t* labels, int64_t N, int C, int64_t ignore_label, int64_t* labels_out, void* ws,
                     size_t ws_bytes, hipStream_t s) {
  MM_CHECK_ARG(C > 0 && C <= MM_PRED_MAXC, "pselab_refine: bad C");
  // a workgroup's LDS counts are 32-bit, and a large N is shared by MAX_BLOCKS workgroups: 2^40 / MAX_BLOCKS = 2^29 points each
  static_assert(((int64_t)1 << 40) / MAX_BLOCKS < ((int64_t)1 << 32), "the bound on N must keep a workgroup's counts below 2^32");
  MM_CHECK_ARG(N >= 0 && N < ((int64_t)1 << 40), "pselab_refine: bad N");
  if (N == 0) return MM_OK;
  MM_CHECK_ARG(probs && labels && labels_out && ws, "pselab_refine: null argument");
  const RefineWs w = refine_ws(ws, C);
  if (ws_bytes < w.bytes) {
    mm_set_error("pselab_refine: workspace too small");
    return MM_ERR_WORKSPACE;
  }
  MM_HIP(hipMemsetAsync(ws, 0, w.bytes, s));
  int64_t nb = mm_cdiv(N, (int64_t)T * 4);
  if (nb > MAX_BLOCKS) nb = MAX_BLOCKS;
  const size_t lds = ((size_t)C * RADIX + C) * sizeof(unsigned);  // <= 32.1 KB
  for (int pass = 0; pass < 4; pass++) {
    hipLaunchKernelGGL(k_refine_hist, dim3((unsigned)nb), dim3(T), lds, s, probs, labels, N, C, pass, w.prefix, w.hist);
    if (pass == 0) MM_LAUNCH_CHECK();  // a bad launch configuration shows at the first launch, before the rest is queued
    hipLaunchKernelGGL(k_refine_select, dim3(1), dim3(RADIX), 0, s, w.hist, C, pass, w.rank, w.prefix, w.thr);
  }
  hipLaunchKernelGGL(k_refine_apply, dim3((unsigned)nb), dim3(T), 0, s, probs, labels, N, C, ignore_label, w.thr, labels_out);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"
