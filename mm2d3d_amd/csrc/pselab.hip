// Pseudo labels for the self-training round (EXP/train.py:297-339 -> the files lib/dataset/*_dataloader.py read back):
//   mm_pselab_predict   per point: max and argmax of softmax(2D logits), of softmax(3D logits) and of their average
//   mm_teacher_labels   the same per-point expression, written as the int64 training labels of both heads (a mean teacher that
//                       labels the target batch inside the step), with an optional confidence threshold and kept counts
//   mm_pselab_refine    lib/utils/refine_pseudo_labels.py, exact: per class the lower median of the confidences by a
//                       most-significant-digit radix select (four 8-bit passes over the order-preserving uint32 image of the
//                       floats), threshold min(median, 0.9f), labels below it become ignore_label
// Counts are integers and are summed with integer atomics: the result does not depend on the order of the additions.
#include "common.h"
#include "pointpred.h"
#include "rows.h"

namespace {
constexpr int PT = 128;      // points per workgroup of the prediction kernel
constexpr int T = 256;
constexpr int RADIX = 256;   // 8 bits per pass
constexpr int MAX_BLOCKS = 2048;

// ---- prediction.  The [rows, C] blocks of both logit matrices go through LDS (stage_rows of rows.h: coalesced copies, then each
// lane reads its own row, pitched to an odd number of words).
template <bool HAS3>
__global__ __launch_bounds__(PT) void k_pselab_predict(const float* __restrict__ l2, int ld2, const float* __restrict__ l3, int ld3,
                                                        int64_t N, int C, float* __restrict__ p2, uint8_t* __restrict__ y2,
                                                        float* __restrict__ p3, uint8_t* __restrict__ y3, float* __restrict__ pe,
                                                        uint8_t* __restrict__ ye) {
  extern __shared__ float tile[];  // [HAS3 ? 2 : 1][PT][pitch]
  const int pitch = C | 1;
  const int64_t row0 = (int64_t)blockIdx.x * PT;
  const int rows = (int)((N - row0) < (int64_t)PT ? (N - row0) : (int64_t)PT);
  float* ta = tile;
  float* tb = tile + PT * pitch;
  stage_rows<PT>(ta, l2 + row0 * ld2, ld2, rows, C, pitch);
  if (HAS3) stage_rows<PT>(tb, l3 + row0 * ld3, ld3, rows, C, pitch);
  __syncthreads();
  if ((int)threadIdx.x >= rows) return;
  const MMPointPred r = mm_point_predict<HAS3>(ta + threadIdx.x * pitch, tb + threadIdx.x * pitch, C);
  const int64_t i = row0 + threadIdx.x;
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
template <bool ENS>
__global__ __launch_bounds__(PT) void k_teacher_labels(const float* __restrict__ l2, int ld2, const float* __restrict__ l3, int ld3,
                                                        int64_t N, int C, float thr, int64_t ignore, int64_t* __restrict__ y2,
                                                        int64_t* __restrict__ y3, float* __restrict__ p2, float* __restrict__ p3,
                                                        unsigned long long* __restrict__ kept) {
  extern __shared__ float tile[];  // [2][PT][pitch]
  const int pitch = C | 1;
  const int64_t row0 = (int64_t)blockIdx.x * PT;
  const int rows = (int)((N - row0) < (int64_t)PT ? (N - row0) : (int64_t)PT);
  float* ta = tile;
  float* tb = tile + PT * pitch;
  stage_rows<PT>(ta, l2 + row0 * ld2, ld2, rows, C, pitch);
  stage_rows<PT>(tb, l3 + row0 * ld3, ld3, rows, C, pitch);
  __syncthreads();
  bool k2 = false, k3 = false;
  if ((int)threadIdx.x < rows) {
    const MMPointPred r = mm_point_predict<true>(ta + threadIdx.x * pitch, tb + threadIdx.x * pitch, C);
    const float pa = ENS ? r.pe : r.pa, pb = ENS ? r.pe : r.pb;
    const int ia = ENS ? r.ie : r.ia, ib = ENS ? r.ie : r.ib;
    k2 = thr < 0.f || pa >= thr;
    k3 = thr < 0.f || pb >= thr;
    const int64_t i = row0 + threadIdx.x;
    y2[i] = k2 ? (int64_t)ia : ignore;
    y3[i] = k3 ? (int64_t)ib : ignore;
    if (p2) p2[i] = pa;
    if (p3) p3[i] = pb;
  }
  if (!kept) return;  // uniform
  const unsigned n2 = (unsigned)__popcll(__ballot(k2)), n3 = (unsigned)__popcll(__ballot(k3));
  __syncthreads();  // every lane has read its rows
  unsigned* cnt = (unsigned*)tile;  // [PT / 64][2]
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) cnt[2 * wave] = n2, cnt[2 * wave + 1] = n3;
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned n = 0;
    for (int w = 0; w < PT / 64; w++) n += cnt[2 * w + threadIdx.x];
    if (n) atomicAdd(&kept[threadIdx.x], (unsigned long long)n);
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

int mm_teacher_labels(const float* logits2d, int ld2, const float* logits3d, int ld3, int64_t N, int C, int ensemble, float thr,
                      int64_t ignore_label, int64_t* label_2d, int64_t* label_3d, float* prob_2d, float* prob_3d,
                      unsigned long long* kept, hipStream_t s) {
  static_assert(PT % 64 == 0, "k_teacher_labels counts per 64-lane wave");
  MM_CHECK_ARG(C > 0 && C <= MM_PRED_MAXC, "teacher_labels: bad C");
  MM_CHECK_ARG(N >= 0 && N <= (int64_t)PT * 0x7fffffff, "teacher_labels: bad N");
  if (N == 0) return MM_OK;
  MM_CHECK_ARG(logits2d && logits3d, "teacher_labels: null logits");
  MM_CHECK_ARG(label_2d && label_3d, "teacher_labels: null labels");
  MM_CHECK_ARG(ld2 >= C && ld3 >= C, "teacher_labels: row pitch below C");
  if (kept) MM_HIP(hipMemsetAsync(kept, 0, 2 * sizeof(unsigned long long), s));
  const dim3 grid((unsigned)mm_cdiv(N, PT));
  const size_t lds = (size_t)2 * PT * (C | 1) * sizeof(float);  // <= 33 KB
  if (ensemble)
    hipLaunchKernelGGL(k_teacher_labels<true>, grid, dim3(PT), lds, s, logits2d, ld2, logits3d, ld3, N, C, thr, ignore_label, label_2d,
                       label_3d, prob_2d, prob_3d, kept);
  else
    hipLaunchKernelGGL(k_teacher_labels<false>, grid, dim3(PT), lds, s, logits2d, ld2, logits3d, ld3, N, C, thr, ignore_label, label_2d,
                       label_3d, prob_2d, prob_3d, kept);
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
