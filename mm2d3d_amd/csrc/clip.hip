// Gradient clipping for the flat optimisers (mm2d3d_amd/clip.py): torch.nn.utils.clip_grad_norm_ / clip_grad_value_ on the
// TRUE gradient g * grad_scale / scale of arenas that hold loss-scaled, un-averaged gradients - without a read-back.
//   k_grad_sqnorm     sum of squares of one fp32 arena, one double partial per workgroup (no atomics: the caller's workspace)
//   k_clip_finalize   one workgroup: the partials of every arena of the step in a fixed order -> total norm, torch's clip
//                     coefficient c = min(1, max_norm / (norm + 1e-6)) and the EFFECTIVE SCALE scale / c.  The update kernels
//                     (optim.hip k_optim) then apply grad_scale * c / scale through their prepare kernels,
//                     unchanged: the clip costs one read of the gradients and no write.
//   k_grad_clip_value clamp of an arena to +-clip_value * scale / grad_scale in place (NaN passes, as torch.clamp)
// Sums are carried in double: an arena holds gradients times a loss scale of 2^16 .. 2^24 and more, whose squares leave fp32's
// range long before the gradient does; (double)x * (double)x is exact and never overflows, so a finite arena gives a finite sum
// and a non-finite sum says that an element was inf / nan (the kernel raises the caller's flag word from it).
#include "common.h"
#include <float.h>
#include <math.h>

namespace {
constexpr int T = 256;
constexpr int UNROLL = 4;                           // 16-byte loads in flight per thread
constexpr int64_t CHUNK4 = (int64_t)T * UNROLL;     // float4s of the smallest chunk: 16 KiB of gradients per workgroup
constexpr int64_t MAX_PARTS = 4096;                 // partials per arena (mm_grad_nonfinite's grid cap)
typedef float f4 __attribute__((ext_vector_type(4)));

// Chunk ownership is a function of n alone (not of the device): workgroup b owns the float4s [b * chunk4(n), (b + 1) * chunk4(n))
// of the 16-byte aligned body; parts(n) workgroups always run, those past the body's end write a zero partial.
inline int64_t chunk4(int64_t n) {
  const int64_t k = mm_cdiv(n / 4, CHUNK4 * MAX_PARTS);
  return CHUNK4 * (k > 1 ? k : 1);
}
inline int64_t parts(int64_t n) {
  const int64_t p = mm_cdiv(n / 4, chunk4(n));
  return p > 1 ? p : 1;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;  // lane 0
}

// lane-0-of-wave-0 result: waves in index order (a fixed order: bit-stable from run to run)
__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < T / 64; w++) t += sh[w];
  return t;
}

// g[0, head) scalar (up to the first 16-byte boundary), body = nb4 float4s from g + head, tail = the rest (< 4): every
// element is read exactly once; head and tail belong to workgroup 0
__global__ __launch_bounds__(T) void k_grad_sqnorm(const float* __restrict__ g, int64_t n, int64_t head, int64_t nb4, int64_t ch4,
                                                    double* __restrict__ part, int* __restrict__ found) {
  __shared__ double sh[T / 64];
  const f4* __restrict__ b = (const f4*)(g + head);
  const int64_t lo = (int64_t)blockIdx.x * ch4;
  const int64_t hi = lo + ch4 < nb4 ? lo + ch4 : nb4;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += CHUNK4) {
    f4 v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      const int64_t j = i + (int64_t)u * T;
      v[u] = j < hi ? b[j] : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      const double x0 = (double)v[u][0], x1 = (double)v[u][1], x2 = (double)v[u][2], x3 = (double)v[u][3];
      a0 = fma(x0, x0, a0), a1 = fma(x1, x1, a1), a2 = fma(x2, x2, a2), a3 = fma(x3, x3, a3);
    }
  }
  double t = block_sum((a0 + a1) + (a2 + a3), sh);
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0) {
      for (int64_t i = 0; i < head; i++) t = fma((double)g[i], (double)g[i], t);
      for (int64_t i = head + 4 * nb4; i < n; i++) t = fma((double)g[i], (double)g[i], t);
    }
    part[blockIdx.x] = t;
    if (found && !(fabs(t) <= DBL_MAX)) found[0] = 1;  // benign race: every writer stores 1
  }
}

__global__ __launch_bounds__(T) void k_clip_finalize(const double* __restrict__ part, int64_t total, const float* __restrict__ scale,
                                                      double grad_scale, float max_norm, float* __restrict__ norm_out,
                                                      float* __restrict__ eff_scale_out) {
  __shared__ double sh[T / 64];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < total; i += T) a += part[i];  // thread t: partials t, t + 256, ... in index order
  const double sum = block_sum(a, sh);
  if (threadIdx.x == 0) {
    const float s = scale[0];
    const float norm = (float)(sqrt(sum) * grad_scale / (double)s);  // of the true gradient: one rounding, to fp32
    const float q = max_norm / (norm + 1e-6f);                        // torch.nn.utils.clip_grad_norm_, in fp32 as there
    const float c = q > 1.f ? 1.f : q;                                // clamp(max = 1): a NaN stays a NaN
    norm_out[0] = norm;
    eff_scale_out[0] = s / c;  // c = 1 leaves the scale's bits alone
  }
}

template <bool VEC>
__global__ __launch_bounds__(T) void k_grad_clip_value(float* __restrict__ g, int64_t n, float clip_value, const float* __restrict__ scale,
                                                        double grad_scale) {
  const int64_t i = ((int64_t)blockIdx.x * T + threadIdx.x) * 4;
  if (i >= n) return;
  const float hi = (float)((double)clip_value * (double)scale[0] / grad_scale), lo = -hi;
  if (VEC && i + 4 <= n) {
    const f4 G = *(const f4*)(g + i);
    f4 R = G;
    bool changed = false;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      R[j] = G[j] < lo ? lo : (G[j] > hi ? hi : G[j]);  // both comparisons are false for a NaN
      changed |= G[j] < lo || G[j] > hi;
    }
    if (changed) *(f4*)(g + i) = R;
    return;
  }
  for (int j = 0; j < 4 && i + j < n; j++) {  // a thread owns elements [i, i + 4)
    const float x = g[i + j];
    if (x < lo) g[i + j] = lo;
    else if (x > hi) g[i + j] = hi;
  }
}
}  // namespace

extern "C" {

size_t mm_grad_sqnorm_ws_bytes(int64_t n) { return n < 0 ? 0 : (size_t)parts(n) * sizeof(double); }

int mm_grad_sqnorm(const float* g, int64_t n, void* partial_ws, int64_t slot, int* found_dev, hipStream_t s) {
  MM_CHECK_ARG(n >= 0 && (g || n == 0) && partial_ws && slot >= 0, "grad_sqnorm: bad argument");
  MM_CHECK_ARG(((uintptr_t)g & 3) == 0 && ((uintptr_t)partial_ws & 7) == 0, "grad_sqnorm: misaligned pointer");
  int64_t head = (int64_t)(((16 - ((uintptr_t)g & 15)) & 15) / 4);
  if (head > n) head = n;
  const int64_t nb4 = (n - head) / 4;  // <= n / 4: parts(n) workgroups cover it
  hipLaunchKernelGGL(k_grad_sqnorm, dim3((unsigned)parts(n)), dim3(T), 0, s, g, n, head, nb4, chunk4(n), (double*)partial_ws + slot,
                     found_dev);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_clip_finalize(const void* partial_ws, const int64_t* counts, int narenas, const float* scale_dev, double grad_scale,
                     double max_norm, float* norm_out_dev, float* eff_scale_out_dev, hipStream_t s) {
  MM_CHECK_ARG(partial_ws && counts && narenas >= 1 && scale_dev && norm_out_dev && eff_scale_out_dev, "clip_finalize: bad argument");
  MM_CHECK_ARG(max_norm >= 0.0 && grad_scale > 0.0, "clip_finalize: max_norm >= 0 and grad_scale > 0");
  int64_t total = 0;
  for (int i = 0; i < narenas; i++) {
    MM_CHECK_ARG(counts[i] >= 0, "clip_finalize: negative count");
    total += counts[i];
  }
  hipLaunchKernelGGL(k_clip_finalize, dim3(1), dim3(T), 0, s, (const double*)partial_ws, total, scale_dev, grad_scale, (float)max_norm,
                     norm_out_dev, eff_scale_out_dev);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_grad_clip_value(float* g, int64_t n, double clip_value, const float* scale_dev, double grad_scale, hipStream_t s) {
  MM_CHECK_ARG(n >= 0 && (g || n == 0) && scale_dev, "grad_clip_value: bad argument");
  MM_CHECK_ARG(clip_value >= 0.0 && grad_scale > 0.0, "grad_clip_value: clip_value >= 0 and grad_scale > 0");
  if (n == 0) return MM_OK;
  const dim3 grid((unsigned)mm_cdiv(n, (int64_t)T * 4));
  if (((uintptr_t)g & 15) == 0)
    hipLaunchKernelGGL(k_grad_clip_value<true>, grid, dim3(T), 0, s, g, n, (float)clip_value, scale_dev, grad_scale);
  else
    hipLaunchKernelGGL(k_grad_clip_value<false>, grid, dim3(T), 0, s, g, n, (float)clip_value, scale_dev, grad_scale);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"
