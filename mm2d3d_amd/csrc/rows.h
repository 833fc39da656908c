// The row toolkit of the kernels that give a lane one row of per-point logits [N, C] (loss.hip, lovasz.hip, pselab.hip): which
// labels count, the row's log-sum-exp, the cross-entropy gradient row, the fixed-order sums and the pitched LDS staging.  ONE
// expression each, so that two losses over the same row agree bit for bit.  (mm_point_predict of pointpred.h keeps its own strict
// `>` maximum scan: it also tracks the argmax and differs from fmaxf on NaN rows.)
// Row pointers may be global memory or LDS: the address space is inferred after inlining.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// a row is counted when its label is a class and not the ignore value
__device__ __forceinline__ bool label_counted(int64_t y, int64_t ignore, int C) { return !(y == ignore || y < 0 || y >= C); }

struct RowLse {
  float m, s;  // the row's maximum, sum_c expf(x[c] - m): logsumexp = m + logf(s), softmax_c = expf(x[c] - m) / s
};

// fmaxf from x[0] on, then the sum ascending in c: the order is part of the result bits
__device__ __forceinline__ RowLse row_lse(const float* x, int C) {
  RowLse r;
  r.m = x[0];
  for (int c = 1; c < C; c++) r.m = fmaxf(r.m, x[c]);
  r.s = 0.f;
  for (int c = 0; c < C; c++) r.s += expf(x[c] - r.m);
  return r;
}

// d[c] = k * (softmax(x)_c - onehot(y)_c), inv = 1 / s of row_lse.  d may BE x (k_ce2s_bwd forms the row in place): no
// __restrict__, and every element is read before it is written.
__device__ __forceinline__ void ce_grad_row(float* d, const float* x, int C, float m, float inv, float k, int y) {
  for (int c = 0; c < C; c++) d[c] = k * (expf(x[c] - m) * inv - (c == y ? 1.f : 0.f));
}

// ---- sums in a fixed order: bit-stable run to run
__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// the LDS tree over a workgroup of NT threads; red: NT doubles, free again after the next __syncthreads
template <int NT>
__device__ __forceinline__ double block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// One wave over partial[nb][K] (K interleaved fp64 sums per workgroup of the pass before): the lanes stride the workgroups
// (independent loads), then the shuffle tree; lane 0 holds the K totals.  (One thread walking <= 1024 partials through dependent
// loads took 18-26 us per call.)
template <int K>
__device__ __forceinline__ void sum_partials(const double* __restrict__ partial, int nb, int lane, double (&v)[K]) {
#pragma unroll
  for (int k = 0; k < K; k++) v[k] = 0.0;
  for (int i = lane; i < nb; i += 64) {
#pragma unroll
    for (int k = 0; k < K; k++) v[k] += partial[K * i + k];
  }
#pragma unroll
  for (int k = 0; k < K; k++) v[k] = wave_sum64(v[k]);
}

// ---- staging: a [rows, C] block (row pitch ld) copied into LDS by a workgroup of NT threads, consecutive lanes on consecutive
// addresses of a row (a lane reading its own row from global memory strides by ld floats).  Each lane then reads its row from
// LDS; pitch = C | 1 words, odd, so that the 64 lanes fall on distinct banks.  The caller synchronises.
template <int NT>
__device__ __forceinline__ void stage_rows(float* __restrict__ dst, const float* __restrict__ src, int64_t ld, int rows, int C,
                                           int pitch) {
  for (int e = threadIdx.x; e < rows * C; e += NT) {
    const int r = e / C, c = e - r * C;
    dst[r * pitch + c] = src[(int64_t)r * ld + c];
  }
}
