// The row toolkit of the kernels that give a lane one row of per-point logits [N, C] (loss.hip, lovasz.hip, pselab.hip, infomax.hip,
// coral.hip).
// ONE expression each, so that two kernels over the same rows agree bit for bit:
//   label_counted, row_lse, ce_grad_row    which labels count, the row's log-sum-exp, the cross-entropy gradient row
//                                          (loss.hip k_ce_*, k_ce2s_*; lovasz.hip; infomax.hip)
//   row_finite                             a row without a NaN or an infinity (k_im_stats, k_im_bwd, k_pl_agree, k_coral_*)
//   wave_sum, block_sum                    the fixed-order sums of a wave and of a workgroup
//   sum_partials<K>                        one wave over the [nb][K] partials of the pass before (k_ce_finalize, k_ce2s_finalize,
//                                          k_kl_finalize, lovasz.hip)
//   sum_partial                            the same with K known at run time, one quantity per call (k_pl_update, k_im_final,
//                                          k_coral_final)
//   row_tile, tile_head                    the rows of tile t, and where a tile's tail rows begin (k_pselab_predict,
//                                          k_teacher_labels, k_pl_stats, k_pl_agree, k_im_stats, k_im_bwd, k_ce2s_fwd, k_ce2s_bwd,
//                                          k_coral_stats, k_coral_bwd)
//   stage_rows, unstage_rows               global memory -> pitched LDS tile and back, coalesced (every kernel above; out:
//                                          k_im_bwd, k_ce2s_bwd, k_coral_bwd)
//   wave_count, block_count                counted rows: ballots per wave, totals through LDS (k_teacher_labels, k_pl_stats,
//                                          k_im_stats, k_coral_stats)
//   col_sum                                a column of a staged tile into an fp64 accumulator, rows ascending (k_pl_stats, k_im_stats)
//   stats_ws, ROWS_MAX_WG, ROWS_FT         the workspace and the sizes of a capped-grid statistics pass and its one-workgroup
//                                          finish (mm_pl_adapt, mm_pl_agree, mm_im_fwd, mm_coral_fwd)
// (mm_point_predict of pointpred.h keeps its own strict `>` maximum scan: it also tracks the argmax and differs from fmaxf on NaN
// rows.)  Row pointers may be global memory or LDS: the address space is inferred after inlining.
#pragma once
#include "common.h"

// a row is counted when its label is a class and not the ignore value
__device__ __forceinline__ bool label_counted(int64_t y, int64_t ignore, int C) { return !(y == ignore || y < 0 || y >= C); }

// every one of the row's logits is finite (NaN fails the comparison): what counts a row in infomax.hip and in k_pl_agree
constexpr float ROWS_F32_MAX = 3.402823466e38f;
__device__ __forceinline__ bool row_finite(const float* x, int C) {
  bool ok = true;
  for (int c = 0; c < C; c++) ok = ok && fabsf(x[c]) <= ROWS_F32_MAX;
  return ok;
}

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
template <typename V>  // double, or long long for counts
__device__ __forceinline__ V wave_sum(V v) {
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
  for (int k = 0; k < K; k++) v[k] = wave_sum(v[k]);
}

// The same over partial[nb][K] with K known at run time: one wave per quantity q (k_pl_update, k_im_final: a wave per quantity,
// sixteen waves).  Every lane calls; lane 0 holds the total.  V: double for the sums, long long for the integer counts beside them.
template <typename V>
__device__ __forceinline__ V sum_partial(const V* __restrict__ partial, int nb, int K, int q, int lane) {
  V v = 0;
  for (int i = lane; i < nb; i += 64) v += partial[(int64_t)i * K + q];
  return wave_sum(v);
}

// ---- tiles: tile t of the rows [first, N) at PT rows per tile is rows [row0, row0 + rows) of the matrix
struct RowTile { int64_t row0; int rows; };
template <int PT>
__device__ __forceinline__ RowTile row_tile(int64_t t, int64_t N, int64_t first = 0) {
  const int64_t row0 = first + t * PT;
  return {row0, (int)((N - row0) < (int64_t)PT ? (N - row0) : (int64_t)PT)};
}
// the head / tail split of a tile for a first tail row P: its rows [0, h) are head rows, [h, rows) are tail rows P + ...
__device__ __forceinline__ int tile_head(int64_t P, int64_t row0, int rows) {
  return (int)(P <= row0 ? 0 : (P - row0 < (int64_t)rows ? P - row0 : (int64_t)rows));
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

// The mirror: the tile (gradient rows formed in place) leaves LDS for dst[rows, C] (row pitch ld) the same way.  ZERO: a tile
// that holds nothing to keep (head rows alone) writes zeros and reads no LDS.  The caller synchronises before.
template <int NT, bool ZERO = false>
__device__ __forceinline__ void unstage_rows(float* __restrict__ dst, int64_t ld, const float* __restrict__ src, int rows, int C,
                                             int pitch) {
  for (int e = threadIdx.x; e < rows * C; e += NT) {
    const int r = e / C, c = e - r * C;
    dst[(int64_t)r * ld + c] = ZERO ? 0.f : src[r * pitch + c];
  }
}

// ---- counted rows: integers throughout, so the order of the additions cannot show.  wave_count: every lane holds the number of
// its wave's lanes that count; a kernel that walks tiles adds these up per wave.  block_count: the workgroup's totals of K such
// per-wave counters, through words[NT / 64][K] of LDS in wave order; thread k < K returns total k (the others 0).  The caller
// makes sure that nobody still reads what `words` may alias.
__device__ __forceinline__ unsigned wave_count(bool counted) { return (unsigned)__popcll(__ballot(counted)); }

template <int NT, int K>
__device__ __forceinline__ long long block_count(const unsigned (&n)[K], unsigned* words) {
  static_assert(NT % 64 == 0, "counts are kept per 64-lane wave");
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; k++) words[K * wave + k] = n[k];
  }
  __syncthreads();
  long long s = 0;
  if (threadIdx.x < K)
    for (int w = 0; w < NT / 64; w++) s += (long long)words[K * w + threadIdx.x];
  return s;
}

// ---- a column of a staged tile: acc += p[r * stride] for r ascending - the order is part of the result bits.  The accumulator
// is the caller's, carried across the tiles a workgroup walks.
__device__ __forceinline__ void col_sum(double& acc, const float* p, int stride, int rows) {
  for (int r = 0; r < rows; r++) acc += (double)p[r * stride];
}

// ---- a capped-grid statistics pass and its finish: at most ROWS_MAX_WG workgroups walk the tiles and leave K fp64 partial sums
// and n integer counts each; one workgroup of ROWS_FT threads (sixteen waves, a wave per quantity) totals them.
constexpr int ROWS_MAX_WG = 1024;
constexpr int ROWS_FT = 1024;

struct StatsWs { double* psum /*[ROWS_MAX_WG][K]*/; long long* pcnt /*[ROWS_MAX_WG][n]*/; size_t bytes; };
inline StatsWs stats_ws(void* ws, int K, int n) {
  const size_t off = mm_align((size_t)ROWS_MAX_WG * K * sizeof(double));
  return {(double*)ws, (long long*)((char*)ws + off), off + mm_align((size_t)ROWS_MAX_WG * n * sizeof(long long))};
}
