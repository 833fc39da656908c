// Lovasz-softmax loss over per-point logits [N, C] (Berman et al., CVPR 2018): for every class the errors e_i = |fg_i - p_ic| of
// the counted rows are ordered descending (stable in the row index) and weighted by the increments of the Jaccard loss along
// that order.  The increments are evaluated in closed form from integers (include/mm2d3d.h), never as a difference of two
// Jaccard values.
//
// Passes (every cross-workgroup dependency is a launch of its own: no look-back, no spin, no grid barrier; integer atomics only):
//   k_lv_keys                one thread per row: softmax, err [C][N], sort keys, foreground counts per class
//   3 x (k_lv_hist, k_lv_block_sums, k_lv_scan_sums, k_lv_rescan, k_lv_scatter)
//                            stable least-significant-digit radix sort of (key, row), every class in one grid (blockIdx.y)
//   k_lv_fg_tiles, k_lv_scan_sums
//                            foreground rows per tile of the sorted order, exclusive scan over the tiles
//   k_lv_eval                closed forms, coef scattered back to row order, sum e * g per (class, tile) in fp64
//   k_lv_finalize            fp64 partials summed in a fixed order: bit-stable run to run
//
// Digit plan: e <= 1.0, so key = 0x3F800000 - bits(e) lies in [0, 0x3F800000] and ascending keys are descending errors; an
// uncounted row gets 0x3F800001 and sorts behind e == 0.  30 significant bits = three 10-bit digits.
#include "common.h"
#include "pointpred.h"
#include "rows.h"

namespace {
constexpr int T = 256;
constexpr int WAVES = T / 64;
constexpr int ITEMS = 4;
constexpr int TILE = T * ITEMS;  // keys per workgroup of the histogram, scatter and evaluation kernels
constexpr int BITS = 10;
constexpr int RADIX = 1 << BITS;
constexpr int PASSES = 3;
constexpr int SCAN_PER = 8;
constexpr int SCAN_BLK = T * SCAN_PER;  // counters per workgroup of the offset scan
constexpr int MAXC = MM_PRED_MAXC;
constexpr int64_t MAXN = (int64_t)1 << 24;
constexpr unsigned KEY_ONE = 0x3F800000u;  // bits of 1.0f
constexpr unsigned KEY_UNCOUNTED = KEY_ONE + 1u;
constexpr unsigned FG_BIT = 0x80000000u;

static_assert(MAXC <= 32, "the row kernels take at most 32 classes");
static_assert(BITS * PASSES >= 30 && RADIX % T == 0, "three digits cover the 30 key bits");

__device__ inline int wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    int t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

// block-wide exclusive scan of one int per thread; the total in *tot
__device__ inline int block_excl_scan(int v, int* tot, int* wsum /*[WAVES] LDS*/) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = wave_incl_scan(v);
  __syncthreads();
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int i = 0; i < WAVES; i++) {
    int x = wsum[i];
    if (i < w) base += x;
    total += x;
  }
  *tot = total;
  return base + inc - v;
}

// counts[0 .. C) = foreground rows per class, counts[C] = counted rows (zeroed by the caller)
__global__ __launch_bounds__(T) void k_lv_keys(const float* __restrict__ logits, int ld, int64_t N, int C,
                                                const int64_t* __restrict__ labels, int64_t ignore, float* __restrict__ err,
                                                unsigned* __restrict__ keys, unsigned* __restrict__ vals, int* __restrict__ counts) {
  __shared__ int cnt[MAXC + 1];
  if (threadIdx.x <= C) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
  if (i < N) {
    const int64_t y = labels[i];
    if (!label_counted(y, ignore, C)) {
      for (int c = 0; c < C; c++) {
        err[c * N + i] = -1.f;
        keys[c * N + i] = KEY_UNCOUNTED;
        vals[c * N + i] = (unsigned)i;
      }
    } else {
      const float* x = logits + i * ld;
      const RowLse l = row_lse(x, C);
      const float m = l.m, inv = 1.f / l.s;
      for (int c = 0; c < C; c++) {
        const float p = expf(x[c] - m) * inv;
        const bool fg = c == (int)y;
        const float e = fabsf((fg ? 1.f : 0.f) - p);
        err[c * N + i] = e;
        unsigned u = __float_as_uint(e);
        if (u > KEY_ONE) u = KEY_ONE;  // non-finite logits: the key stays inside its 30 bits
        keys[c * N + i] = KEY_ONE - u;
        vals[c * N + i] = (unsigned)i | (fg ? FG_BIT : 0u);
      }
      atomicAdd(&cnt[(int)y], 1);
      atomicAdd(&cnt[C], 1);
    }
  }
  __syncthreads();
  if (threadIdx.x <= C && cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], cnt[threadIdx.x]);
}

// cnt[c][d * ntiles + t] = keys of tile t of class c whose digit is d: digit-major, so the exclusive scan of the row is the
// destination of the first such key
__global__ __launch_bounds__(T) void k_lv_hist(const unsigned* __restrict__ keys, int64_t N, int ntiles, int shift,
                                                int* __restrict__ cnt) {
  __shared__ int h[RADIX];
  for (int d = threadIdx.x; d < RADIX; d += T) h[d] = 0;
  __syncthreads();
  const int c = blockIdx.y, t = blockIdx.x;
  const unsigned* k = keys + (int64_t)c * N;
  const int64_t base = (int64_t)t * TILE;
#pragma unroll
  for (int r = 0; r < ITEMS; r++) {
    const int64_t pos = base + r * T + threadIdx.x;
    if (pos < N) atomicAdd(&h[(k[pos] >> shift) & (RADIX - 1)], 1);
  }
  __syncthreads();
  int* o = cnt + (int64_t)c * RADIX * ntiles;
  for (int d = threadIdx.x; d < RADIX; d += T) o[(int64_t)d * ntiles + t] = h[d];
}

// ---- exclusive scan of m int32 per class (blockIdx.y) in three launches: sums per block, one workgroup over the sums, rescan
__global__ __launch_bounds__(T) void k_lv_block_sums(const int* __restrict__ in, int64_t m, int nb, int* __restrict__ sums) {
  __shared__ int wsum[WAVES];
  const int* a = in + (int64_t)blockIdx.y * m;
  const int64_t base = (int64_t)blockIdx.x * SCAN_BLK + threadIdx.x * SCAN_PER;
  int v = 0;
#pragma unroll
  for (int i = 0; i < SCAN_PER; i++)
    if (base + i < m) v += a[base + i];
  int tot;
  block_excl_scan(v, &tot, wsum);
  if (threadIdx.x == 0) sums[(int64_t)blockIdx.y * nb + blockIdx.x] = tot;
}

// in place; more than T sums: the workgroup walks them T at a time and carries the total
__global__ __launch_bounds__(T) void k_lv_scan_sums(int* __restrict__ sums, int nb) {
  __shared__ int wsum[WAVES];
  int* a = sums + (int64_t)blockIdx.y * nb;
  int carry = 0;
  for (int b0 = 0; b0 < nb; b0 += T) {
    const int i = b0 + threadIdx.x;
    const int v = i < nb ? a[i] : 0;
    int tot;
    const int ex = block_excl_scan(v, &tot, wsum);
    if (i < nb) a[i] = carry + ex;
    carry += tot;
  }
}

// in place: every thread holds its SCAN_PER counters before it writes them
__global__ __launch_bounds__(T) void k_lv_rescan(int* __restrict__ io, int64_t m, int nb, const int* __restrict__ sums) {
  __shared__ int wsum[WAVES];
  int* a = io + (int64_t)blockIdx.y * m;
  const int64_t base = (int64_t)blockIdx.x * SCAN_BLK + threadIdx.x * SCAN_PER;
  int x[SCAN_PER];
  int v = 0;
#pragma unroll
  for (int i = 0; i < SCAN_PER; i++) {
    x[i] = base + i < m ? a[base + i] : 0;
    v += x[i];
  }
  int tot;
  int ex = block_excl_scan(v, &tot, wsum) + sums[(int64_t)blockIdx.y * nb + blockIdx.x];
#pragma unroll
  for (int i = 0; i < SCAN_PER; i++) {
    if (base + i < m) a[base + i] = ex;
    ex += x[i];
  }
}

// Stable scatter of one tile.  Wave w owns the tile's keys [w * 256, w * 256 + 256) and walks them 64 at a time; lanes that hold
// the same digit find each other with one ballot per digit bit, the lowest of them takes the wave's running count of the digit
// and hands it to the others by a shuffle.  Destination = scanned offset of (digit, tile) + the earlier waves' keys of the digit
// + the rank inside the wave: source order is kept among equal digits.
__global__ __launch_bounds__(T) void k_lv_scatter(const unsigned* __restrict__ keys_in, const unsigned* __restrict__ vals_in,
                                                   unsigned* __restrict__ keys_out, unsigned* __restrict__ vals_out, int64_t N,
                                                   int ntiles, int shift, const int* __restrict__ off) {
  __shared__ int wcnt[WAVES][RADIX];
  for (int d = threadIdx.x; d < WAVES * RADIX; d += T) (&wcnt[0][0])[d] = 0;
  __syncthreads();
  const int c = blockIdx.y, t = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t cbase = (int64_t)c * N;
  const int64_t base = (int64_t)t * TILE + w * (64 * ITEMS);
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned k[ITEMS], v[ITEMS];
  int dig[ITEMS], rank[ITEMS];
  bool valid[ITEMS];
#pragma unroll
  for (int r = 0; r < ITEMS; r++) {
    const int64_t pos = base + r * 64 + lane;
    valid[r] = pos < N;
    k[r] = valid[r] ? keys_in[cbase + pos] : 0u;
    v[r] = valid[r] ? vals_in[cbase + pos] : 0u;
    dig[r] = (int)((k[r] >> shift) & (RADIX - 1));
    unsigned long long peers = __ballot(valid[r]);
#pragma unroll
    for (int b = 0; b < BITS; b++) {
      const bool bit = (dig[r] >> b) & 1;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const int leader = valid[r] ? __ffsll((long long)peers) - 1 : lane;
    int old = 0;
    if (valid[r] && leader == lane) {
      old = wcnt[w][dig[r]];
      wcnt[w][dig[r]] = old + __popcll(peers);
    }
    old = __shfl(old, leader, 64);
    rank[r] = old + __popcll(peers & below);
  }
  __syncthreads();
  const int* o = off + (int64_t)c * RADIX * ntiles;
  for (int d = threadIdx.x; d < RADIX; d += T) {
    int b = o[(int64_t)d * ntiles + t];
#pragma unroll
    for (int i = 0; i < WAVES; i++) {
      const int n = wcnt[i][d];
      wcnt[i][d] = b;
      b += n;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < ITEMS; r++) {
    const int64_t dst = (int64_t)wcnt[w][dig[r]] + rank[r];
    if (valid[r] && dst >= 0 && dst < N) {
      keys_out[cbase + dst] = k[r];
      vals_out[cbase + dst] = v[r];
    }
  }
}

// fgt[c][t] = foreground rows among the sorted positions of tile t
__global__ __launch_bounds__(T) void k_lv_fg_tiles(const unsigned* __restrict__ vals, int64_t N, int ntiles, int* __restrict__ fgt) {
  __shared__ int wsum[WAVES];
  const unsigned* v = vals + (int64_t)blockIdx.y * N;
  const int64_t base = (int64_t)blockIdx.x * TILE;
  int n = 0;
#pragma unroll
  for (int r = 0; r < ITEMS; r++) {
    const int64_t pos = base + r * T + threadIdx.x;
    if (pos < N) n += (int)(v[pos] >> 31);
  }
  int tot;
  block_excl_scan(n, &tot, wsum);
  if (threadIdx.x == 0) fgt[(int64_t)blockIdx.y * ntiles + blockIdx.x] = tot;
}

__device__ inline int included_classes(const int* __restrict__ counts, int C, int classes_all) {
  if (classes_all) return counts[C] > 0 ? C : 0;
  int n = 0;
  for (int c = 0; c < C; c++) n += counts[c] > 0 ? 1 : 0;
  return n;
}

// sorted position j (rank r = j + 1) of class c: f = foreground rows among ranks 1 .. r, U = G + r - f, I = G - f
__global__ __launch_bounds__(T) void k_lv_eval(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals, int64_t N, int C,
                                                int ntiles, int classes_all, const int* __restrict__ counts,
                                                const int* __restrict__ fgt, float* __restrict__ coef, double* __restrict__ partial) {
  __shared__ int wsum[WAVES];
  __shared__ double red[T];
  const int c = blockIdx.y, t = blockIdx.x;
  const int64_t cbase = (int64_t)c * N;
  const int G = counts[c], ncount = counts[C];
  const bool included = classes_all ? ncount > 0 : G > 0;
  const float nf = (float)included_classes(counts, C, classes_all);
  int f = fgt[(int64_t)c * ntiles + t];
  double sum = 0.0;
  for (int r = 0; r < ITEMS; r++) {
    const int64_t pos = (int64_t)t * TILE + r * T + threadIdx.x;
    const bool valid = pos < N;
    const unsigned v = valid ? vals[cbase + pos] : 0u;
    const int fg = (int)(v >> 31);
    int tot;
    const int fi = f + block_excl_scan(fg, &tot, wsum) + fg;
    f += tot;
    if (!valid) continue;
    float g = 0.f;
    if (included && pos < ncount) {
      const int rank = (int)pos + 1;
      const int U = G + rank - fi, I = G - fi;
      if (G == 0)
        g = rank == 1 ? 1.f : 0.f;
      else if (fg)
        g = 1.f / (float)U;
      else
        g = (float)I / ((float)U * (float)(U - 1));
      const float e = __uint_as_float(KEY_ONE - keys[cbase + pos]);
      sum += (double)e * (double)g;
    }
    const float q = g / nf;  // g == 0 wherever nf == 0
    const int64_t row = v & 0x00FFFFFFu;
    if (row < N) coef[cbase + row] = g == 0.f ? 0.f : (fg ? -q : q);
  }
  const double s = block_sum<T>(sum, red);
  if (threadIdx.x == 0) partial[(int64_t)c * ntiles + t] = s;
}

// one workgroup: wave w sums the tiles of classes w, w + 4, ... (lanes stride the partials, then a fixed shuffle tree), thread 0 adds
// the classes in order
__global__ __launch_bounds__(T) void k_lv_finalize(const double* __restrict__ partial, int C, int ntiles, int classes_all,
                                                    const int* __restrict__ counts, float* __restrict__ stats) {
  __shared__ double lc[MAXC];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int c = w; c < C; c += WAVES) {
    double a[1];
    sum_partials<1>(partial + (int64_t)c * ntiles, ntiles, lane, a);
    if (lane == 0) lc[c] = a[0];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n = included_classes(counts, C, classes_all);
    double a = 0.0;
    for (int c = 0; c < C; c++)
      if (classes_all || counts[c] > 0) a += lc[c];
    stats[0] = n ? (float)(a / (double)n) : 0.f;
    stats[1] = (float)n;
    stats[2] = (float)counts[C];
  }
}

// dlogits_ik = grad_out * p_ik * (coef[k][i] - sum_c coef[c][i] * p_ic); a row whose coefficients are all zero gets zeros
__global__ __launch_bounds__(T) void k_lv_bwd(const float* __restrict__ logits, int ld, int64_t N, int C, const float* __restrict__ coef,
                                               const float* __restrict__ gout, float* __restrict__ dlogits, int ld_d) {
  const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
  if (i >= N) return;
  const float* x = logits + i * ld;
  float* d = dlogits + i * ld_d;
  bool any = false;
  for (int c = 0; c < C; c++) any = any || coef[c * N + i] != 0.f;
  if (!any) {
    for (int c = 0; c < C; c++) d[c] = 0.f;
    return;
  }
  const RowLse l = row_lse(x, C);
  const float m = l.m, inv = 1.f / l.s;
  float dot = 0.f;
  for (int c = 0; c < C; c++) dot += coef[c * N + i] * (expf(x[c] - m) * inv);
  const float g = gout[0];
  for (int c = 0; c < C; c++) d[c] = g * (expf(x[c] - m) * inv) * (coef[c * N + i] - dot);
}

struct LvWs {
  unsigned *keys[2], *vals[2];
  int *cnt, *sums, *fgt, *counts;
  double* partial;
  size_t bytes;
  int ntiles, nb;
};

// ws == nullptr: only the size
LvWs lv_ws(void* ws, int64_t N, int C) {
  LvWs w;
  w.ntiles = (int)mm_cdiv(N > 0 ? N : 1, TILE);
  w.nb = (int)mm_cdiv((int64_t)RADIX * w.ntiles, SCAN_BLK);
  const size_t kv = mm_align((size_t)C * (size_t)(N > 0 ? N : 1) * sizeof(unsigned));
  const size_t cnt = mm_align((size_t)C * RADIX * w.ntiles * sizeof(int));
  const size_t sums = mm_align((size_t)C * w.nb * sizeof(int));
  const size_t fgt = mm_align((size_t)C * w.ntiles * sizeof(int));
  const size_t counts = mm_align((size_t)(MAXC + 1) * sizeof(int));
  const size_t partial = mm_align((size_t)C * w.ntiles * sizeof(double));
  char* p = (char*)ws;
  size_t o = 0;
  for (int i = 0; i < 2; i++) {
    w.keys[i] = (unsigned*)(p + o), o += kv;
    w.vals[i] = (unsigned*)(p + o), o += kv;
  }
  w.cnt = (int*)(p + o), o += cnt;
  w.sums = (int*)(p + o), o += sums;
  w.fgt = (int*)(p + o), o += fgt;
  w.counts = (int*)(p + o), o += counts;
  w.partial = (double*)(p + o), o += partial;
  w.bytes = o + 256;
  return w;
}

static_assert(MAXN * MAXC < ((int64_t)1 << 31), "N * C stays below 2^31: the [C][N] arrays are indexed by int32 offsets of the scan");
bool lv_size_ok(int64_t N, int C) { return C >= 1 && C <= MAXC && N >= 0 && N <= MAXN; }
}  // namespace

extern "C" {

size_t mm_lovasz_ws_bytes(int64_t N, int C) { return lv_size_ok(N, C) ? lv_ws(nullptr, N, C).bytes : 0; }

int mm_lovasz_fwd(const float* logits, int ld, int64_t N, int C, const int64_t* labels, int64_t ignore_index, int classes_all,
                  float* err, float* coef, float* stats, void* ws, size_t ws_bytes, hipStream_t s) {
  MM_CHECK_ARG(C >= 1 && C <= MAXC && ld >= C, "lovasz: bad C (1 <= C <= %d, ld >= C)", MAXC);
  MM_CHECK_ARG(N >= 0 && N <= MAXN, "lovasz: N outside [0, 2^24]");
  MM_CHECK_ARG(stats && ws, "lovasz: null stats or workspace");
  MM_CHECK_ARG(N == 0 || (logits && labels && err && coef), "lovasz: null logits, labels, err or coef");
  const LvWs w = lv_ws(ws, N, C);
  if (ws_bytes < w.bytes) {
    mm_set_error("lovasz: workspace too small: %zu < %zu", ws_bytes, w.bytes);
    return MM_ERR_WORKSPACE;
  }
  MM_HIP(hipMemsetAsync(w.counts, 0, (size_t)(MAXC + 1) * sizeof(int), s));
  if (N == 0) {
    hipLaunchKernelGGL(k_lv_finalize, dim3(1), dim3(T), 0, s, w.partial, C, 0, classes_all ? 1 : 0, w.counts, stats);
    MM_LAUNCH_CHECK();
    return MM_OK;
  }
  const dim3 tiles((unsigned)w.ntiles, (unsigned)C), blocks((unsigned)w.nb, (unsigned)C), one(1, (unsigned)C);
  const int64_t m = (int64_t)RADIX * w.ntiles;
  hipLaunchKernelGGL(k_lv_keys, dim3((unsigned)mm_cdiv(N, T)), dim3(T), 0, s, logits, ld, N, C, labels, ignore_index, err, w.keys[0],
                     w.vals[0], w.counts);
  MM_LAUNCH_CHECK();  // a bad launch configuration shows at the first launch, before the rest is queued
  int cur = 0;
  for (int pass = 0; pass < PASSES; pass++, cur ^= 1) {
    const int shift = BITS * pass;
    hipLaunchKernelGGL(k_lv_hist, tiles, dim3(T), 0, s, w.keys[cur], N, w.ntiles, shift, w.cnt);
    hipLaunchKernelGGL(k_lv_block_sums, blocks, dim3(T), 0, s, w.cnt, m, w.nb, w.sums);
    hipLaunchKernelGGL(k_lv_scan_sums, one, dim3(T), 0, s, w.sums, w.nb);
    hipLaunchKernelGGL(k_lv_rescan, blocks, dim3(T), 0, s, w.cnt, m, w.nb, w.sums);
    hipLaunchKernelGGL(k_lv_scatter, tiles, dim3(T), 0, s, w.keys[cur], w.vals[cur], w.keys[cur ^ 1], w.vals[cur ^ 1], N, w.ntiles,
                       shift, w.cnt);
  }
  hipLaunchKernelGGL(k_lv_fg_tiles, tiles, dim3(T), 0, s, w.vals[cur], N, w.ntiles, w.fgt);
  hipLaunchKernelGGL(k_lv_scan_sums, one, dim3(T), 0, s, w.fgt, w.ntiles);
  hipLaunchKernelGGL(k_lv_eval, tiles, dim3(T), 0, s, w.keys[cur], w.vals[cur], N, C, w.ntiles, classes_all ? 1 : 0, w.counts, w.fgt,
                     coef, w.partial);
  hipLaunchKernelGGL(k_lv_finalize, dim3(1), dim3(T), 0, s, w.partial, C, w.ntiles, classes_all ? 1 : 0, w.counts, stats);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_lovasz_bwd(const float* logits, int ld, int64_t N, int C, const float* coef, const float* grad_out, float* dlogits, int ld_d,
                  hipStream_t s) {
  MM_CHECK_ARG(C >= 1 && C <= MAXC && ld >= C, "lovasz: bad C (1 <= C <= %d, ld >= C)", MAXC);
  MM_CHECK_ARG(ld_d >= C, "lovasz: gradient row pitch below C");
  MM_CHECK_ARG(N >= 0 && N <= MAXN, "lovasz: N outside [0, 2^24]");
  if (N == 0) return MM_OK;
  MM_CHECK_ARG(logits && coef && grad_out && dlogits, "lovasz: null logits, coef, grad_out or dlogits");
  hipLaunchKernelGGL(k_lv_bwd, dim3((unsigned)mm_cdiv(N, T)), dim3(T), 0, s, logits, ld, N, C, coef, grad_out, dlogits, ld_d);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"
