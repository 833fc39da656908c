// Sparse-to-dense cross-modal matching (the window search of DsCML, Peng et al., ICCV 2021): every point looks for the pixel of the
// (2r + 1)^2 window round its own whose dense logits match its row best; include/mm2d3d.h has the definition.
//   mm_xm_search  k_xm_search<DIR>: the candidates of a point lie on the lanes of a lane group of LP = 16 (r <= 1), 32 (r = 2) or
//                 64 (r = 3) lanes, so a wave serves 4, 2 or 1 points and a workgroup of 256 threads a tile of 16, 8 or 4.  Lane 0 of
//                 a group holds the centre, the others the rest of the window row-major: the lanes of one window row read
//                 neighbouring pixels, C consecutive floats each in the NHWC layout - the requests of a group fall on (2r + 1) short
//                 runs of the map, which neighbouring points share through L2.  (A lane per POINT that walks the window serially
//                 makes 49 dependent strided row reads per lane at r = 3 and leaves 15 of 64 lanes' worth of a wave waiting on
//                 each: the design this layout replaces.)  A lane copies its pixel's row into a pitch-(C | 1) LDS row (any map
//                 strides; NCHW maps are read with stride sc), the group copies the point row once.  Lane 0 takes the point row's
//                 log-sum-exp (row_lse of rows.h), the group's lanes then share the C per-class terms of the point row - its
//                 log-softmax and, for DIR 0, its softmax: one expf per class and point, not per candidate.  Every lane forms its
//                 candidate's KL with the expressions of k_kl_fwd (loss.hip); the argmin is a butterfly over (counted, value,
//                 candidate order) with __shfl_xor inside the group, the same total order on every lane.  Lane 0 writes sel / klmin
//                 and counts the rows that left the centre.  A capped grid walks the tiles; the four integer counters leave as
//                 per-workgroup partials.
//                 k_xm_counts: one workgroup, a wave per counter, totals the partials in a fixed order (sum_partial of rows.h).
// One kernel body serves every r (LP is a run-time argument): the centre's value of an r = 0 call and of an r = 3 call are the same
// instructions, the same bits.  No atomics, no host read, no workgroup waits for another: bit-stable run to run.
#include "common.h"
#include "pointpred.h"
#include "rows.h"

namespace {
constexpr int T = 256;
constexpr int MAXC = MM_PRED_MAXC;
constexpr int RMAX = 3;
constexpr int PR = 3 * MAXC;  // floats of LDS per lane group: the point row, its per-class terms u and v

struct Cand {
  bool ok;  // inside the image and not NaN
  float v;
  int ord;
};
// the better of two candidates: a counted one before a skipped one, then the smaller value, then the earlier in the order
__device__ __forceinline__ Cand better(const Cand a, const Cand b) {
  if (a.ok != b.ok) return a.ok ? a : b;
  if (a.ok && a.v != b.v) return a.v < b.v ? a : b;
  return a.ord < b.ord ? a : b;
}
// candidate `ord` of the window: 0 is the centre, then the others row-major (dy ascending, then dx)
__device__ __forceinline__ void cand_offset(int ord, int r, int& dy, int& dx) {
  const int side = 2 * r + 1, centre = r * side + r;
  int t = ord == 0 ? centre : (ord - 1 < centre ? ord - 1 : ord);
  dy = t / side - r, dx = t - (t / side) * side - r;
}

// DIR 0: KL(softmax(row_i) || softmax(map_j)) - the point row teaches the pixel.  DIR 1: KL(softmax(map_j) || softmax(row_i)).
template <int DIR>
__global__ __launch_bounds__(T) void k_xm_search(const float* __restrict__ seg, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int B, int H,
                                                  int W, int C, const int32_t* __restrict__ key, const float* __restrict__ rows, int ld,
                                                  int64_t N, int64_t P, int r, int LP, int64_t ntiles, int32_t* __restrict__ sel,
                                                  float* __restrict__ klmin, long long* __restrict__ pcnt /*[grid][4]*/) {
  extern __shared__ float lds[];  // [T][pitch] pixel rows, then [T / LP][PR] point rows and their terms
  __shared__ unsigned long long words[T / 64][4];
  const int pitch = C | 1, PT = T / LP, ncand = (2 * r + 1) * (2 * r + 1);
  const int tid = threadIdx.x, g = tid / LP, sub = tid - g * LP;
  float* px = lds + tid * pitch;
  float* pr = lds + T * pitch + g * PR;
  float *u = pr + MAXC, *v = pr + 2 * MAXC;
  const int64_t npix = (int64_t)B * H * W;
  unsigned long long cnt[4] = {0, 0, 0, 0};  // moved rows of [0, P), of [P, N); their displacements
  int dy, dx;
  cand_offset(sub < ncand ? sub : 0, r, dy, dx);
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t i = t * PT + g;
    const bool active = i < N;
    const int32_t k = active ? key[i] : 0;
    const bool inmap = active && k >= 0 && (int64_t)k < npix;  // a key outside the map reads nothing and stays where it is
    const int b = k / (H * W), rem = k - b * (H * W), y = rem / W, x = rem - y * W;
    const bool in = inmap && sub < ncand && y + dy >= 0 && y + dy < H && x + dx >= 0 && x + dx < W;
    if (in) {
      const float* p = seg + (int64_t)b * sb + (int64_t)(y + dy) * sy + (int64_t)(x + dx) * sx;
      for (int c = 0; c < C; c++) px[c] = p[(int64_t)c * sc];
    }
    if (active)
      for (int c = sub; c < C; c += LP) pr[c] = rows[i * ld + c];
    __syncthreads();
    RowLse rl = {0.f, 1.f};
    if (sub == 0 && active) rl = row_lse(pr, C);
    const float m = __shfl(rl.m, 0, LP), s = __shfl(rl.s, 0, LP);
    const float lrow = m + logf(s);
    if (active)
      for (int c = sub; c < C; c += LP) {
        const float lq = pr[c] - lrow;  // the point row's log-softmax
        u[c] = lq;
        if (DIR == 0) v[c] = expf(lq);
      }
    __syncthreads();
    Cand best = {false, 0.f, sub};
    if (in) {
      const RowLse rj = row_lse(px, C);
      const float lj = rj.m + logf(rj.s);
      float a = 0.f;
      if (DIR == 0) {
        for (int c = 0; c < C; c++) a += v[c] * (u[c] - (px[c] - lj));
      } else {
        for (int c = 0; c < C; c++) {
          const float lq = px[c] - lj;
          a += expf(lq) * (lq - u[c]);
        }
      }
      best.v = a;
      best.ok = a == a;
    }
    const Cand own = best;
    for (int d = LP >> 1; d > 0; d >>= 1) {
      Cand o;
      o.ok = __shfl_xor((int)best.ok, d, 64) != 0;
      o.v = __shfl_xor(best.v, d, 64);
      o.ord = __shfl_xor(best.ord, d, 64);
      best = better(best, o);
    }
    if (sub == 0 && active) {
      // nothing counted: the centre, with the centre's own value (NaN, or 0 bits of a key outside the map)
      if (!best.ok) best = own;
      if (!inmap) best.v = __int_as_float(0x7fc00000);
      int by, bx;
      cand_offset(best.ord, r, by, bx);
      sel[i] = k + by * W + bx;
      klmin[i] = best.v;
      if (best.ord != 0) {
        const int seg_i = i >= P ? 1 : 0, ay = by < 0 ? -by : by, ax = bx < 0 ? -bx : bx;
        cnt[seg_i] += 1;
        cnt[2 + seg_i] += (unsigned long long)(ay > ax ? ay : ax);
      }
    }
  }
  // the workgroup's four totals: integers, so the order of the additions cannot show
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const long long w = wave_sum((long long)cnt[q]);
    if ((tid & 63) == 0) words[tid >> 6][q] = (unsigned long long)w;
  }
  __syncthreads();
  if (tid < 4) {
    long long a = 0;
    for (int w = 0; w < T / 64; w++) a += (long long)words[w][tid];
    pcnt[(int64_t)blockIdx.x * 4 + tid] = a;
  }
}

__global__ __launch_bounds__(T) void k_xm_counts(const long long* __restrict__ pcnt, int nb, int64_t* __restrict__ counts) {
  const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long a = sum_partial<long long>(pcnt, nb, 4, q, lane);
  if (lane == 0) counts[q] = (int64_t)a;
}

size_t search_lds(int C, int LP) { return ((size_t)T * (C | 1) + (size_t)(T / LP) * PR) * sizeof(float); }
}  // namespace

extern "C" {

size_t mm_xm_search_ws_bytes(void) { return mm_align((size_t)ROWS_MAX_WG * 4 * sizeof(long long)); }

int mm_xm_search(const float* seg, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int B, int H, int W, int C, const int32_t* key,
                 const float* rows, int ld, int64_t N, int64_t P, int r, int direction, int32_t* sel, float* klmin, int64_t* counts,
                 void* ws, size_t ws_bytes, hipStream_t s) {
  MM_CHECK_ARG(r >= 0 && r <= RMAX, "xm_search: window radius %d outside [0, %d]", r, RMAX);
  MM_CHECK_ARG(C >= 2 && C <= MAXC, "xm_search: %d classes, the window search takes 2 to %d", C, MAXC);
  MM_CHECK_ARG(direction == 0 || direction == 1, "xm_search: direction %d is neither 0 (row teaches map) nor 1 (map teaches row)", direction);
  MM_CHECK_ARG(N >= 0 && N < (1ll << 31) && N * C < (1ll << 31), "xm_search: too many elements (N=%lld C=%d)", (long long)N, C);
  MM_CHECK_ARG(P >= 0 && P <= N, "xm_search: row split %lld outside [0, %lld]", (long long)P, (long long)N);
  MM_CHECK_ARG(B > 0 && H > 0 && W > 0 && (int64_t)B * H * W < (1ll << 31), "xm_search: bad map shape (B=%d H=%d W=%d)", B, H, W);
  MM_CHECK_ARG(ld >= C, "xm_search: row pitch %d below C = %d", ld, C);
  MM_CHECK_ARG(counts && ws, "xm_search: null counts or workspace");
  MM_CHECK_ARG(N == 0 || (seg && key && rows && sel && klmin), "xm_search: null seg, key, rows, sel or klmin");
  if (ws_bytes < mm_xm_search_ws_bytes()) {
    mm_set_error("xm_search: workspace too small (%zu < %zu)", ws_bytes, mm_xm_search_ws_bytes());
    return MM_ERR_WORKSPACE;
  }
  const int ncand = (2 * r + 1) * (2 * r + 1), LP = ncand <= 16 ? 16 : (ncand <= 32 ? 32 : 64);
  const int64_t ntiles = mm_cdiv(N, T / LP);
  const int nb = (int)(ntiles < ROWS_MAX_WG ? ntiles : ROWS_MAX_WG);
  if (nb > 0) {
    auto kern = direction == 0 ? k_xm_search<0> : k_xm_search<1>;
    hipLaunchKernelGGL(kern, dim3(nb), dim3(T), search_lds(C, LP), s, seg, sb, sy, sx, sc, B, H, W, C, key, rows, ld, N, P, r, LP, ntiles,
                       sel, klmin, (long long*)ws);
  }
  hipLaunchKernelGGL(k_xm_counts, dim3(1), dim3(T), 0, s, (const long long*)ws, nb, counts);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"
