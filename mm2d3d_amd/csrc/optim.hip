// Fused AdamW / Adam / SGD / RMSprop updates over flat fp32 arenas (mm2d3d_amd/optimizers.py FlatAdamW / FlatAdam / FlatSGD /
// FlatRMSprop): the reference's optimiser registry (lib/optimizers.py: adamw, adam, sgd, rmsprop; its trainer runs AdamW,
// train.py:627-636), and the device side of the loss scale (mm2d3d_amd/amp.py).  ONE kernel family, templated on the optimiser and
// its compile-time flags: a variant neither reads nor writes a state array it does not use.  Arithmetic is fp32 in the op order of
// torch's single-tensor paths (torch/optim/{sgd,adam,adamw,rmsprop}.py); g is the gradient times grad_scale.  A thread owns four
// consecutive elements, 16-byte accesses when every array of the range is 16-byte aligned (all arenas of a range share one
// offset), else the scalar instantiation; every element is updated exactly once.
#include "common.h"
#include <math.h>

namespace {
constexpr int T = 256;

enum { SGD = 0, ADAM = 1, RMSPROP = 2 };
// compile-time flags, two bits per optimiser
constexpr int SGD_MOMENTUM = 1, SGD_NESTEROV = 2;
constexpr int ADAM_AMSGRAD = 1, ADAM_DECOUPLED = 2;  // decoupled weight decay = AdamW
constexpr int RMS_MOMENTUM = 1, RMS_CENTERED = 2;

// The coefficients of one parameter group's update: formed on the host and passed as kernel arguments (plain step) or read from
// the device (loss-scaled step, written by k_optim_prepare).  Meaning per optimiser:
//   SGD      lr; wd; k0 = momentum (Nesterov look-ahead); k1 = momentum of the buffer update, k2 = 1 - dampening
//            (k1 = 0, k2 = 1 on the optimiser's first taken step: torch sets buf = g there)
//   Adam     lr = lr / bias_correction1; wd = weight decay (L2) or 1 - lr * wd (decoupled); k0 = 1 - beta1; k1 = beta2;
//            k2 = 1 - beta2; k3 = sqrt(bias_correction2); eps
//   RMSprop  lr; wd; k0 = alpha; k1 = 1 - alpha; k2 = momentum; eps
struct OptCoef {
  float gs, wd, lr, k0, k1, k2, k3, eps;
  int skip, pad;
};
struct OptHyper {  // what the host knows: SGD (lr, a = momentum, b = dampening, wd); Adam (lr, a = beta1, b = beta2, eps, wd);
  double lr, a, b, eps, wd, mu;  // RMSprop (lr, a = alpha, eps, wd, mu = momentum)
};

// t = the step this update is (counts from 1); the same code serves the host (plain step) and k_optim_prepare
__host__ __device__ inline OptCoef make_coef(int kind, int decoupled, const OptHyper& h, long long t, double grad_scale) {
  OptCoef c;
  c.gs = (float)grad_scale, c.wd = (float)h.wd, c.lr = (float)h.lr, c.eps = (float)h.eps;
  c.k0 = c.k1 = c.k2 = c.k3 = 0.f, c.skip = 0, c.pad = 0;
  if (kind == SGD) {
    const bool first = t <= 1;
    c.k0 = (float)h.a, c.k1 = first ? 0.f : (float)h.a, c.k2 = first ? 1.f : (float)(1.0 - h.b);
  } else if (kind == ADAM) {
    const double tt = (double)(t > 0 ? t : 1);
    const double bc1 = 1.0 - pow(h.a, tt), bc2 = 1.0 - pow(h.b, tt);
    c.lr = (float)(h.lr / bc1), c.k0 = (float)(1.0 - h.a), c.k1 = (float)h.b, c.k2 = (float)(1.0 - h.b), c.k3 = (float)sqrt(bc2);
    if (decoupled) c.wd = (float)(1.0 - h.lr * h.wd);
  } else {
    c.k0 = (float)h.a, c.k1 = (float)(1.0 - h.a), c.k2 = (float)h.mu;
  }
  return c;
}

// which of the three state arrays a variant touches: SGD (buf, -, -); Adam (m, v, vmax); RMSprop (sq, gavg, buf)
template <int KIND, int FLAGS>
struct Uses {
  static constexpr bool s0 = KIND == SGD ? (FLAGS & SGD_MOMENTUM) != 0 : true;
  static constexpr bool s1 = KIND == ADAM ? true : (KIND == RMSPROP ? (FLAGS & RMS_CENTERED) != 0 : false);
  static constexpr bool s2 = KIND == ADAM ? (FLAGS & ADAM_AMSGRAD) != 0 : (KIND == RMSPROP ? (FLAGS & RMS_MOMENTUM) != 0 : false);
};

template <int KIND, int FLAGS>
__device__ __forceinline__ void opt_update(const OptCoef& c, float gj, float& p, float& a, float& b, float& d) {
  float g = gj * c.gs;
  if (KIND == SGD) {
    g = g + c.wd * p;
    if (FLAGS & SGD_MOMENTUM) {
      a = c.k1 * a + c.k2 * g;
      g = (FLAGS & SGD_NESTEROV) ? g + c.k0 * a : a;
    }
    p = p - c.lr * g;
  } else if (KIND == ADAM) {
    float pi = p;
    if (FLAGS & ADAM_DECOUPLED)
      pi = p * c.wd;
    else
      g = g + c.wd * p;
    a = a + c.k0 * (g - a);
    b = c.k1 * b + c.k2 * g * g;
    float vv = b;
    if (FLAGS & ADAM_AMSGRAD) vv = d = fmaxf(d, b);
    p = pi - c.lr * (a / (sqrtf(vv) / c.k3 + c.eps));
  } else {
    g = g + c.wd * p;
    a = c.k0 * a + c.k1 * g * g;
    float avg;
    if (FLAGS & RMS_CENTERED) {
      b = b + c.k1 * (g - b);
      avg = sqrtf(a - b * b) + c.eps;
    } else {
      avg = sqrtf(a) + c.eps;
    }
    if (FLAGS & RMS_MOMENTUM) {
      d = c.k2 * d + g / avg;
      p = p - c.lr * d;
    } else {
      p = p - c.lr * (g / avg);
    }
  }
}

template <int KIND, int FLAGS, bool VEC, bool DEV>
__global__ __launch_bounds__(T) void k_optim(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                              float* __restrict__ s1, float* __restrict__ s2, int64_t n, float gs, float wd,
                                              float lr, float k0, float k1, float k2, float k3, float eps,
                                              const OptCoef* __restrict__ dc, const int* __restrict__ skip, int nskip) {
  typedef Uses<KIND, FLAGS> U;
  // The plain step's coefficients arrive as eight scalars, not as an OptCoef by value: with a struct the compiler pairs the
  // multiplies and adds of the scalar path differently (which product joins which fused multiply-add), and AdamW's weights would
  // leave the bits of tests/golden/adamw_bits.npz by an ulp or two on ranges that start unaligned and in ragged tails.  This
  // rests on the compiler's contraction heuristics, not on the language: a new compiler may pair them differently again, and the
  // golden test will say so.  (The DEV instantiations take the eight arguments too and ignore them: one signature for all.)
  OptCoef c = {gs, wd, lr, k0, k1, k2, k3, eps, 0, 0};
  // skip words (the data-parallel reducer's collective flags): decided on the device, uniform
  for (int i = 0; i < nskip; i++)
    if (skip[i]) return;
  if (DEV) {
    c = *dc;
    if (c.skip) return;  // uniform
  }
  const int64_t i = ((int64_t)blockIdx.x * T + threadIdx.x) * 4;
  if (i >= n) return;
  if (VEC && i + 4 <= n) {  // 16-byte accesses (host: every array in use is 16-B aligned); same arithmetic per element
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 G = *(const f4*)(g + i);
    f4 P = *(f4*)(p + i), A = {0.f, 0.f, 0.f, 0.f}, B = A, D = A;
    if (U::s0) A = *(f4*)(s0 + i);
    if (U::s1) B = *(f4*)(s1 + i);
    if (U::s2) D = *(f4*)(s2 + i);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float pj = P[j], aj = A[j], bj = B[j], dj = D[j];
      opt_update<KIND, FLAGS>(c, G[j], pj, aj, bj, dj);
      P[j] = pj, A[j] = aj, B[j] = bj, D[j] = dj;
    }
    *(f4*)(p + i) = P;
    if (U::s0) *(f4*)(s0 + i) = A;
    if (U::s1) *(f4*)(s1 + i) = B;
    if (U::s2) *(f4*)(s2 + i) = D;
    return;
  }
  for (int j = 0; j < 4 && i + j < n; j++) {  // a thread owns elements [i, i+4)
    float aj = 0.f, bj = 0.f, dj = 0.f;
    if (U::s0) aj = s0[i + j];
    if (U::s1) bj = s1[i + j];
    if (U::s2) dj = s2[i + j];
    opt_update<KIND, FLAGS>(c, g[i + j], p[i + j], aj, bj, dj);
    if (U::s0) s0[i + j] = aj;
    if (U::s1) s1[i + j] = bj;
    if (U::s2) s2[i + j] = dj;
  }
}

// one thread: the coefficients of one parameter group from the device state, so that a skipped step (torch.cuda.amp.GradScaler
// semantics) needs no read-back.  ONE decision for every optimiser of the step (the reference's HybridOptim is one optimiser to
// Lightning's GradScaler, train.py:627-636: a non-finite gradient in either network skips both updates) and for the caller's
// extra skip words.  t = *step + 1 is the step this update would be; it is committed to *step only when the step is taken and
// ``advance`` is set (first group of an optimiser).
__global__ void k_optim_prepare(int kind, int decoupled, const float* __restrict__ scale, const int* __restrict__ found, int nfound,
                                long long* __restrict__ step, int advance, OptHyper h, double grad_scale, OptCoef* __restrict__ out) {
  int skip = 0;
  for (int i = 0; i < nfound; i++) skip |= found[i] != 0;
  const long long t = step[0] + (advance ? 1 : 0);
  if (!skip && advance) step[0] = t;
  OptCoef c = make_coef(kind, decoupled, h, t, grad_scale / (double)scale[0]);
  c.skip = skip;
  *out = c;
}

// found[0] |= any element of g is inf / nan (benign race: every writer stores 1)
__global__ __launch_bounds__(T) void k_grad_nonfinite(const float* __restrict__ g, int64_t n, int* __restrict__ found) {
  const int64_t stride = (int64_t)gridDim.x * T * 4;
  bool bad = false;
  for (int64_t i = ((int64_t)blockIdx.x * T + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n && (((uintptr_t)(g + i)) & 15) == 0) {
      typedef float f4 __attribute__((ext_vector_type(4)));
      const f4 G = *(const f4*)(g + i);
#pragma unroll
      for (int j = 0; j < 4; j++) bad |= !(fabsf(G[j]) <= 3.402823466e38f);
    } else {
      for (int j = 0; j < 4 && i + j < n; j++) bad |= !(fabsf(g[i + j]) <= 3.402823466e38f);
    }
  }
  if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) found[0] = 1;
}

// GradScaler.update(): found -> scale *= backoff, tracker = 0; else tracker += 1 and scale *= growth every ``interval`` clean steps
__global__ void k_amp_update(float* __restrict__ scale, int* __restrict__ tracker, const int* __restrict__ found, int nfound,
                             float growth, float backoff, int interval) {
  int any = 0;
  for (int i = 0; i < nfound; i++) any |= found[i];
  if (any) {
    scale[0] *= backoff;
    tracker[0] = 0;
  } else if (++tracker[0] >= interval) {
    scale[0] *= growth;
    tracker[0] = 0;
  }
}

template <int KIND, int FLAGS>
int launch(float* p, const float* g, float* s0, float* s1, float* s2, int64_t n, const OptCoef& c, const OptCoef* dc,
           const int* skip, int nskip, hipStream_t s) {
  typedef Uses<KIND, FLAGS> U;
  if ((U::s0 && !s0) || (U::s1 && !s1) || (U::s2 && !s2) || !p || !g) {
    mm_set_error("optim: a state array this variant uses is NULL");
    return MM_ERR_ARG;
  }
  uintptr_t a = (uintptr_t)p | (uintptr_t)g;  // parameter spans may start anywhere
  if (U::s0) a |= (uintptr_t)s0;
  if (U::s1) a |= (uintptr_t)s1;
  if (U::s2) a |= (uintptr_t)s2;
  const dim3 grid((unsigned)mm_cdiv(n, (int64_t)T * 4));
  const auto kernel = (a & 15) == 0 ? (dc ? k_optim<KIND, FLAGS, true, true> : k_optim<KIND, FLAGS, true, false>)
                                    : (dc ? k_optim<KIND, FLAGS, false, true> : k_optim<KIND, FLAGS, false, false>);
  hipLaunchKernelGGL(kernel, grid, dim3(T), 0, s, p, g, s0, s1, s2, n, c.gs, c.wd, c.lr, c.k0, c.k1, c.k2, c.k3, c.eps, dc, skip, nskip);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

template <int KIND>
int dispatch(int flags, float* p, const float* g, float* s0, float* s1, float* s2, int64_t n, const OptCoef& c, const void* dc,
             const int* skip, int nskip, hipStream_t s) {
  MM_CHECK_ARG(n >= 0, "optim: n < 0");
  MM_CHECK_ARG(nskip >= 0 && nskip <= 16 && (nskip == 0 || skip), "optim: bad skip words");
  if (n == 0) return MM_OK;
  const OptCoef* d = (const OptCoef*)dc;
  switch (flags) {
    case 0: return launch<KIND, 0>(p, g, s0, s1, s2, n, c, d, skip, nskip, s);
    case 1: return launch<KIND, 1>(p, g, s0, s1, s2, n, c, d, skip, nskip, s);
    case 2: return launch<KIND, 2>(p, g, s0, s1, s2, n, c, d, skip, nskip, s);
    default: return launch<KIND, 3>(p, g, s0, s1, s2, n, c, d, skip, nskip, s);
  }
}

int prepare(int kind, int decoupled, const float* scale_dev, const int* found_dev, int nfound, int64_t* step_dev, int advance,
            const OptHyper& h, double grad_scale, void* coef_dev, hipStream_t s) {
  MM_CHECK_ARG(scale_dev && found_dev && step_dev && coef_dev && nfound >= 1 && nfound <= 32, "optim prepare: bad argument");
  hipLaunchKernelGGL(k_optim_prepare, dim3(1), dim3(1), 0, s, kind, decoupled, scale_dev, found_dev, nfound, (long long*)step_dev,
                     advance, h, grad_scale, (OptCoef*)coef_dev);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

inline int sgd_flags(const float* buf, int nesterov) { return (buf ? SGD_MOMENTUM : 0) | (nesterov ? SGD_NESTEROV : 0); }
inline int adam_flags(const float* vmax, int decoupled) { return (vmax ? ADAM_AMSGRAD : 0) | (decoupled ? ADAM_DECOUPLED : 0); }
inline int rms_flags(const float* gavg, const float* buf) { return (buf ? RMS_MOMENTUM : 0) | (gavg ? RMS_CENTERED : 0); }
}  // namespace

extern "C" {

int mm_optim_coef_bytes(void) { return (int)sizeof(OptCoef); }

// ---- plain steps: the host passes the hyper-parameters; ``step`` counts the optimiser's taken steps from 1
int mm_sgd_step(float* p, const float* g, float* buf, int64_t n, double lr, double momentum, double dampening, double weight_decay,
                int nesterov, int64_t step, double grad_scale, const int* skip_dev, int nskip, hipStream_t s) {
  MM_CHECK_ARG(step >= 1, "sgd: step counts from 1");
  MM_CHECK_ARG(!nesterov || buf, "sgd: nesterov needs the momentum buffer");
  const OptHyper h = {lr, momentum, dampening, 0.0, weight_decay, 0.0};
  return dispatch<SGD>(sgd_flags(buf, nesterov), p, g, buf, nullptr, nullptr, n, make_coef(SGD, 0, h, step, grad_scale), nullptr,
                       skip_dev, nskip, s);
}

int mm_adam_step(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, double lr, double beta1, double beta2,
                 double eps, double weight_decay, int decoupled, int64_t step, double grad_scale, const int* skip_dev, int nskip,
                 hipStream_t s) {
  MM_CHECK_ARG(step >= 1, "adam: step counts from 1");
  const OptHyper h = {lr, beta1, beta2, eps, weight_decay, 0.0};
  return dispatch<ADAM>(adam_flags(vmax, decoupled), p, g, m, v, vmax, n, make_coef(ADAM, decoupled, h, step, grad_scale), nullptr,
                        skip_dev, nskip, s);
}

int mm_rmsprop_step(float* p, const float* g, float* sq, float* gavg, float* buf, int64_t n, double lr, double alpha, double eps,
                    double weight_decay, double momentum, double grad_scale, const int* skip_dev, int nskip, hipStream_t s) {
  const OptHyper h = {lr, alpha, 0.0, eps, weight_decay, momentum};
  return dispatch<RMSPROP>(rms_flags(gavg, buf), p, g, sq, gavg, buf, n, make_coef(RMSPROP, 0, h, 1, grad_scale), nullptr, skip_dev,
                           nskip, s);
}

// ---- loss-scaled steps: mm_*_prepare writes one parameter group's coefficients (mm_optim_coef_bytes bytes) from the
// device-resident scale, flag words and step counter; mm_*_step_dev applies them (a no-op when they say "skip")
int mm_sgd_prepare(const float* scale_dev, const int* found_dev, int nfound, int64_t* step_dev, int advance, double lr,
                   double momentum, double dampening, double weight_decay, double grad_scale, void* coef_dev, hipStream_t s) {
  const OptHyper h = {lr, momentum, dampening, 0.0, weight_decay, 0.0};
  return prepare(SGD, 0, scale_dev, found_dev, nfound, step_dev, advance, h, grad_scale, coef_dev, s);
}

int mm_adam_prepare(const float* scale_dev, const int* found_dev, int nfound, int64_t* step_dev, int advance, double lr,
                    double beta1, double beta2, double eps, double weight_decay, int decoupled, double grad_scale, void* coef_dev,
                    hipStream_t s) {
  const OptHyper h = {lr, beta1, beta2, eps, weight_decay, 0.0};
  return prepare(ADAM, decoupled, scale_dev, found_dev, nfound, step_dev, advance, h, grad_scale, coef_dev, s);
}

int mm_rmsprop_prepare(const float* scale_dev, const int* found_dev, int nfound, int64_t* step_dev, int advance, double lr,
                       double alpha, double eps, double weight_decay, double momentum, double grad_scale, void* coef_dev,
                       hipStream_t s) {
  const OptHyper h = {lr, alpha, 0.0, eps, weight_decay, momentum};
  return prepare(RMSPROP, 0, scale_dev, found_dev, nfound, step_dev, advance, h, grad_scale, coef_dev, s);
}

int mm_sgd_step_dev(float* p, const float* g, float* buf, int64_t n, int nesterov, const void* coef_dev, hipStream_t s) {
  MM_CHECK_ARG(coef_dev != nullptr, "sgd_step_dev: no coefficients");
  MM_CHECK_ARG(!nesterov || buf, "sgd: nesterov needs the momentum buffer");
  return dispatch<SGD>(sgd_flags(buf, nesterov), p, g, buf, nullptr, nullptr, n, OptCoef{}, coef_dev, nullptr, 0, s);
}

int mm_adam_step_dev(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, int decoupled, const void* coef_dev,
                     hipStream_t s) {
  MM_CHECK_ARG(coef_dev != nullptr, "adam_step_dev: no coefficients");
  return dispatch<ADAM>(adam_flags(vmax, decoupled), p, g, m, v, vmax, n, OptCoef{}, coef_dev, nullptr, 0, s);
}

int mm_rmsprop_step_dev(float* p, const float* g, float* sq, float* gavg, float* buf, int64_t n, const void* coef_dev,
                        hipStream_t s) {
  MM_CHECK_ARG(coef_dev != nullptr, "rmsprop_step_dev: no coefficients");
  return dispatch<RMSPROP>(rms_flags(gavg, buf), p, g, sq, gavg, buf, n, OptCoef{}, coef_dev, nullptr, 0, s);
}

// ---- the loss scale (torch.cuda.amp.GradScaler semantics without a read-back; mm2d3d_amd/amp.py)
int mm_grad_nonfinite(const float* g, int64_t n, int* found_dev, hipStream_t s) {
  if (n == 0) return MM_OK;
  int64_t nb = mm_cdiv(n, (int64_t)T * 4);
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(k_grad_nonfinite, dim3((unsigned)nb), dim3(T), 0, s, g, n, found_dev);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_amp_update(float* scale_dev, int* tracker_dev, const int* found_dev, int nfound, double growth, double backoff, int interval,
                  hipStream_t s) {
  MM_CHECK_ARG(scale_dev && tracker_dev && found_dev && nfound >= 0 && interval >= 1, "amp_update: bad arguments");
  hipLaunchKernelGGL(k_amp_update, dim3(1), dim3(1), 0, s, scale_dev, tracker_dev, found_dev, nfound, (float)growth, (float)backoff, interval);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- mean-teacher weights
// e <- lerp(e, p, 1 - decay) over a device table of tensor pairs (mm2d3d_amd/ema.py WeightEMA: the optimisers' arenas and the
// modules' floating-point buffers), ONE launch for every pair, gated by the decision the optimiser update of the same step was
// gated by: the caller's skip words and OptCoef::skip of a device-counted step.  These kernels live in this file only because they
// read OptCoef::skip.  Within a row the contract is k_optim's: a thread owns four consecutive elements, 16-byte accesses when both
// pointers of the row are 16-byte aligned and the four elements fit, else element by element.
namespace {
struct EmaRow {
  float* dst;      // the teacher's tensor
  float* src;      // the live tensor
  long long n;     // elements (0 is legal: the row owns no workgroup)
  long long first; // number of the row's first workgroup: the sum of cdiv(n, 4 T) over the rows before it
};

// The row of this workgroup: the last one whose first workgroup is <= blockIdx.x (rows without elements share their successor's
// number and are never the last).  Returns the thread's first element in the row, or -1 when it owns none.
__device__ __forceinline__ long long ema_locate(const EmaRow* __restrict__ table, int nrows, EmaRow& r) {
  const long long b = blockIdx.x;
  int lo = 0, hi = nrows;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (table[mid].first <= b)
      lo = mid;
    else
      hi = mid;
  }
  r = table[lo];
  const long long local = b - r.first;
  if (local < 0) return -1;
  const long long i = (local * T + threadIdx.x) * 4;
  return i < r.n ? i : -1;
}

__device__ __forceinline__ bool ema_vec(const EmaRow& r, long long i) {
  return ((((uintptr_t)r.dst | (uintptr_t)r.src) & 15) == 0) && i + 4 <= r.n;
}

// torch's lerp(e, p, w) in fp32: exact at both ends (p == e leaves e as it is; w = 1 gives p)
__device__ __forceinline__ float ema_lerp(float e, float p, float w) {
  const float d = p - e;
  return w < 0.5f ? e + w * d : p - d * (1.f - w);
}

__global__ __launch_bounds__(T) void k_ema_update(const EmaRow* __restrict__ table, int nrows, double decay, int warmup,
                                                   long long t_host, const long long* __restrict__ step,
                                                   const OptCoef* __restrict__ dc, const int* __restrict__ skip, int nskip) {
  for (int i = 0; i < nskip; i++)  // uniform, decided on the device
    if (skip[i]) return;
  if (dc && dc->skip) return;
  double dt = decay;
  if (warmup) {
    const double t = (double)(step ? step[0] : t_host);  // taken steps, this one included
    dt = fmin(decay, (1.0 + t) / (10.0 + t));
  }
  const float w = (float)(1.0 - dt);
  EmaRow r;
  const long long i = ema_locate(table, nrows, r);
  if (i < 0) return;
  if (ema_vec(r, i)) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 P = *(const f4*)(r.src + i);
    f4 E = *(f4*)(r.dst + i);
#pragma unroll
    for (int j = 0; j < 4; j++) E[j] = ema_lerp(E[j], P[j], w);
    *(f4*)(r.dst + i) = E;
    return;
  }
  for (int j = 0; j < 4 && i + j < r.n; j++) r.dst[i + j] = ema_lerp(r.dst[i + j], r.src[i + j], w);
}

__global__ __launch_bounds__(T) void k_ema_swap(const EmaRow* __restrict__ table, int nrows) {
  EmaRow r;
  const long long i = ema_locate(table, nrows, r);
  if (i < 0) return;
  if (ema_vec(r, i)) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 P = *(f4*)(r.src + i), E = *(f4*)(r.dst + i);
    *(f4*)(r.src + i) = E;
    *(f4*)(r.dst + i) = P;
    return;
  }
  for (int j = 0; j < 4 && i + j < r.n; j++) {
    const float pj = r.src[i + j];
    r.src[i + j] = r.dst[i + j];
    r.dst[i + j] = pj;
  }
}

int ema_check_table(const void* table_dev, int nrows, int64_t nblocks) {
  MM_CHECK_ARG(nrows >= 0 && nblocks >= 0 && nblocks <= 0x7fffffffLL, "ema: bad table size");
  MM_CHECK_ARG(nblocks == 0 || (nrows >= 1 && table_dev), "ema: workgroups without a table");
  return MM_OK;
}
}  // namespace

extern "C" {

int mm_ema_row_bytes(void) { return (int)sizeof(EmaRow); }

int mm_ema_update(const void* table_dev, int nrows, int64_t nblocks, double decay, int warmup, int64_t t_host, const int64_t* step_dev,
                  const void* coef_dev, const int* skip_dev, int nskip, hipStream_t s) {
  if (int rc = ema_check_table(table_dev, nrows, nblocks)) return rc;
  MM_CHECK_ARG(decay >= 0.0 && decay < 1.0, "ema_update: decay outside [0, 1)");
  MM_CHECK_ARG(t_host >= 0, "ema_update: t < 0");
  MM_CHECK_ARG(nskip >= 0 && nskip <= 16 && (nskip == 0 || skip_dev), "ema_update: bad skip words");
  if (nblocks == 0) return MM_OK;
  hipLaunchKernelGGL(k_ema_update, dim3((unsigned)nblocks), dim3(T), 0, s, (const EmaRow*)table_dev, nrows, decay, warmup ? 1 : 0,
                     (long long)t_host, (const long long*)step_dev, (const OptCoef*)coef_dev, skip_dev, nskip);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_ema_swap(const void* table_dev, int nrows, int64_t nblocks, hipStream_t s) {
  if (int rc = ema_check_table(table_dev, nrows, nblocks)) return rc;
  if (nblocks == 0) return MM_OK;
  hipLaunchKernelGGL(k_ema_swap, dim3((unsigned)nblocks), dim3(T), 0, s, (const EmaRow*)table_dev, nrows);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"
