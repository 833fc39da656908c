// The per-point prediction shared by evaluation (loss.hip k_eval_confusion) and pseudo-label export (pselab.hip
// k_pselab_predict): argmax of the 2D logits, of the 3D logits and of the softmax average (EXP/train.py:297-339).  ONE expression
// for both kernels, so the labels a model exports are the labels its evaluation counted.
#pragma once
#include <hip/hip_runtime.h>

constexpr int MM_PRED_MAXC = 32;  // class-count limit of the row-wise kernels (loss.hip MAXC)

struct MMPointPred {
  int ia, ib, ie;     // argmax of row a, of row b, of 0.5 * (softmax(a) + softmax(b)); the FIRST maximum wins (strict >)
  float pa, pb, pe;   // the maxima themselves: softmax(a)[ia], softmax(b)[ib], the ensemble's
};

// a, b: one row of C logits each (global memory or LDS: the address space is inferred after inlining).  HAS_B = false: a 2D-only
// prediction, only ia / pa are meaningful.
template <bool HAS_B>
__device__ __forceinline__ MMPointPred mm_point_predict(const float* a, const float* b, int C) {
  MMPointPred r;
  if (!HAS_B) {
    float ma = a[0];
    int ia = 0;
    for (int c = 1; c < C; c++)
      if (a[c] > ma) { ma = a[c]; ia = c; }
    float sa = 0.f;
    for (int c = 0; c < C; c++) sa += expf(a[c] - ma);
    r.ia = ia, r.ib = 0, r.ie = 0;
    r.pa = 1.f / sa;  // expf(a[ia] - ma) = expf(0) = 1 exactly
    r.pb = 0.f, r.pe = 0.f;
    return r;
  }
  float ma = a[0], mb = b[0];
  int ia = 0, ib = 0;
  for (int c = 1; c < C; c++) {
    if (a[c] > ma) { ma = a[c]; ia = c; }
    if (b[c] > mb) { mb = b[c]; ib = c; }
  }
  float sa = 0.f, sb = 0.f;
  for (int c = 0; c < C; c++) {
    sa += expf(a[c] - ma);
    sb += expf(b[c] - mb);
  }
  float best = -1.f;
  int ie = 0;
  for (int c = 0; c < C; c++) {
    float e = 0.5f * (expf(a[c] - ma) / sa + expf(b[c] - mb) / sb);
    if (e > best) { best = e; ie = c; }
  }
  r.ia = ia, r.ib = ib, r.ie = ie;
  r.pa = 1.f / sa, r.pb = 1.f / sb, r.pe = best;
  return r;
}
