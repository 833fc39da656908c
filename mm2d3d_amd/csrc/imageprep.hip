// GPU-side camera-image preparation (datasets.gpu_batch(..., image="gpu")): crop, PIL BILINEAR resize, the four colour-jitter
// operations, float conversion + normalisation, fliplr and the NCHW fp32 store of a whole batch, bit-exact with the host path
// (PIL + numpy, mm2d3d_amd/datasets.py _resize / color_jitter.ColorJitter / _float_image / _normalise).
//   resize   Image.resize(size, BILINEAR)            nuscenes_dataloader.py:257-262, semantic_kitti.py:321-392, a2d2.py:268-276
//   jitter   ColorJitter(...)(PIL image)             nuscenes_dataloader.py:286-287
// The host decodes (PIL), draws, and builds the tables (mm2d3d_amd/imageprep.py): per scene a descriptor (window of the
// decoded image, Q22 coefficients of both axes, jitter operations in drawn order, hue shift, flip), fp32 factors and a
// [3][256] LUT that holds the float conversion + normalisation of every byte value.
//
// Three launches over the batch (blockIdx.y = scene, one thread per pixel):
//   k_img_hpass   horizontal pass, uint8 -> uint8 temp, only the source rows the vertical pass reads (Resample.c)
//   k_img_vpass   vertical pass + the jitter operations before Contrast + per-scene int64 sums of L (Contrast's mean)
//   k_img_finish  Contrast, the remaining operations, LUT, fliplr, store
// Every intermediate is uint8, as in PIL, where every operation returns an 8-bit image.  An axis the resize leaves unchanged
// runs with one tap of weight 1 << 22, which reproduces its input exactly.
//
// Arithmetic (Pillow 12 libImaging): Resample.c accumulates in int32 from 1 << 21 and clips acc >> 22; Blend.c computes
// (float)a + alpha * (float)(b - a) in fp32, multiply then add, never fused; Convert.c's rgb2hsv / hsv2rgb mix fp32 and
// fp64 step by step.  Hence no contraction in this file: the pragma below governs the operators written here, but not the
// bodies of the __fmul_rn / __fadd_rn style helpers, which the HIP runtime wrapper defines before this file's first line (once
// inlined, their product and sum fused into one FMA: Contrast and Color then differed from Pillow on about 2 % of the pixels).
#pragma clang fp contract(off)
#include "common.h"

namespace {
constexpr int T = 256;
constexpr int QBITS = 22;  // Resample.c PRECISION_BITS
// descriptor words (include/mm2d3d.h MM_IMG_*; mm2d3d_amd/imageprep.py D_*)
enum { D_SRC_OFF, D_SRC_PITCH, D_WIN_W, D_WIN_H, D_TMP_ROWS, D_YBOX_FIRST, D_KX, D_KY, D_HCOEF, D_VCOEF, D_TMP_OFF, D_OPS, D_NOPS, D_NPRE,
       D_HUE, D_FLIP, D_N };
enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_COLOR = 2, OP_HUE = 3 };

__device__ inline int clip_q(int acc) {
  acc >>= QBITS;
  return acc < 0 ? 0 : acc > 255 ? 255 : acc;
}
__device__ inline int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// ImagingConvert RGB -> L (Convert.c L24)
__device__ inline int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// ImagingBlend (Blend.c)
__device__ inline int blend(int a, int b, float f) {
  const float t = (float)a + f * (float)(b - a);
  if (f >= 0.f && f <= 1.f) return (int)t;
  return t <= 0.f ? 0 : t >= 255.f ? 255 : (int)t;
}

// Convert.c rgb2hsv_row / hsv2rgb, the hue shift of color_jitter.ColorJitter in between
__device__ inline void hue_shift(int& r, int& g, int& b, int shift) {
  const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
  if (mx == mn) return;  // H = S = 0: hsv2rgb gives (v, v, v) = the input
  const float cr = (float)(mx - mn);
  const float s = cr / (float)mx;
  const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
  float h;
  if (r == mx)
    h = bc - gc;
  else if (g == mx)
    h = (float)(2.0 + (double)rc - (double)bc);
  else
    h = (float)(4.0 + (double)gc - (double)rc);
  h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
  const int hh = (clip8((int)((double)h * 255.0)) + shift) & 255;
  const int ss = clip8((int)((double)s * 255.0));
  const int v = mx;
  if (ss == 0) {
    r = g = b = v;
    return;
  }
  const double h6 = (double)hh * 6.0 / 255.0;
  const int i = (int)floor(h6);
  const float f = (float)(h6 - (double)(float)i);
  const float fs = (float)((double)ss / 255.0);
  const double vd = (double)v;
  const int p = clip8((int)round(vd * (1.0 - (double)fs)));
  const int q = clip8((int)round(vd * (1.0 - (double)(fs * f))));
  const int t = clip8((int)round(vd * (1.0 - (double)fs * (1.0 - (double)f))));
  switch (i % 6) {
    case 0: r = v, g = t, b = p; break;
    case 1: r = q, g = v, b = p; break;
    case 2: r = p, g = v, b = t; break;
    case 3: r = p, g = q, b = v; break;
    case 4: r = t, g = p, b = v; break;
    default: r = v, g = p, b = q; break;
  }
}

// operations j0 .. j1-1 of a scene's drawn list (4 bits each); `mean` is only read by Contrast
__device__ inline void apply_ops(const int64_t* d, const float* f, int j0, int j1, int mean, int& r, int& g, int& b) {
  const int64_t ops = d[D_OPS];
  for (int j = j0; j < j1; j++) {
    const int op = (int)((ops >> (4 * j)) & 15);
    if (op == OP_BRIGHTNESS) {
      r = blend(0, r, f[0]), g = blend(0, g, f[0]), b = blend(0, b, f[0]);
    } else if (op == OP_CONTRAST) {
      r = blend(mean, r, f[1]), g = blend(mean, g, f[1]), b = blend(mean, b, f[1]);
    } else if (op == OP_COLOR) {
      const int l = luma(r, g, b);
      r = blend(l, r, f[2]), g = blend(l, g, f[2]), b = blend(l, b, f[2]);
    } else {
      hue_shift(r, g, b, (int)d[D_HUE]);
    }
  }
}

// tmp[scene] [tmp_rows][W][3] = horizontal pass over source rows ybox_first .. ybox_first + tmp_rows - 1 of the window
__global__ __launch_bounds__(T) void k_img_hpass(const uint8_t* __restrict__ src, const int64_t* __restrict__ desc,
                                                 const int32_t* __restrict__ coef, int W, uint8_t* __restrict__ tmp) {
  const int64_t* d = desc + (int64_t)blockIdx.y * D_N;
  const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
  if (i >= d[D_TMP_ROWS] * W) return;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  const int32_t* hb = coef + d[D_HCOEF];
  const int kx = (int)d[D_KX];
  const int xmin = hb[2 * x], xmax = hb[2 * x + 1];
  const int32_t* k = hb + 2 * W + (int64_t)x * kx;
  const uint8_t* p = src + d[D_SRC_OFF] + (d[D_YBOX_FIRST] + y) * d[D_SRC_PITCH] + (int64_t)xmin * 3;
  int s0 = 1 << (QBITS - 1), s1 = s0, s2 = s0;
  for (int j = 0; j < xmax; j++) {
    const int w = k[j];
    s0 += (int)p[3 * j] * w;
    s1 += (int)p[3 * j + 1] * w;
    s2 += (int)p[3 * j + 2] * w;
  }
  uint8_t* o = tmp + d[D_TMP_OFF] + i * 3;
  o[0] = (uint8_t)clip_q(s0), o[1] = (uint8_t)clip_q(s1), o[2] = (uint8_t)clip_q(s2);
}

// mid[scene] [H][W][3] = vertical pass + the operations before Contrast; sums[scene] += L of that image when Contrast follows
__global__ __launch_bounds__(T) void k_img_vpass(const int64_t* __restrict__ desc, const int32_t* __restrict__ coef,
                                                 const float* __restrict__ factors, int H, int W, const uint8_t* __restrict__ tmp,
                                                 uint8_t* __restrict__ mid, int64_t* __restrict__ sums) {
  const int sc = blockIdx.y;
  const int64_t* d = desc + (int64_t)sc * D_N;
  const int64_t npix = (int64_t)H * W;
  const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
  const bool contrast = d[D_NPRE] < d[D_NOPS];
  __shared__ unsigned long long block_sum;
  if (threadIdx.x == 0) block_sum = 0;
  if (contrast) __syncthreads();
  if (i < npix) {
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    const int32_t* vb = coef + d[D_VCOEF];
    const int ky = (int)d[D_KY];
    const int ymin = vb[2 * y], ymax = vb[2 * y + 1];
    const int32_t* k = vb + 2 * H + (int64_t)y * ky;
    const uint8_t* p = tmp + d[D_TMP_OFF] + ((int64_t)ymin * W + x) * 3;
    const int64_t pitch = (int64_t)W * 3;
    int s0 = 1 << (QBITS - 1), s1 = s0, s2 = s0;
    for (int j = 0; j < ymax; j++) {
      const int w = k[j];
      s0 += (int)p[j * pitch] * w;
      s1 += (int)p[j * pitch + 1] * w;
      s2 += (int)p[j * pitch + 2] * w;
    }
    int r = clip_q(s0), g = clip_q(s1), b = clip_q(s2);
    apply_ops(d, factors + sc * 4, 0, (int)d[D_NPRE], 0, r, g, b);
    uint8_t* o = mid + (sc * npix + i) * 3;
    o[0] = (uint8_t)r, o[1] = (uint8_t)g, o[2] = (uint8_t)b;
    if (contrast) atomicAdd(&block_sum, (unsigned long long)luma(r, g, b));  // integer sums: exact in any order
  }
  if (contrast) {
    __syncthreads();
    if (threadIdx.x == 0 && block_sum) atomicAdd((unsigned long long*)&sums[sc], block_sum);
  }
}

// img[scene][c][y][flip ? W-1-x : x] = lut[scene][c][Contrast + remaining operations of mid]
__global__ __launch_bounds__(T) void k_img_finish(const int64_t* __restrict__ desc, const float* __restrict__ factors,
                                                  const float* __restrict__ lut, int H, int W, const uint8_t* __restrict__ mid,
                                                  const int64_t* __restrict__ sums, float* __restrict__ img) {
  const int sc = blockIdx.y;
  const int64_t* d = desc + (int64_t)sc * D_N;
  const int64_t npix = (int64_t)H * W;
  const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
  if (i >= npix) return;
  const uint8_t* p = mid + (sc * npix + i) * 3;
  int r = p[0], g = p[1], b = p[2];
  const int npre = (int)d[D_NPRE], nops = (int)d[D_NOPS];
  if (npre < nops) {  // ImageEnhance.Contrast: int(mean of L + 0.5), the mean as Python's int / int true division
    const int mean = (int)((double)sums[sc] / (double)npix + 0.5);
    apply_ops(d, factors + sc * 4, npre, nops, mean, r, g, b);
  }
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  const int xo = d[D_FLIP] ? W - 1 - x : x;
  const float* l = lut + (int64_t)sc * 768;
  float* o = img + (int64_t)sc * 3 * npix + (int64_t)y * W + xo;
  o[0] = l[r];
  o[npix] = l[256 + g];
  o[2 * npix] = l[512 + b];
}
}  // namespace

extern "C" {

// See include/mm2d3d.h.  Every descriptor is checked against the buffer sizes on the host before anything is launched.
int mm_image_prepare(const uint8_t* src, int64_t src_bytes, const int64_t* desc_dev, const int64_t* desc_host, int B, int H, int W,
                     const int32_t* coef, int64_t coef_len, const float* factors, const float* lut, uint8_t* tmp, int64_t tmp_bytes,
                     uint8_t* mid, int64_t* sums, float* img, hipStream_t s) {
  MM_CHECK_ARG(src && desc_dev && desc_host && coef && factors && lut && tmp && mid && sums && img, "image_prepare: null pointer");
  MM_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 30), "image_prepare: bad sizes B=%d H=%d W=%d", B, H, W);
  int64_t max_tmp = 0;
  for (int b = 0; b < B; b++) {
    const int64_t* d = desc_host + (int64_t)b * D_N;
    const int64_t rows = d[D_TMP_ROWS], y0 = d[D_YBOX_FIRST], pitch = d[D_SRC_PITCH], win_w = d[D_WIN_W], win_h = d[D_WIN_H];
    bool ok = rows > 0 && y0 >= 0 && y0 + rows <= win_h && win_w > 0 && pitch >= win_w * 3 && d[D_SRC_OFF] >= 0 &&
              d[D_SRC_OFF] + (win_h - 1) * pitch + win_w * 3 <= src_bytes;
    ok = ok && d[D_KX] > 0 && d[D_KY] > 0 && d[D_HCOEF] >= 0 && d[D_HCOEF] + (int64_t)W * (2 + d[D_KX]) <= coef_len && d[D_VCOEF] >= 0 &&
         d[D_VCOEF] + (int64_t)H * (2 + d[D_KY]) <= coef_len;
    ok = ok && d[D_TMP_OFF] >= 0 && d[D_TMP_OFF] + rows * W * 3 <= tmp_bytes && d[D_NOPS] >= 0 && d[D_NOPS] <= 4 && d[D_NPRE] >= 0 &&
         d[D_NPRE] <= d[D_NOPS] && d[D_HUE] >= 0 && d[D_HUE] < 256;
    for (int j = 0; ok && j < d[D_NOPS]; j++) ok = ((d[D_OPS] >> (4 * j)) & 15) <= OP_HUE && (j != d[D_NPRE] || ((d[D_OPS] >> (4 * j)) & 15) == OP_CONTRAST);
    MM_CHECK_ARG(ok, "image_prepare: descriptor of scene %d does not fit its buffers", b);
    max_tmp = rows > max_tmp ? rows : max_tmp;
  }
  MM_HIP(hipMemsetAsync(sums, 0, (size_t)B * 8, s));
  const int64_t npix = (int64_t)H * W;
  hipLaunchKernelGGL(k_img_hpass, dim3((unsigned)mm_cdiv(max_tmp * W, T), B), dim3(T), 0, s, src, desc_dev, coef, W, tmp);
  hipLaunchKernelGGL(k_img_vpass, dim3((unsigned)mm_cdiv(npix, T), B), dim3(T), 0, s, desc_dev, coef, factors, H, W, tmp, mid, sums);
  hipLaunchKernelGGL(k_img_finish, dim3((unsigned)mm_cdiv(npix, T), B), dim3(T), 0, s, desc_dev, factors, lut, H, W, mid, sums, img);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"
