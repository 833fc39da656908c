// Baseline-JPEG decoder for a batch of camera images (datasets.gpu_batch(..., image="gpu")), bit-exact with what Pillow's
// bundled libjpeg-turbo returns from np.asarray(Image.open(path)).  The host parses the headers and builds the tables
// (mm2d3d_amd/jpeg.py); the file bytes sit in one device buffer.  Stages, each one launch over the whole batch:
//   1. unstuff and split      k_jpg_flags / k_jpg_scatter (+ two exclusive scans): FF 00 -> FF, fill FF dropped, RST0-7
//                             located; k_jpg_intervals / k_jpg_submap: bit length of every restart interval, its lanes
//   2. Huffman decode         one lane per SUBSEQ_BITS of an interval (Weissenberger & Schmidt, ICPP 2018: JPEG's
//                             self-synchronisation).  k_jpg_sync0 decodes every lane from a guessed state; k_jpg_sync (NSYNC
//                             launches) restarts lane k from lane k-1's end state until nothing changes; k_jpg_fix finishes
//                             an interval whose chain is still inconsistent with one lane, sequentially; an exclusive scan of
//                             the blocks begun per lane places them; k_jpg_final writes the coefficients from proven states
//   3. DC prediction          k_jpg_dc: segmented prefix sum of the DC differences per component, reset per interval
//   4. dequantise + IDCT      k_jpg_idct: jidctint.c jpeg_idct_islow, one thread per block -> uint8 component planes
//   5. upsample + colour      k_jpg_color: jdsample.c fancy upsampling, jdcolor.c ycc_rgb_convert -> [H][W][3]
// A lane's state is (bit position in its interval, block slot in the MCU, coefficient index).  Lane k is proven when its
// start state equals lane k-1's end state and lane k-1 is proven; lane 0 of an interval starts from the true state.  A lane
// reads only bytes of its own interval (bits past the interval's end read as 0, as libjpeg fills after a marker) and
// never runs past the interval's end.  Status words per image (MM_JPG_ST_*): invalid marker or restart sequence, invalid
// Huffman code, an interval whose data ran out before its blocks were complete.  Integer arithmetic only.
#pragma clang fp contract(off)
#include "common.h"

#include <algorithm>

namespace {
constexpr int T = 256;
constexpr int SUBSEQ_BITS = 2048;  // mm2d3d_amd/jpeg.py SUBSEQ_BITS
constexpr int NSYNC = 4;           // re-sync launches before the sequential fix-up
constexpr int HUFF_WORDS = 1024;   // fast[512], maxcode[18], valoffset[18], huffval[256] (jpeg.py huff_table)
constexpr int64_t INVALID = -1;    // the end state of a lane whose decode failed (and of every lane started from it)
// descriptor words (include/mm2d3d.h MM_JPG_*; mm2d3d_amd/jpeg.py J_*)
enum { D_SEG_OFF, D_SEG_LEN, D_W, D_H, D_HS, D_VS, D_MCUS_X, D_MCUS_Y, D_RESTART, D_N_IV, D_IV0, D_SUB0, D_SUB_CAP, D_BLK0, D_PLANE_OFF,
       D_OUT_OFF, D_QT0, D_QT1, D_QT2, D_DC0, D_DC1, D_DC2, D_AC0, D_AC1, D_AC2, D_N = 32 };
enum { ST_MARKER = 1, ST_RESTART = 2, ST_HUFFMAN = 4, ST_INCOMPLETE = 8 };

// jutils.c jpeg_natural_order: zigzag index -> natural index, 16 extra entries of 63 for a run past the end of a block
__constant__ uint8_t kNatural[80] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33,
                                     40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36,
                                     29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                                     47, 55, 62, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

// workspace layout, shared by mm_jpeg_ws_bytes and mm_jpeg_decode
struct Layout {
  size_t kept, kscan, mark, mscan, comp, cbase, clen, iv_start, iv_end, iv_img, iv_nsub, iv_fsub, iv_bad, iv_hi, iv_done, sub_iv, start, end0,
      end1, cnt0, cnt1, bscan, coef, planes, scan, total;
  Layout(int B, int64_t data, int64_t niv, int64_t nsub, int64_t nblk, int64_t plane) {
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += mm_align(bytes); return r; };
    kept = take((data + 1) * 4), kscan = take((data + 1) * 4), mark = take((data + 1) * 4), mscan = take((data + 1) * 4);
    comp = take(data + 16), cbase = take(B * 4), clen = take(B * 4);
    iv_start = take(niv * 4), iv_end = take(niv * 4), iv_img = take(niv * 4), iv_nsub = take((niv + 1) * 4), iv_fsub = take((niv + 1) * 4);
    iv_bad = take(niv * 4), iv_hi = take(niv * 4), iv_done = take(niv * 4);
    sub_iv = take(nsub * 4), start = take(nsub * 8), end0 = take(nsub * 8), end1 = take(nsub * 8), cnt0 = take((nsub + 1) * 4),
    cnt1 = take((nsub + 1) * 4), bscan = take((nsub + 1) * 4);
    coef = take(nblk * 128), planes = take(plane);
    int64_t m = data + 1 > nsub + 1 ? data + 1 : nsub + 1;
    m = m > niv + 1 ? m : niv + 1;
    scan = take(mm_scan_ws_bytes(m));
    total = o;
  }
};

__device__ inline int64_t pack(int pos, int slot, int k) { return ((int64_t)pos << 16) | (slot << 8) | k; }

// ---------------------------------------------------------------------------------------------------- 1. unstuff and split
// kept[g] = 1 for a data byte of an entropy-coded segment (FF of FF 00 included), mark[g] = 1 for the FF of an RST marker
__global__ __launch_bounds__(T) void k_jpg_flags(const uint8_t* __restrict__ data, const int64_t* __restrict__ desc,
                                                 int32_t* __restrict__ kept, int32_t* __restrict__ mark, int32_t* __restrict__ status) {
  const int64_t* d = desc + (int64_t)blockIdx.y * D_N;
  const int64_t j = (int64_t)blockIdx.x * T + threadIdx.x, len = d[D_SEG_LEN];
  if (j >= len) return;
  const int64_t g = d[D_SEG_OFF] + j;
  const int b = data[g];
  const int prev = j > 0 ? data[g - 1] : 0;
  const int next = j + 1 < len ? data[g + 1] : 0xFF;  // an FF that ends the segment is fill
  int k = 0, m = 0;
  if (b == 0xFF) {
    k = next == 0x00;
    m = next >= 0xD0 && next <= 0xD7;
    if (!k && !m && next != 0xFF) atomicOr(status + blockIdx.y, ST_MARKER);
  } else if (prev == 0xFF) {  // the 00 of FF 00, or the second byte of a marker
    k = 0;
  } else {
    k = 1;
  }
  kept[g] = k;
  mark[g] = m;
}

// compact bytes of image b at comp[kscan[g]]; interval starts (byte offsets relative to the image's first compact byte)
__global__ __launch_bounds__(T) void k_jpg_scatter(const uint8_t* __restrict__ data, const int64_t* __restrict__ desc,
                                                   const int32_t* __restrict__ kept, const int32_t* __restrict__ kscan,
                                                   const int32_t* __restrict__ mark, const int32_t* __restrict__ mscan,
                                                   uint8_t* __restrict__ comp, int32_t* __restrict__ cbase, int32_t* __restrict__ clen,
                                                   int32_t* __restrict__ iv_start, int32_t* __restrict__ status) {
  const int b = blockIdx.y;
  const int64_t* d = desc + (int64_t)b * D_N;
  const int64_t j = (int64_t)blockIdx.x * T + threadIdx.x, len = d[D_SEG_LEN], s0 = d[D_SEG_OFF];
  const int niv = (int)d[D_N_IV], iv0 = (int)d[D_IV0];
  if (j == 0) {
    cbase[b] = kscan[s0];
    clen[b] = kscan[s0 + len] - kscan[s0];
    iv_start[iv0] = 0;
    if (mscan[s0 + len] - mscan[s0] != niv - 1) atomicOr(status + b, ST_RESTART);
  }
  if (j >= len) return;
  const int64_t g = s0 + j;
  if (kept[g]) comp[kscan[g]] = data[g];
  if (mark[g]) {
    const int idx = mscan[g] - mscan[s0] + 1;  // the interval this marker opens
    if (idx < niv && (data[g + 1] & 7) == ((idx - 1) & 7))
      iv_start[iv0 + idx] = kscan[g] - kscan[s0];
    else
      atomicOr(status + b, ST_RESTART);
  }
}

// per interval: end byte, image, number of lanes (>= 1)
__global__ __launch_bounds__(T) void k_jpg_intervals(const int64_t* __restrict__ desc, const int32_t* __restrict__ clen,
                                                     const int32_t* __restrict__ iv_start, int32_t* __restrict__ iv_end,
                                                     int32_t* __restrict__ iv_img, int32_t* __restrict__ iv_nsub) {
  const int b = blockIdx.y;
  const int64_t* d = desc + (int64_t)b * D_N;
  const int i = blockIdx.x * T + threadIdx.x, niv = (int)d[D_N_IV];
  if (i >= niv) return;
  const int g = (int)d[D_IV0] + i;
  const int s = iv_start[g];
  int e = i + 1 < niv ? iv_start[g + 1] : clen[b];
  e = e < s ? s : e;  // a broken restart sequence (status set): empty interval, its blocks never complete
  iv_end[g] = e;
  iv_img[g] = b;
  const int n = (int)(((int64_t)(e - s) * 8 + SUBSEQ_BITS - 1) / SUBSEQ_BITS);
  iv_nsub[g] = n > 1 ? n : 1;
}

// sub_iv[lane slot] = interval (slots of image b: SUB0 .. SUB0 + SUB_CAP - 1; unused slots stay -1)
__global__ __launch_bounds__(64) void k_jpg_submap(const int64_t* __restrict__ desc, const int32_t* __restrict__ iv_img,
                                                   const int32_t* __restrict__ iv_nsub, const int32_t* __restrict__ iv_fsub,
                                                   int32_t* __restrict__ sub_iv, int32_t* __restrict__ status) {
  const int iv = blockIdx.x;
  const int b = iv_img[iv];
  const int64_t* d = desc + (int64_t)b * D_N;
  const int64_t f = iv_fsub[iv] - iv_fsub[d[D_IV0]], n = iv_nsub[iv];
  if (f + n > d[D_SUB_CAP]) {
    if (threadIdx.x == 0) atomicOr(status + b, ST_RESTART);
    return;
  }
  for (int64_t j = threadIdx.x; j < n; j += 64) sub_iv[d[D_SUB0] + f + j] = iv;
}

// ---------------------------------------------------------------------------------------------------- 2. Huffman decode
struct Lane {
  const uint8_t* p;  // first byte of the interval
  int nbytes, nbits;
  const int32_t* dc[3];
  const int32_t* ac[3];
  int nluma, bpm;
};

__device__ inline int huff_extend(int v, int s) { return s && v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// Decodes from state (pos, slot, k) until pos >= stop (jdhuff.c decode_mcu_slow / jpeg_huff_decode, one symbol per step).
// Returns the number of blocks begun.  WRITE: coefficients (DC difference at [0]) of block `nb` go to coef + (blk0 + nb) * 64
// until `nblk` blocks are complete; done = 1 then.  err: 1 invalid Huffman code, 2 ran past the end of the interval.
template <bool WRITE>
__device__ int decode_run(const Lane& L, int& pos, int& slot, int& k, int stop, int& err, int16_t* __restrict__ coef, int64_t blk0,
                          int nb, int nblk, int& done) {
  int begun = 0;
  int byte = pos >> 3;
  uint64_t acc = 0;
  int have = 0;
  auto refill = [&]() {
    while (have <= 56) {
      const uint64_t v = byte < L.nbytes ? L.p[byte] : 0;
      acc |= v << (56 - have);
      byte++;
      have += 8;
    }
  };
  refill();
  acc <<= (pos & 7);
  have -= pos & 7;
  while (true) {
    if (WRITE && k == 0 && nb == nblk) {
      done = 1;
      break;
    }
    if (pos >= stop) break;
    refill();
    const int c = slot < L.nluma ? 0 : slot - L.nluma + 1;
    const int32_t* t = k == 0 ? L.dc[c] : L.ac[c];
    const int w = (int)(acc >> 48);
    int e = t[w >> 7], len, sym;
    if (e) {
      len = e >> 8, sym = e & 255;
    } else {
      len = 10;
      while (len <= 16 && (w >> (16 - len)) > t[512 + len]) len++;
      if (len > 16) {
        err = 1;
        break;
      }
      sym = t[548 + (((w >> (16 - len)) + t[530 + len]) & 255)];
    }
    acc <<= len;
    int used = len;
    const int s = k == 0 ? sym : (sym & 15);
    int v = 0;
    if (s) {
      v = huff_extend((int)(acc >> (64 - s)), s);
      acc <<= s;
      used += s;
    }
    have -= used;
    pos += used;
    if (pos > L.nbits) {
      err = 2;
      break;
    }
    if (k == 0) {
      if (WRITE) coef[(blk0 + nb) * 64] = (int16_t)v;
      nb++;
      begun++;
      k = 1;
    } else {
      const int r = sym >> 4;
      if (s) {
        k += r;
        if (WRITE) coef[(blk0 + nb - 1) * 64 + kNatural[k < 79 ? k : 79]] = (int16_t)v;
        k++;
      } else {
        k = r == 15 ? k + 16 : 64;
      }
    }
    if (k >= 64) {
      k = 0;
      if (++slot == L.bpm) slot = 0;
    }
  }
  return begun;
}

// the lane of slot g: its interval, its index j in the interval, the interval's data and tables; false for an unused slot
__device__ inline bool lane_of(int64_t g, const int64_t* __restrict__ desc, const int32_t* __restrict__ sub_iv,
                               const int32_t* __restrict__ iv_start, const int32_t* __restrict__ iv_end,
                               const int32_t* __restrict__ iv_img, const int32_t* __restrict__ iv_fsub,
                               const int32_t* __restrict__ cbase, const uint8_t* __restrict__ comp,
                               const int32_t* __restrict__ huff, Lane& L, int& iv, int64_t& j, const int64_t*& d) {
  iv = sub_iv[g];
  if (iv < 0) return false;
  const int b = iv_img[iv];
  d = desc + (int64_t)b * D_N;
  j = g - (d[D_SUB0] + iv_fsub[iv] - iv_fsub[d[D_IV0]]);
  L.p = comp + cbase[b] + iv_start[iv];
  L.nbytes = iv_end[iv] - iv_start[iv];
  L.nbits = L.nbytes * 8;
  for (int c = 0; c < 3; c++) {
    L.dc[c] = huff + d[D_DC0 + c] * HUFF_WORDS;
    L.ac[c] = huff + d[D_AC0 + c] * HUFF_WORDS;
  }
  L.nluma = (int)(d[D_HS] * d[D_VS]);
  L.bpm = L.nluma + 2;
  return true;
}

#define LANE_ARGS                                                                                                                     \
  const int64_t *__restrict__ desc, const int32_t *__restrict__ sub_iv, const int32_t *__restrict__ iv_start,                       \
      const int32_t *__restrict__ iv_end, const int32_t *__restrict__ iv_img, const int32_t *__restrict__ iv_fsub,                  \
      const int32_t *__restrict__ cbase, const uint8_t *__restrict__ comp, const int32_t *__restrict__ huff
#define LANE_PASS desc, sub_iv, iv_start, iv_end, iv_img, iv_fsub, cbase, comp, huff

__device__ inline int64_t run_from(const Lane& L, int64_t st, int64_t j, int& cnt) {
  cnt = 0;
  if (st == INVALID) return INVALID;
  int pos = (int)(st >> 16), slot = (int)((st >> 8) & 255), k = (int)(st & 255), err = 0, done = 0;
  const int stop = (int)((j + 1) * SUBSEQ_BITS < L.nbits ? (j + 1) * SUBSEQ_BITS : L.nbits);
  cnt = decode_run<false>(L, pos, slot, k, stop, err, nullptr, 0, 0, 0, done);
  return err ? INVALID : pack(pos, slot, k);
}

// every lane from a guessed state.  Lane 0 of an interval starts from the true state; lane j > 0 first decodes lane j-1's bits
// from (slot 0, coefficient 0) as a warm-up and starts from the state it reaches at the first symbol boundary at or past
// j * SUBSEQ_BITS - the same boundary at which lane j-1 stops, so a warm-up that has synchronised gives lane j-1's true end
// state (lane 1 warms up from the interval's true start).  A lane that does not synchronise within SUBSEQ_BITS is wrong
// about the MCU block slot most often: the four luma blocks of 4:2:0 share one table pair, Cb and Cr the other, so a slot
// offset survives until the luma / chroma pattern differs.  Without the warm-up about one lane in five was still
// unsynchronised at its end; with it, about one in twenty.
__global__ __launch_bounds__(T) void k_jpg_sync0(LANE_ARGS, int64_t nsub, int64_t* __restrict__ start, int64_t* __restrict__ end,
                                                 int32_t* __restrict__ cnt) {
  const int64_t g = (int64_t)blockIdx.x * T + threadIdx.x;
  if (g >= nsub) return;
  Lane L;
  int iv;
  int64_t j;
  const int64_t* d;
  if (!lane_of(g, LANE_PASS, L, iv, j, d)) return;
  int64_t st = pack(0, 0, 0);
  if (j > 0) {
    int pos = (int)((j - 1) * SUBSEQ_BITS), slot = 0, k = 0, err = 0, done = 0;
    decode_run<false>(L, pos, slot, k, (int)(j * SUBSEQ_BITS), err, nullptr, 0, 0, 0, done);
    st = err ? pack((int)(j * SUBSEQ_BITS), 0, 0) : pack(pos, slot, k);
  }
  int c;
  start[g] = st;
  end[g] = run_from(L, st, j, c);
  cnt[g] = c;
}

// one re-sync round: lane j restarts from lane j-1's end state of the previous round when that differs from its own start
__global__ __launch_bounds__(T) void k_jpg_sync(LANE_ARGS, int64_t nsub, int64_t* __restrict__ start, const int64_t* __restrict__ end_in,
                                                const int32_t* __restrict__ cnt_in, int64_t* __restrict__ end_out,
                                                int32_t* __restrict__ cnt_out) {
  const int64_t g = (int64_t)blockIdx.x * T + threadIdx.x;
  if (g >= nsub) return;
  Lane L;
  int iv;
  int64_t j;
  const int64_t* d;
  if (!lane_of(g, LANE_PASS, L, iv, j, d)) return;
  const int64_t st = j > 0 ? end_in[g - 1] : start[g];
  if (st == start[g]) {
    end_out[g] = end_in[g];
    cnt_out[g] = cnt_in[g];
    return;
  }
  int c;
  start[g] = st;
  end_out[g] = run_from(L, st, j, c);
  cnt_out[g] = c;
}

__global__ __launch_bounds__(T) void k_jpg_check(const int32_t* __restrict__ sub_iv, const int32_t* __restrict__ iv_fsub,
                                                 const int32_t* __restrict__ iv_img, const int64_t* __restrict__ desc, int64_t nsub,
                                                 const int64_t* __restrict__ start, const int64_t* __restrict__ end,
                                                 int32_t* __restrict__ iv_bad, int32_t* __restrict__ iv_hi) {
  const int64_t g = (int64_t)blockIdx.x * T + threadIdx.x;
  if (g >= nsub) return;
  const int iv = sub_iv[g];
  if (iv < 0) return;
  const int64_t* d = desc + (int64_t)iv_img[iv] * D_N;
  const int64_t j = g - (d[D_SUB0] + iv_fsub[iv] - iv_fsub[d[D_IV0]]);
  if (j > 0 && start[g] != end[g - 1]) {  // the inconsistent lanes of the interval lie within [iv_bad, iv_hi]
    atomicMin(iv_bad + iv, (int)j);
    atomicMax(iv_hi + iv, (int)j);
  }
}

// an interval whose chain is still inconsistent: one lane walks it in order from its first inconsistent lane, past the last one
// until a lane's start no longer changes (bounded by the interval's length).  One workgroup per interval, so that the walks of
// different images run side by side instead of in the lanes of one wavefront, one after another.
__global__ __launch_bounds__(64) void k_jpg_fix(LANE_ARGS, const int32_t* __restrict__ iv_nsub, const int32_t* __restrict__ iv_bad,
                                                const int32_t* __restrict__ iv_hi, int64_t* __restrict__ start, int64_t* __restrict__ end,
                                                int32_t* __restrict__ cnt) {
  const int iv = blockIdx.x;
  if (threadIdx.x != 0 || iv_bad[iv] == 0x7FFFFFFF) return;
  const int b = iv_img[iv];
  const int64_t* d = desc + (int64_t)b * D_N;
  const int64_t g0 = d[D_SUB0] + iv_fsub[iv] - iv_fsub[d[D_IV0]];
  Lane L;
  int iv2;
  int64_t j;
  const int64_t* d2;
  if (!lane_of(g0, LANE_PASS, L, iv2, j, d2)) return;
  const int hi = iv_hi[iv];
  int64_t prev = end[g0 + iv_bad[iv] - 1];  // the end state of the lane before, carried in a register
  for (int64_t jj = iv_bad[iv]; jj < iv_nsub[iv]; jj++) {
    const int64_t g = g0 + jj;
    if (prev == start[g]) {
      if (jj > hi) break;  // this lane and every later one are consistent
      prev = end[g];
      continue;
    }
    int c;
    start[g] = prev;
    prev = end[g] = run_from(L, prev, jj, c);
    cnt[g] = c;
  }
}

// every lane from its proven start state: the coefficients of its blocks (coef zero-filled before); iv_done when complete
__global__ __launch_bounds__(T) void k_jpg_final(LANE_ARGS, int64_t nsub, const int64_t* __restrict__ start, const int32_t* __restrict__ bscan,
                                                 int16_t* __restrict__ coef, int32_t* __restrict__ iv_done, int32_t* __restrict__ status) {
  const int64_t g = (int64_t)blockIdx.x * T + threadIdx.x;
  if (g >= nsub) return;
  Lane L;
  int iv;
  int64_t j;
  const int64_t* d;
  if (!lane_of(g, LANE_PASS, L, iv, j, d)) return;
  const int64_t st = start[g];
  if (st == INVALID) return;  // the chain failed before this lane: the interval does not complete (k_jpg_status)
  const int64_t mcus = d[D_MCUS_X] * d[D_MCUS_Y], ri = d[D_RESTART] ? d[D_RESTART] : mcus;
  const int64_t i = iv - d[D_IV0];
  const int64_t mcu0 = i * ri, imcus = mcus - mcu0 < ri ? mcus - mcu0 : ri;
  const int nblk = (int)(imcus * L.bpm);
  const int nb = bscan[g] - bscan[g - j];
  int pos = (int)(st >> 16), slot = (int)((st >> 8) & 255), k = (int)(st & 255), err = 0, done = 0;
  if (nb > nblk || (k != 0 && nb == 0)) return;  // past the interval's last block (padding decoded by the sync passes)
  const int stop = (int)((j + 1) * SUBSEQ_BITS < L.nbits ? (j + 1) * SUBSEQ_BITS : L.nbits);
  decode_run<true>(L, pos, slot, k, stop, err, coef, d[D_BLK0] + mcu0 * L.bpm, nb, nblk, done);
  if (err == 1) atomicOr(status + (d - desc) / D_N, ST_HUFFMAN);
  if (done) iv_done[iv] = 1;
}

__global__ __launch_bounds__(T) void k_jpg_status(const int32_t* __restrict__ iv_img, const int32_t* __restrict__ iv_done, int niv,
                                                  int32_t* __restrict__ status) {
  const int iv = blockIdx.x * T + threadIdx.x;
  if (iv < niv && !iv_done[iv]) atomicOr(status + iv_img[iv], ST_INCOMPLETE);
}

// ---------------------------------------------------------------------------------------------------- 3. DC prediction
// One workgroup per (component, image): inclusive segmented scan of the DC differences of the component's blocks in scan
// order, reset at the first block of every restart interval (jdhuff.c process_restart zeroes last_dc_val).
constexpr int DC_T = 1024;
__global__ __launch_bounds__(DC_T) void k_jpg_dc(const int64_t* __restrict__ desc, int16_t* __restrict__ coef) {
  const int c = blockIdx.x;
  const int64_t* d = desc + (int64_t)blockIdx.y * D_N;
  const int nluma = (int)(d[D_HS] * d[D_VS]), bpm = nluma + 2;
  const int nbc = c == 0 ? nluma : 1, off = c == 0 ? 0 : nluma + c - 1;
  const int64_t mcus = d[D_MCUS_X] * d[D_MCUS_Y], ri = d[D_RESTART];
  const int64_t n = mcus * nbc;
  __shared__ int val[DC_T];
  __shared__ int flg[DC_T];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  for (int64_t base = 0; base < n; base += DC_T) {
    const int64_t i = base + threadIdx.x;
    int v = 0, f = 0;
    int64_t blk = 0;
    if (i < n) {
      const int64_t mcu = i / nbc, e = i - mcu * nbc;
      blk = d[D_BLK0] + mcu * bpm + off + e;
      v = coef[blk * 64];
      f = e == 0 && ri && mcu % ri == 0;
    }
    __syncthreads();  // carry of the previous chunk is visible
    if (threadIdx.x == 0 && !f) v += carry;
    val[threadIdx.x] = v;
    flg[threadIdx.x] = f;
    __syncthreads();
    for (int s = 1; s < DC_T; s <<= 1) {  // (f1, v1) + (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2)
      int pv = 0, pf = 0;
      if (threadIdx.x >= s) pv = val[threadIdx.x - s], pf = flg[threadIdx.x - s];
      __syncthreads();
      if (threadIdx.x >= s && !f) v += pv, f |= pf;
      val[threadIdx.x] = v;
      flg[threadIdx.x] = f;
      __syncthreads();
    }
    if (i < n) coef[blk * 64] = (int16_t)v;
    if (threadIdx.x == DC_T - 1) carry = v;
  }
}

// ---------------------------------------------------------------------------------------------------- 4. islow IDCT
// jidctint.c jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2, DESCALE rounding, range_limit[x & RANGE_MASK] of the post-IDCT
// table (jdmaster.c prepare_range_limit_table: CENTERJSAMPLE added, values wrapped mod 1024 and clamped to 0..255)
constexpr int CB = 13, P1 = 2;
__device__ inline void idct8(int32_t x0, int32_t x1, int32_t x2, int32_t x3, int32_t x4, int32_t x5, int32_t x6, int32_t x7, int sh,
                             int32_t* o) {
  int32_t z1 = (x2 + x6) * 4433;                // FIX_0_541196100
  const int32_t tmp2 = z1 + x6 * -15137;        // FIX_1_847759065
  const int32_t tmp3 = z1 + x2 * 6270;          // FIX_0_765366865
  const int32_t tmp0 = (x0 + x4) * (1 << CB), tmp1 = (x0 - x4) * (1 << CB);
  const int32_t t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
  int32_t t0 = x7, t1 = x5, t2 = x3, t3 = x1;
  z1 = t0 + t3;
  int32_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int32_t z5 = (z3 + z4) * 9633;          // FIX_1_175875602
  t0 *= 2446, t1 *= 16819, t2 *= 25172, t3 *= 12299;  // FIX_0_298631336, FIX_2_053119869, FIX_3_072711026, FIX_1_501321110
  z1 *= -7373, z2 *= -20995;                    // FIX_0_899976223, FIX_2_562915447
  z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;  // FIX_1_961570560, FIX_0_390180644
  t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
  const int32_t r = 1 << (sh - 1);
  o[0] = (t10 + t3 + r) >> sh, o[7] = (t10 - t3 + r) >> sh;
  o[1] = (t11 + t2 + r) >> sh, o[6] = (t11 - t2 + r) >> sh;
  o[2] = (t12 + t1 + r) >> sh, o[5] = (t12 - t1 + r) >> sh;
  o[3] = (t13 + t0 + r) >> sh, o[4] = (t13 - t0 + r) >> sh;
}

__device__ inline int64_t plane_width(const int64_t* d, int c) { return d[D_MCUS_X] * 8 * (c == 0 ? d[D_HS] : 1); }
__device__ inline int64_t plane_off(const int64_t* d, int c) {
  const int64_t y = d[D_MCUS_X] * d[D_HS] * 8 * d[D_MCUS_Y] * d[D_VS] * 8, ch = d[D_MCUS_X] * 8 * d[D_MCUS_Y] * 8;
  return d[D_PLANE_OFF] + (c == 0 ? 0 : y + (c - 1) * ch);
}

// one thread per block of image blockIdx.y: dequantise, IDCT, 8x8 samples into the component's plane
__global__ __launch_bounds__(T) void k_jpg_idct(const int64_t* __restrict__ desc, const int32_t* __restrict__ qt,
                                                const int16_t* __restrict__ coef, uint8_t* __restrict__ planes) {
  const int64_t* d = desc + (int64_t)blockIdx.y * D_N;
  const int nluma = (int)(d[D_HS] * d[D_VS]), bpm = nluma + 2;
  const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x, mx = d[D_MCUS_X];
  if (i >= mx * d[D_MCUS_Y] * bpm) return;
  const int64_t mcu = i / bpm;
  const int slot = (int)(i - mcu * bpm);
  const int c = slot < nluma ? 0 : slot - nluma + 1;
  const int hs = c == 0 ? (int)d[D_HS] : 1, vs = c == 0 ? (int)d[D_VS] : 1;
  const int e = c == 0 ? slot : 0;
  const int64_t bx = (mcu % mx) * hs + e % hs, by = (mcu / mx) * vs + e / hs;
  const int32_t* q = qt + d[D_QT0 + c] * 64;
  const int16_t* in = coef + (d[D_BLK0] + i) * 64;
  int16_t x[64];
#pragma unroll
  for (int v = 0; v < 8; v++) {
    const int4 w = *reinterpret_cast<const int4*>(in + v * 8);
    const int16_t* h = reinterpret_cast<const int16_t*>(&w);
#pragma unroll
    for (int u = 0; u < 8; u++) x[v * 8 + u] = h[u];
  }
  int32_t ws[64], o[8];
#pragma unroll
  for (int u = 0; u < 8; u++) {  // pass 1: columns
    idct8(x[u] * q[u], x[8 + u] * q[8 + u], x[16 + u] * q[16 + u], x[24 + u] * q[24 + u], x[32 + u] * q[32 + u], x[40 + u] * q[40 + u],
          x[48 + u] * q[48 + u], x[56 + u] * q[56 + u], CB - P1, o);
#pragma unroll
    for (int v = 0; v < 8; v++) ws[v * 8 + u] = o[v];
  }
  const int64_t pw = plane_width(d, c);
  uint8_t* out = planes + plane_off(d, c) + by * 8 * pw + bx * 8;
#pragma unroll
  for (int v = 0; v < 8; v++) {  // pass 2: rows
    idct8(ws[v * 8], ws[v * 8 + 1], ws[v * 8 + 2], ws[v * 8 + 3], ws[v * 8 + 4], ws[v * 8 + 5], ws[v * 8 + 6], ws[v * 8 + 7],
          CB + P1 + 3, o);
    uint64_t row = 0;
#pragma unroll
    for (int u = 0; u < 8; u++) {
      int s = ((o[u] & 1023) ^ 512) - 512 + 128;
      s = s < 0 ? 0 : s > 255 ? 255 : s;
      row |= (uint64_t)s << (8 * u);
    }
    *reinterpret_cast<uint64_t*>(out + v * pw) = row;
  }
}

// ---------------------------------------------------------------------------------------------------- 5. upsample + colour
// jdsample.c h2v1_fancy_upsample / h2v2_fancy_upsample when the downsampled width is > 2, else h2v1_upsample / h2v2_upsample;
// context rows above the first and below the last real row replicate it (jdmainct.c make_funny_pointers /
// set_bottom_pointers).  Then jdcolor.c ycc_rgb_convert with build_ycc_rgb_table's values (SCALEBITS 16, ONE_HALF).
__device__ inline int chroma(const uint8_t* __restrict__ p, int64_t pw, int x, int y, int hs, int vs, int dw, int dh) {
  if (hs == 1) return p[(int64_t)y * pw + x];
  const int i = x >> 1;
  if (dw <= 2) return p[(int64_t)(y >> (vs - 1)) * pw + i];
  if (vs == 1) {
    const uint8_t* r = p + (int64_t)y * pw;
    const int v = r[i] * 3;
    if (x & 1) return i == dw - 1 ? r[i] : (v + r[i + 1] + 2) >> 2;
    return i == 0 ? r[0] : (v + r[i - 1] + 1) >> 2;
  }
  const int yi = y >> 1;
  int yf = (y & 1) ? yi + 1 : yi - 1;
  yf = yf < 0 ? 0 : yf >= dh ? dh - 1 : yf;
  const uint8_t *r0 = p + (int64_t)yi * pw, *r1 = p + (int64_t)yf * pw;
  const int cs = r0[i] * 3 + r1[i];
  if (x & 1) return i == dw - 1 ? (cs * 4 + 7) >> 4 : (cs * 3 + r0[i + 1] * 3 + r1[i + 1] + 7) >> 4;
  return i == 0 ? (cs * 4 + 8) >> 4 : (cs * 3 + r0[i - 1] * 3 + r1[i - 1] + 8) >> 4;
}

__device__ inline uint8_t clamp255(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

__global__ __launch_bounds__(T) void k_jpg_color(const int64_t* __restrict__ desc, const uint8_t* __restrict__ planes,
                                                 uint8_t* __restrict__ out) {
  const int64_t* d = desc + (int64_t)blockIdx.y * D_N;
  const int W = (int)d[D_W], H = (int)d[D_H];
  const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;
  if (i >= (int64_t)W * H) return;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  const int hs = (int)d[D_HS], vs = (int)d[D_VS];
  const int dw = (W + hs - 1) / hs, dh = (H + vs - 1) / vs;
  const int Y = planes[plane_off(d, 0) + (int64_t)y * plane_width(d, 0) + x];
  const int cb = chroma(planes + plane_off(d, 1), plane_width(d, 1), x, y, hs, vs, dw, dh) - 128;
  const int cr = chroma(planes + plane_off(d, 2), plane_width(d, 2), x, y, hs, vs, dw, dh) - 128;
  uint8_t* o = out + d[D_OUT_OFF] + i * 3;
  o[0] = clamp255(Y + ((91881 * cr + 32768) >> 16));                    // Cr_r_tab: FIX(1.40200)
  o[1] = clamp255(Y + ((-46802 * cr + (-22554 * cb + 32768)) >> 16));  // Cr_g_tab + Cb_g_tab: FIX(0.71414), FIX(0.34414)
  o[2] = clamp255(Y + ((116130 * cb + 32768) >> 16));                   // Cb_b_tab: FIX(1.77200)
}

struct Totals {
  int64_t niv = 0, nsub = 0, nblk = 0, plane = 0, max_seg = 0, max_iv = 0, max_blk = 0, max_pix = 0;
};
}  // namespace

extern "C" {

size_t mm_jpeg_ws_bytes(int B, int64_t data_bytes, int64_t n_intervals, int64_t n_lanes, int64_t n_blocks, int64_t plane_bytes) {
  return Layout(B, data_bytes, n_intervals, n_lanes, n_blocks, plane_bytes).total;
}

// See include/mm2d3d.h.  Every descriptor is checked against the buffer sizes on the host before anything is launched.
int mm_jpeg_decode(const uint8_t* data, int64_t data_bytes, const int64_t* desc_dev, const int64_t* desc_host, int B, const int32_t* huff,
                   int64_t n_huff, const int32_t* qt, int64_t n_qt, uint8_t* out, int64_t out_bytes, int32_t* status, void* ws,
                   size_t ws_bytes, hipStream_t s) {
  MM_CHECK_ARG(data && desc_dev && desc_host && huff && qt && out && status && ws, "jpeg_decode: null pointer");
  MM_CHECK_ARG(B > 0 && B <= 65535 && data_bytes > 0 && data_bytes < ((int64_t)1 << 31), "jpeg_decode: bad sizes B=%d data_bytes=%lld", B,
               (long long)data_bytes);
  Totals t;
  for (int b = 0; b < B; b++) {
    const int64_t* d = desc_host + (int64_t)b * D_N;
    const int64_t W = d[D_W], H = d[D_H], hs = d[D_HS], vs = d[D_VS], mx = d[D_MCUS_X], my = d[D_MCUS_Y], ri = d[D_RESTART];
    // bit positions are int: a segment stays below 2^28 bytes
    bool ok = d[D_SEG_OFF] >= 0 && d[D_SEG_LEN] >= 0 && d[D_SEG_LEN] < ((int64_t)1 << 28) && d[D_SEG_OFF] + d[D_SEG_LEN] <= data_bytes;
    ok = ok && W > 0 && H > 0 && W <= 65535 && H <= 65535 && (hs == 1 || hs == 2) && (vs == 1 || vs == 2) && vs <= hs;
    ok = ok && mx == mm_cdiv(W, 8 * hs) && my == mm_cdiv(H, 8 * vs) && ri >= 0 && ri <= 65535;
    const int64_t mcus = mx * my, bpm = hs * vs + 2;
    ok = ok && d[D_N_IV] == (ri ? mm_cdiv(mcus, ri) : 1) && d[D_IV0] >= 0 && d[D_SUB0] >= 0 && d[D_BLK0] >= 0 && d[D_PLANE_OFF] >= 0;
    ok = ok && d[D_SUB_CAP] >= mm_cdiv(d[D_SEG_LEN] * 8, SUBSEQ_BITS) + d[D_N_IV];
    ok = ok && d[D_OUT_OFF] >= 0 && d[D_OUT_OFF] + W * H * 3 <= out_bytes;
    for (int c = 0; c < 3; c++)
      ok = ok && d[D_QT0 + c] >= 0 && d[D_QT0 + c] < n_qt && d[D_DC0 + c] >= 0 && d[D_DC0 + c] < n_huff && d[D_AC0 + c] >= 0 &&
           d[D_AC0 + c] < n_huff;
    MM_CHECK_ARG(ok, "jpeg_decode: descriptor of image %d is inconsistent", b);
    const int64_t plane = mx * hs * 8 * my * vs * 8 + 2 * mx * 8 * my * 8;
    t.niv = std::max(t.niv, d[D_IV0] + d[D_N_IV]);
    t.nsub = std::max(t.nsub, d[D_SUB0] + d[D_SUB_CAP]);
    t.nblk = std::max(t.nblk, d[D_BLK0] + mcus * bpm);
    t.plane = std::max(t.plane, d[D_PLANE_OFF] + plane);
    t.max_seg = std::max(t.max_seg, d[D_SEG_LEN]);
    t.max_iv = std::max(t.max_iv, d[D_N_IV]);
    t.max_blk = std::max(t.max_blk, mcus * bpm);
    t.max_pix = std::max(t.max_pix, W * H);
  }
  MM_CHECK_ARG(t.niv < ((int64_t)1 << 31) && t.nsub < ((int64_t)1 << 31), "jpeg_decode: too many intervals / lanes");
  // images must not share intervals, lanes, blocks or planes
  for (int a = 0; a < B; a++)
    for (int b = a + 1; b < B; b++) {
      const int64_t *da = desc_host + (int64_t)a * D_N, *db = desc_host + (int64_t)b * D_N;
      auto apart = [](int64_t a0, int64_t an, int64_t b0, int64_t bn) { return a0 + an <= b0 || b0 + bn <= a0; };
      const int64_t ba = da[D_MCUS_X] * da[D_MCUS_Y] * (da[D_HS] * da[D_VS] + 2), bb = db[D_MCUS_X] * db[D_MCUS_Y] * (db[D_HS] * db[D_VS] + 2);
      MM_CHECK_ARG(apart(da[D_IV0], da[D_N_IV], db[D_IV0], db[D_N_IV]) && apart(da[D_SUB0], da[D_SUB_CAP], db[D_SUB0], db[D_SUB_CAP]) &&
                       apart(da[D_BLK0], ba, db[D_BLK0], bb) && apart(da[D_SEG_OFF], da[D_SEG_LEN], db[D_SEG_OFF], db[D_SEG_LEN]),
                   "jpeg_decode: images %d and %d overlap", a, b);
    }
  const Layout Lo(B, data_bytes, t.niv, t.nsub, t.nblk, t.plane);
  if (ws_bytes < Lo.total) {
    mm_set_error("jpeg_decode: workspace too small: %zu < %zu", ws_bytes, Lo.total);
    return MM_ERR_WORKSPACE;
  }
  char* w = (char*)ws;
  int32_t *kept = (int32_t*)(w + Lo.kept), *kscan = (int32_t*)(w + Lo.kscan), *mark = (int32_t*)(w + Lo.mark), *mscan = (int32_t*)(w + Lo.mscan);
  uint8_t* comp = (uint8_t*)(w + Lo.comp);
  int32_t *cbase = (int32_t*)(w + Lo.cbase), *clen = (int32_t*)(w + Lo.clen);
  int32_t *iv_start = (int32_t*)(w + Lo.iv_start), *iv_end = (int32_t*)(w + Lo.iv_end), *iv_img = (int32_t*)(w + Lo.iv_img);
  int32_t *iv_nsub = (int32_t*)(w + Lo.iv_nsub), *iv_fsub = (int32_t*)(w + Lo.iv_fsub), *iv_bad = (int32_t*)(w + Lo.iv_bad);
  int32_t *iv_hi = (int32_t*)(w + Lo.iv_hi), *iv_done = (int32_t*)(w + Lo.iv_done), *sub_iv = (int32_t*)(w + Lo.sub_iv);
  int64_t *start = (int64_t*)(w + Lo.start), *end[2] = {(int64_t*)(w + Lo.end0), (int64_t*)(w + Lo.end1)};
  int32_t* cnt[2] = {(int32_t*)(w + Lo.cnt0), (int32_t*)(w + Lo.cnt1)};
  int32_t* bscan = (int32_t*)(w + Lo.bscan);
  int16_t* coef = (int16_t*)(w + Lo.coef);
  uint8_t* planes = (uint8_t*)(w + Lo.planes);
  void* sws = w + Lo.scan;
  const size_t sws_bytes = Lo.total - Lo.scan;

  MM_HIP(hipMemsetAsync(status, 0, (size_t)B * 4, s));
  MM_HIP(hipMemsetAsync(kept, 0, Lo.mscan + (size_t)(data_bytes + 1) * 4 - Lo.kept, s));  // kept, kscan, mark, mscan
  MM_HIP(hipMemsetAsync(comp, 0, (size_t)data_bytes + 16, s));
  MM_HIP(hipMemsetAsync(iv_start, 0, (size_t)t.niv * 4, s));
  MM_HIP(hipMemsetAsync(iv_nsub, 0, (size_t)(t.niv + 1) * 4, s));
  MM_HIP(hipMemsetAsync(iv_bad, 0x7F, (size_t)t.niv * 4, s));  // 0x7FFFFFFF: no inconsistent lane
  MM_HIP(hipMemsetAsync(iv_hi, 0, (size_t)t.niv * 4, s));
  MM_HIP(hipMemsetAsync(iv_done, 0, (size_t)t.niv * 4, s));
  MM_HIP(hipMemsetAsync(iv_img, 0, (size_t)t.niv * 4, s));
  MM_HIP(hipMemsetAsync(sub_iv, 0xFF, (size_t)t.nsub * 4, s));
  MM_HIP(hipMemsetAsync(cnt[0], 0, (size_t)(t.nsub + 1) * 4, s));
  MM_HIP(hipMemsetAsync(cnt[1], 0, (size_t)(t.nsub + 1) * 4, s));
  MM_HIP(hipMemsetAsync(coef, 0, (size_t)t.nblk * 128, s));

  // 1. unstuff and split
  const dim3 gseg((unsigned)mm_cdiv(t.max_seg + 1, T), B);
  hipLaunchKernelGGL(k_jpg_flags, gseg, dim3(T), 0, s, data, desc_dev, kept, mark, status);
  MM_LAUNCH_CHECK();
  int rc;
  if ((rc = mm_exclusive_scan_i32(kept, kscan, data_bytes + 1, nullptr, sws, sws_bytes, s, 1)) != MM_OK) return rc;
  if ((rc = mm_exclusive_scan_i32(mark, mscan, data_bytes + 1, nullptr, sws, sws_bytes, s, 1)) != MM_OK) return rc;
  hipLaunchKernelGGL(k_jpg_scatter, gseg, dim3(T), 0, s, data, desc_dev, kept, kscan, mark, mscan, comp, cbase, clen, iv_start, status);
  hipLaunchKernelGGL(k_jpg_intervals, dim3((unsigned)mm_cdiv(t.max_iv, T), B), dim3(T), 0, s, desc_dev, clen, iv_start, iv_end, iv_img,
                     iv_nsub);
  MM_LAUNCH_CHECK();
  if ((rc = mm_exclusive_scan_i32(iv_nsub, iv_fsub, t.niv + 1, nullptr, sws, sws_bytes, s, 1)) != MM_OK) return rc;
  hipLaunchKernelGGL(k_jpg_submap, dim3((unsigned)t.niv), dim3(64), 0, s, desc_dev, iv_img, iv_nsub, iv_fsub, sub_iv, status);

  // 2. Huffman decode
  const dim3 gsub((unsigned)mm_cdiv(t.nsub, T));
  hipLaunchKernelGGL(k_jpg_sync0, gsub, dim3(T), 0, s, desc_dev, sub_iv, iv_start, iv_end, iv_img, iv_fsub, cbase, comp, huff, t.nsub, start,
                     end[0], cnt[0]);
  for (int r = 1; r <= NSYNC; r++)
    hipLaunchKernelGGL(k_jpg_sync, gsub, dim3(T), 0, s, desc_dev, sub_iv, iv_start, iv_end, iv_img, iv_fsub, cbase, comp, huff, t.nsub,
                       start, end[(r - 1) & 1], cnt[(r - 1) & 1], end[r & 1], cnt[r & 1]);
  int64_t* endf = end[NSYNC & 1];
  int32_t* cntf = cnt[NSYNC & 1];
  hipLaunchKernelGGL(k_jpg_check, gsub, dim3(T), 0, s, sub_iv, iv_fsub, iv_img, desc_dev, t.nsub, start, endf, iv_bad, iv_hi);
  hipLaunchKernelGGL(k_jpg_fix, dim3((unsigned)t.niv), dim3(64), 0, s, desc_dev, sub_iv, iv_start, iv_end, iv_img, iv_fsub, cbase, comp,
                     huff, iv_nsub, iv_bad, iv_hi, start, endf, cntf);
  MM_LAUNCH_CHECK();
  if ((rc = mm_exclusive_scan_i32(cntf, bscan, t.nsub + 1, nullptr, sws, sws_bytes, s, 1)) != MM_OK) return rc;
  hipLaunchKernelGGL(k_jpg_final, gsub, dim3(T), 0, s, desc_dev, sub_iv, iv_start, iv_end, iv_img, iv_fsub, cbase, comp, huff, t.nsub, start,
                     bscan, coef, iv_done, status);
  hipLaunchKernelGGL(k_jpg_status, dim3((unsigned)mm_cdiv(t.niv, T)), dim3(T), 0, s, iv_img, iv_done, (int)t.niv, status);

  // 3-5. DC prediction, IDCT, upsampling + colour
  hipLaunchKernelGGL(k_jpg_dc, dim3(3, B), dim3(DC_T), 0, s, desc_dev, coef);
  hipLaunchKernelGGL(k_jpg_idct, dim3((unsigned)mm_cdiv(t.max_blk, T), B), dim3(T), 0, s, desc_dev, qt, coef, planes);
  hipLaunchKernelGGL(k_jpg_color, dim3((unsigned)mm_cdiv(t.max_pix, T), B), dim3(T), 0, s, desc_dev, planes, out);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"
