/* mm2d3d.h - C ABI of libmm2d3d_hip.so: the MI355X (gfx950) hot path of CVLAB-Unibo/MM2D3D.
 *
 * The reference has no FFI of its own: its 3D arithmetic is reached through the Python module
 * `sparseconvnet` (un-vendored dependency, /root/reference/environment.yml:37) and its 2D arithmetic through
 * torch.nn.  This header declares the entry points a binding for that path uses; each cites the reference
 * call site it replaces (EXP = /root/reference/experiments_USA_SING/rgbd_rgbxyz_sigmoid_for_rgb).
 * INTEGRATION.md shows the ctypes stub (mm2d3d_amd/_lib.py is the shipped one).
 *
 * Conventions
 *   - every pointer named *_dev or documented "device" is a HIP device pointer; *_host is host memory;
 *   - feature matrices are row-major fp32 with an explicit row stride `ld_*` in floats;
 *   - the library never allocates device memory: outputs and workspaces are supplied by the caller
 *     (size queries: mm_*_ws_bytes); all work is enqueued on `stream` and returns immediately;
 *   - no process-wide mutable state: what outlives a call (grid-barrier words, fault word, mode switches of the
 *     single-launch batch norms) lives in a per-device HANDLE (mm_create) over memory the caller supplied; entry points
 *     that use it take the handle first; modes of the stateless engines travel as explicit arguments; no entry point
 *     reads an environment variable (the Python layer reads them once and passes them on).  One host thread per handle
 *     at a time.  [The only process-wide memory are per-device "done" bits of idempotent hipFuncSetAttribute calls.]
 *   - return value 0 = ok, negative = error (MM_ERR_*), message via mm_last_error() (thread-local);
 *   - integer results (ids, rulebooks) are deterministic and follow the canonical orders of SURVEY.md A.8;
 *     floating-point reductions run in a fixed order (no float atomics): results are bit-stable run to run.
 */
#ifndef MM2D3D_H
#define MM2D3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mm_stream_t; /* hipStream_t */

#define MM_OK 0
#define MM_ERR_ARG (-1)
#define MM_ERR_HIP (-2)
#define MM_ERR_WORKSPACE (-3)
#define MM_ERR_UNSUPPORTED (-4)

const char* mm_last_error(void);

/* ---------------------------------------------------------------- per-device handle (csrc/handle.hip)
 * The reference keeps the equivalent state inside torch / cuDNN / SparseConvNet handles; this ABI exposes it. */
typedef void* mm_handle_t;
size_t mm_handle_sync_bytes(void);  /* device memory, zero-filled by the caller: 64 barrier slots of 2 KB (one per stream) */
size_t mm_handle_fault_bytes(void); /* pinned, device-mapped host memory (hipHostMalloc / torch pinned), zero-filled */
int mm_create(int device_id, void* sync_dev, size_t sync_bytes, void* fault_host, size_t fault_bytes, mm_handle_t* out);
int mm_destroy(mm_handle_t h);
#define MM_OPT_BN2D_FUSED 0   /* single-launch BatchNorm2d kernels: bit 0 = forward, bit 1 = backward; default 3 */
#define MM_OPT_BN3D_FUSED 1   /* the same for the sparse rows (mm_bn_*); default 3 */
#define MM_OPT_OS_SORT 2      /* reserved (the tile-table sort is an argument of mm_os_table_build) */
#define MM_OPT_SPCONV_TERMS 3 /* reserved (the sparse engines take their mode as an argument, MM_SPCONV_*) */
#define MM_OPT_DW_WIDE 4      /* reserved */
/* returns the previous value (>= 0) or MM_ERR_ARG.  The single-launch batch-norm kernels need every CU at once: use 0 when
 * several PROCESSES share one GPU, and clear the bit of a direction whose launches overlap kernels of another stream that
 * spin-wait across their own workgroups (collectives, look-back scans; csrc/fused_bn.h). */
int mm_set_option(mm_handle_t h, int option, int value);
int mm_get_option(mm_handle_t h, int option);
/* 1 if a single-launch batch-norm kernel launched through h gave up at its grid barrier since the last call (its grid was not
 * co-resident).  That launch's outputs are invalid; the handle's single-launch kernels are switched off (three-kernel path) and
 * its barrier words re-armed.  A host-memory read when nothing happened. */
int mm_fault_poll(mm_handle_t h);

/* ---------------------------------------------------------------- active sets and rulebooks (csrc/meta.hip)
 * Replaces the host hash-map work of scn.InputLayer(3, full_scale, mode=4) (EXP/3d_net/scn_unet.py:113,121)
 * and the rulebook construction of scn.SubmanifoldConvolution / Convolution / Deconvolution
 * (scn_unet.py:43,45,52,114 / :68-70 / :75-77). */

/* power-of-two capacity >= 2*n_items for the open-addressing table */
int64_t mm_hash_capacity(int64_t n_items);
size_t mm_dedupe_ws_bytes(int64_t n_bound);

/* Dedupe items into active sites, ids in order of first occurrence.
 *   coords        device [n,4] (x,y,z,batch), int64 when coords_is_i64 else int32; 0 <= value < 65536
 *   n_bound       rows allocated; n_dev (device int32, may be NULL) = actual row count <= n_bound
 *   shift         x,y,z >> shift before keying (0: InputLayer; 1: parents of a stride-2 Convolution)
 *   tkeys/tvals   device table [cap] (uint64 / int32), cap = mm_hash_capacity(n_bound); afterwards key -> site id
 *   item2vox      device [n]   site id of every item
 *   vox_coords    device [n,4] int32 coords of the sites (first n_active rows)
 *   csr_off/items device [n+1]/[n]  site -> its items, ascending
 *   n_active_dev  device int32 [1];  err_dev device int32 [1] set non-zero on out-of-range coordinates */
int mm_voxel_dedupe(const void* coords, int coords_is_i64, int64_t n_bound, const int32_t* n_dev, int shift,
                    uint64_t* tkeys, int32_t* tvals, int64_t cap, int32_t* item2vox, int32_t* vox_coords,
                    int32_t* csr_off, int32_t* csr_items, int32_t* n_active_dev, int32_t* err_dev, int no_spin, void* ws,
                    size_t ws_bytes, mm_stream_t stream);
/* no_spin != 0 (here and below): only kernels whose workgroups never wait for each other (plain three-launch prefix sums
 * instead of the decoupled look-back scan) - what a build on a side stream beside grid-barrier kernels needs. */

/* nbr[k*n + o] = id of the active site at coord(o) + offset(k), k = ((dx+1)*3 + (dy+1))*3 + (dz+1), or -1 */
/* out[0] = number of active rows with batch index < split.  Rows are in first-occurrence order of a batch-sorted point
 * list (collate_scn_base, lib/dataset/__init__.py:63-67), so those are rows 0 .. out[0]-1: the statistics-group boundary
 * of the batch-norm layers when source and target scenes share one pass. */
int mm_batch_lower_bound(const int32_t* vox_coords, const int32_t* n_dev, int32_t split, int32_t* out, mm_stream_t stream);
int mm_subm_neighbors(const int32_t* vox_coords, int64_t n, int32_t spatial_size, const uint64_t* tkeys,
                      const int32_t* tvals, int64_t cap, int32_t* nbr, mm_stream_t stream);

/* nbr[k*n_coarse + parent] = child with offset k = ((x&1)*2 + (y&1))*2 + (z&1), or -1 */
int mm_down_neighbors(const int32_t* vox_coords_fine, int64_t n_fine, const int32_t* fine2coarse, int64_t n_coarse,
                      int32_t* nbr, mm_stream_t stream);

size_t mm_rulebook_ws_bytes(int64_t n_out, int K);
/* neighbour table -> k-major rule lists rin/rout (capacity K*n_out, pairs sorted by out id inside a bucket),
 * offsets[K+1] (device), CSR over out rows: csr_off[n_out+1], csr_pos[R] = rule positions in ascending k.
 * csr_off = csr_pos = NULL skips the CSR (levels served by the output-stationary engine never read it);
 * mm_rulebook_csr builds it later from the same table (same workspace size). */
int mm_rulebook_compact(const int32_t* nbr, int K, int64_t n_out, int32_t* rin, int32_t* rout, int32_t* offsets,
                        int32_t* csr_off, int32_t* csr_pos, int no_spin, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_rulebook_csr(const int32_t* nbr, int K, int64_t n_out, int32_t* csr_off, int32_t* csr_pos, int no_spin, void* ws,
                    size_t ws_bytes, mm_stream_t stream);

/* ---- every level in one launch per stage (same results as the per-level entry points above, bit for bit)
 * The whole dedupe chain points -> level 0 -> ... -> level nlev-1 without waiting for a level's size: the sites of level l are
 * the distinct (x >> l, y >> l, z >> l, batch) of the points, ranked by their smallest point index, which is the order of first
 * occurrence among the rows of level l-1.  At most 12 launches.
 *   coords        device int64 [n_pts,4]
 *   tkeys/tvals   [nlev][cap], cap = mm_hash_capacity(n_pts); afterwards key -> site id, per level
 *   item2vox      [nlev][max(n_pts,1)]    row l: items of level l (points for l = 0, rows of level l-1 otherwise) -> site id
 *   vox_coords    [nlev][max(n_pts,1)][4]
 *   csr_off/items [nlev][n_pts+1] / [nlev][max(n_pts,1)]
 *   split         >= 0: counts[nlev+1+l] = rows of level l with batch index < split (mm_batch_lower_bound); < 0: left 0
 *   counts        device int32 [2*nlev+1], written here: sites per level, then the error word (1 coordinate out of range, 2 table
 *                 full), then the split rows */
size_t mm_dedupe_levels_ws_bytes(int64_t n_pts, int nlev);
int mm_voxel_dedupe_levels(const int64_t* coords, int64_t n_pts, int nlev, uint64_t* tkeys, int32_t* tvals, int64_t cap,
                           int32_t* item2vox, int32_t* vox_coords, int32_t* csr_off, int32_t* csr_items, int32_t split,
                           int32_t* counts, int no_spin, void* ws, size_t ws_bytes, mm_stream_t stream);
/* Neighbour tables of several levels: mm_subm_neighbors (K = 27: vox_coords, n, spatial_size and the table of one level) and
 * mm_down_neighbors (K = 8: vox_coords and n of the fine level, fine2coarse, n_coarse) in three launches for all of them.
 * Host array of at most MM_META_BATCH entries. */
#define MM_META_BATCH 32
typedef struct mm_nbr_desc {
  const int32_t* vox_coords; const uint64_t* tkeys; const int32_t* tvals; const int32_t* fine2coarse; int32_t* nbr;
  int64_t n, n_coarse, cap; int32_t spatial_size, K;
} mm_nbr_desc;
int mm_neighbors_batch(const mm_nbr_desc* d, int nd, mm_stream_t stream);
/* mm_rulebook_compact of several neighbour tables that lie back to back in one array nbr (table j: K * n_out words from word
 * start; start of table 0 is 0): the rule lists of table j begin at word start of rin / rout, its K + 1 bucket offsets at word offs
 * of offsets.  row0 >= 0: also its CSR, n_out + 1 words from word row0 of csr_off (back to back in table order, from 0) and K * n_out
 * words from word pos0 of csr_pos.  ws: mm_rulebook_batch_ws_bytes(words of nbr, words of csr_off). */
typedef struct mm_rulebook_desc {
  int64_t start, n_out, row0, pos0; int32_t K, offs;
} mm_rulebook_desc;
size_t mm_rulebook_batch_ws_bytes(int64_t nbr_words, int64_t csr_rows);
int mm_rulebook_compact_batch(const int32_t* nbr, const mm_rulebook_desc* d, int nd, int32_t* rin, int32_t* rout, int32_t* offsets,
                              int32_t* csr_off, int32_t* csr_pos, int no_spin, void* ws, size_t ws_bytes, mm_stream_t stream);

/* ---------------------------------------------------------------- GPU-side sample preparation (csrc/dataprep.hip)
 * The loader-side numpy code of the reference for a whole batch of scenes, bit-exact with it:
 * augment_and_scale_3d + int cast + range mask (lib/utils/augmentation_3d.py:83-158, nuscenes_dataloader.py:323-332),
 * pixel indices / last-write-wins depth and 2D label maps / fliplr / RGB point features (nuscenes_dataloader.py:262-283,
 * 291-297,361-364), collate with the batch index as last coordinate column (lib/dataset/__init__.py:63-68,91-96).
 * The random draws (rotation matrix, translation fractions, flips) are made on the host in the reference's order. */
size_t mm_voxelize_ws_bytes(int64_t n_total, int B);
/* points [n_total][3] fp32 (scene b = rows scene_off[b]..scene_off[b+1]); rot [B][9] fp32; u [B][3] fp64 (rand(3) draws)
 * -> locs int64 [kept][4] (x,y,z,scene), keep int32 [kept] (original rows, order preserved), counts int32 [B+1] (per scene,
 * total), min_value fp32 [B][3], offset fp64 [B][3] */
int mm_voxelize_batch(const float* points, const int32_t* scene_off_dev, const int32_t* scene_off_host, int B, const float* rot,
                      const double* u, int transl, float scale, int full_scale, int64_t* locs, int32_t* keep, int32_t* counts,
                      float* min_value, double* offset, void* ws, size_t ws_bytes, mm_stream_t stream);
/* the same for fp64 points (VirtualKITTI with camera_coords: the reference's points are float64 there): the arithmetic of
 * numpy on float64 arrays (rot fp32, widened exactly; points.rot, * scale, min, translation and + offset in fp64);
 * scale and min_value fp64; workspace of mm_voxelize_ws_bytes_f64 */
size_t mm_voxelize_ws_bytes_f64(int64_t n_total, int B);
int mm_voxelize_batch_f64(const double* points, const int32_t* scene_off_dev, const int32_t* scene_off_host, int B, const float* rot,
                          const double* u, int transl, double scale, int full_scale, int64_t* locs, int32_t* keep, int32_t* counts,
                          double* min_value, double* offset, void* ws, size_t ws_bytes, mm_stream_t stream);
/* points_img [n_total][2] fp32 (row, col), depth_vals [n_total] -> img_indices int64 [n_total][2], depth fp32 [B][H][W],
 * seg2d fp64 [B][H][W] (optional, needs labels); flip [B] bytes (optional); winner int32 [B*H*W] scratch; err: 1 = outside */
int mm_project_batch(const float* points_img, const float* depth_vals, const int64_t* labels, const int32_t* scene_off_dev,
                     const int32_t* scene_off_host, int B, int H, int W, const uint8_t* flip, int64_t* img_indices, float* depth,
                     double* seg2d, int32_t* winner, int32_t* err, mm_stream_t stream);
/* per-point arrays of the kept rows; feats[p][c] = image[scene(p)][c][row][col] (image fp32 [B][C][H][W]) */
int mm_collect_points(const int32_t* keep, const int32_t* n_keep_dev, int64_t n_bound, const int64_t* locs, const int64_t* img_indices,
                      const int64_t* labels, const float* image, int C, int H, int W, const float* points, int64_t* img_indices_out,
                      int64_t* labels_out, float* feats_out, float* points_out, mm_stream_t stream);
/* the same with fp64 points and points_out (the kept rows of mm_voxelize_batch_f64) */
int mm_collect_points_f64(const int32_t* keep, const int32_t* n_keep_dev, int64_t n_bound, const int64_t* locs, const int64_t* img_indices,
                          const int64_t* labels, const float* image, int C, int H, int W, const double* points, int64_t* img_indices_out,
                          int64_t* labels_out, float* feats_out, double* points_out, mm_stream_t stream);
/* device-count forms, for a caller that must not wait for the stream (mm2d3d_amd/pipeline.py): the launch covers n_total = the
 * batch's point count, the size every output is allocated at; the kept total is read on the device from counts[B] (counts =
 * the [B+1] words of mm_voxelize_batch) and rows at or beyond it are left untouched.  extra_in / extra_out: n_extra (<= 3) host
 * arrays of device pointers to per-point arrays of extra_bytes-wide elements (1, 2, 4 or 8: the pseudo labels), gathered in
 * the same launch: extra_out[j][p] = extra_in[j][keep[p]] */
int mm_collect_points_dev(const int32_t* keep, const int32_t* counts_dev, int B, int64_t n_total, const int64_t* locs,
                          const int64_t* img_indices, const int64_t* labels, const float* image, int C, int H, int W, const float* points,
                          int64_t* img_indices_out, int64_t* labels_out, float* feats_out, float* points_out,
                          const void* const* extra_in, void* const* extra_out, int n_extra, int extra_bytes, mm_stream_t stream);
int mm_collect_points_f64_dev(const int32_t* keep, const int32_t* counts_dev, int B, int64_t n_total, const int64_t* locs,
                              const int64_t* img_indices, const int64_t* labels, const float* image, int C, int H, int W,
                              const double* points, int64_t* img_indices_out, int64_t* labels_out, float* feats_out, double* points_out,
                              const void* const* extra_in, void* const* extra_out, int n_extra, int extra_bytes, mm_stream_t stream);

/* ---------------------------------------------------------------- camera-image preparation (csrc/imageprep.hip)
 * The image half of the loaders' per-sample code for a whole batch, bit-exact with PIL + numpy: the crop and the
 * Image.resize(size, BILINEAR) of the front ends (semantic_kitti.py:321-392, a2d2.py:268-276, nuscenes_dataloader.py:257-262),
 * the ColorJitter of the PIL image (nuscenes_dataloader.py:286-287), float conversion, fliplr and normalisation.  Decoding and
 * every random draw stay on the host (mm2d3d_amd/imageprep.py builds the tables).
 *   src        device uint8, the decoded RGB images back to back ([H_i][W_i][3] each), src_bytes long
 *   desc       int64 [B][16] per scene, device copy and host copy (the host copy is checked against the buffer sizes):
 *              MM_IMG_SRC_OFF 0 byte offset of the window's first pixel in src   MM_IMG_SRC_PITCH 1 bytes per source row
 *              MM_IMG_WIN_W 2, MM_IMG_WIN_H 3 window size          MM_IMG_TMP_ROWS 4, MM_IMG_YBOX_FIRST 5 source rows of the
 *              horizontal pass                                     MM_IMG_KX 6, MM_IMG_KY 7 taps per output column / row
 *              MM_IMG_HCOEF 8, MM_IMG_VCOEF 9 int32 index into coef of bounds [W][2] (first tap, tap count) then Q22 weights
 *              [W][KX] (vertical: [H][2], [H][KY], first taps relative to YBOX_FIRST)   MM_IMG_TMP_OFF 10 byte offset into tmp
 *              MM_IMG_OPS 11 jitter operations in drawn order, 4 bits each (0 brightness, 1 contrast, 2 saturation, 3 hue)
 *              MM_IMG_NOPS 12 count, MM_IMG_NPRE 13 operations before contrast (= NOPS without contrast)
 *              MM_IMG_HUE 14 hue shift 0..255                      MM_IMG_FLIP 15 fliplr
 *   factors    device fp32 [B][4] jitter factors by operation; lut device fp32 [B][3][256] = normalise(u8 / 255.0)
 *   tmp        device uint8 scratch, tmp_bytes >= sum of TMP_ROWS * W * 3; mid device uint8 scratch [B][H][W][3];
 *   sums       device int64 [B] scratch (sums of L before contrast)
 * -> img fp32 [B][3][H][W], already flipped where FLIP is set.  Three launches. */
int mm_image_prepare(const uint8_t* src, int64_t src_bytes, const int64_t* desc_dev, const int64_t* desc_host, int B, int H, int W,
                     const int32_t* coef, int64_t coef_len, const float* factors, const float* lut, uint8_t* tmp, int64_t tmp_bytes,
                     uint8_t* mid, int64_t* sums, float* img, mm_stream_t stream);

/* ---------------------------------------------------------------- baseline-JPEG decode (csrc/jpeg.hip)
 * The camera JPEGs of a batch decoded on the GPU into the source buffer mm_image_prepare reads, bit-exact with Pillow's
 * libjpeg-turbo (np.asarray(Image.open(path))): jdhuff.c Huffman decode, DC prediction, jidctint.c jpeg_idct_islow,
 * jdsample.c fancy upsampling, jdcolor.c ycc_rgb_convert.  Eligible files only (mm2d3d_amd/jpeg.py parse): SOF0/SOF1, 8-bit,
 * Huffman, three YCbCr components in one interleaved scan, luma sampling 1x1 / 2x1 / 2x2 and chroma 1x1, any restart interval.
 *   data       device uint8, the files' bytes (headers included), data_bytes long (< 2^31)
 *   desc       int64 [B][32] per image, device copy and host copy (the host copy is checked against the buffer sizes):
 *              MM_JPG_SEG_OFF 0, MM_JPG_SEG_LEN 1 byte range of the entropy-coded segment in data (SOS end .. EOI)
 *              MM_JPG_W 2, MM_JPG_H 3 image size        MM_JPG_HS 4, MM_JPG_VS 5 luma sampling factors
 *              MM_JPG_MCUS_X 6, MM_JPG_MCUS_Y 7 MCUs per row / column        MM_JPG_RESTART 8 MCUs per restart interval (0: none)
 *              MM_JPG_N_IV 9 restart intervals, MM_JPG_IV0 10 the first one's index in the batch
 *              MM_JPG_SUB0 11, MM_JPG_SUB_CAP 12 decoding lanes (>= ceil(SEG_LEN * 8 / 2048) + N_IV)
 *              MM_JPG_BLK0 13 first block (8x8 coefficients) in the batch  MM_JPG_PLANE_OFF 14 byte offset of the component planes
 *              MM_JPG_OUT_OFF 15 byte offset of the [H][W][3] RGB image in out
 *              MM_JPG_QT0..2 16-18 quantisation table (qt row), MM_JPG_DC0..2 19-21, MM_JPG_AC0..2 22-24 Huffman table (huff
 *              row) of Y, Cb, Cr; words 25-31 reserved (0).  Images share no interval, lane, block, plane or data range.
 *   huff       device int32 [n_huff][1024]: fast[512] = length << 8 | symbol for codes of at most 9 bits, libjpeg's maxcode[18]
 *              and valoffset[18], huffval[256]       qt device int32 [n_qt][64], natural order
 *   out        device uint8, out_bytes long          status device int32 [B], written by the kernels:
 *              MM_JPG_ST_* bits, 0 = decoded; read it after the stream has run.  No kernel reads or writes outside the buffers.
 *   ws         device scratch of mm_jpeg_ws_bytes(B, data_bytes, total intervals, total lanes, total blocks, plane bytes)
 *              (totals = max over images of IV0 + N_IV, SUB0 + SUB_CAP, BLK0 + blocks, PLANE_OFF + plane bytes) */
#define MM_JPG_ST_MARKER 1     /* a marker other than RST0-7 inside the entropy-coded segment */
#define MM_JPG_ST_RESTART 2    /* restart markers missing, extra or out of sequence */
#define MM_JPG_ST_HUFFMAN 4    /* a bit pattern that is no code of the Huffman table */
#define MM_JPG_ST_INCOMPLETE 8 /* an interval's data ended before its blocks were complete */
size_t mm_jpeg_ws_bytes(int B, int64_t data_bytes, int64_t n_intervals, int64_t n_lanes, int64_t n_blocks, int64_t plane_bytes);
int mm_jpeg_decode(const uint8_t* data, int64_t data_bytes, const int64_t* desc_dev, const int64_t* desc_host, int B, const int32_t* huff,
                   int64_t n_huff, const int32_t* qt, int64_t n_qt, uint8_t* out, int64_t out_bytes, int32_t* status, void* ws,
                   size_t ws_bytes, mm_stream_t stream);

/* ---------------------------------------------------------------- sparse convolution engines (csrc/spconv.hip)
 * scn.SubmanifoldConvolution / Convolution / Deconvolution forward and backward. */
size_t mm_spconv_ws_bytes(int64_t n_rules, int Cin, int Cout, int K);
/* out[dst[r]] (+)= in[src[r]] . W[k(r)] over a k-major rulebook (offsets_host = host copy of offsets[K+1]).
 *   unique_dst != 0: every destination row has exactly one rule (direct writes);
 *   else destinations are reduced through csr_off/csr_pos in ascending k and rows without rules become 0.
 *   weight element (k,ci,co) = W[kk*w_kstride + ci*s_ci + co*s_co], kk = kflip ? K-1-k : k.
 *   mode (fp32 rows): MM_SPCONV_DEFAULT = fp32-faithful three-term split-bf16 products on the matrix-rate-bound widths;
 *   MM_SPCONV_FP32 = plain fp32 engines everywhere; MM_SPCONV_TWO_TERMS = two terms (faster; fails the gradient parity bar:
 *   diagnostics only); | MM_SPCONV_DW_NARROW: the weight gradient keeps its <= 4 x 4 channel tiles (same slabs, so the same
 *   sums bit for bit as with the default tiles). */
#define MM_SPCONV_DEFAULT 0
#define MM_SPCONV_FP32 1
#define MM_SPCONV_TWO_TERMS 2
#define MM_SPCONV_DW_NARROW 4
#define MM_SPCONV_DW16_ELEM 8 /* 16-bit rows: the weight gradient gathers single elements (the round-3 kernel) instead of whole rows
                              * through LDS and transpose reads (round 6, same slab sums): A/B measurements */
int mm_spconv_apply(const float* in, int ld_in, int Cin, float* out, int ld_out, int Cout, int64_t n_out,
                    const int32_t* src, const int32_t* dst, const int32_t* offsets_dev, const int32_t* offsets_host,
                    int K, const int32_t* csr_off, const int32_t* csr_pos, int unique_dst, const float* W,
                    int64_t w_kstride, int s_ci, int s_co, int kflip, int mode, void* ws, size_t ws_bytes, mm_stream_t stream);
/* The same with the weights' three-term bf16 fragments supplied by the caller (Wpk: written by mm_spconv_os_pack /
 * mm_spconv_os_pack_batch for the same K, Cin, Cout, strides and kflip; NULL = pack inside the call): a net packs every
 * layer once per optimiser step in one launch instead of once per layer call. */
int mm_spconv_apply_packed(const float* in, int ld_in, int Cin, float* out, int ld_out, int Cout, int64_t n_out,
                           const int32_t* src, const int32_t* dst, const int32_t* offsets_dev, const int32_t* offsets_host,
                           int K, const int32_t* csr_off, const int32_t* csr_pos, int unique_dst, const float* W,
                           int64_t w_kstride, int s_ci, int s_co, int kflip, const void* Wpk, int mode, void* ws, size_t ws_bytes,
                           mm_stream_t stream);
size_t mm_spconv_dw_ws_bytes(const int32_t* offsets_host, int K, int Cin, int Cout);
/* dW[k][ci][co] (+)= sum over rules r of bucket k: in[src[r]][ci] * dout[dst[r]][co] */
int mm_spconv_dw(const float* in, int ld_in, int Cin, const float* dout, int ld_do, int Cout, const int32_t* src,
                 const int32_t* dst, const int32_t* offsets_host, int K, float* dW, int accumulate, int mode, void* ws,
                 size_t ws_bytes, mm_stream_t stream);

/* ---------------------------------------------------------------- output-stationary engine (csrc/ostable.hip, csrc/osconv.hip)
 * The same three scn convolutions (scn_unet.py:43,45,52,68-70,75-77,114), forward and data gradient, without the
 * tmp[rule] round trip: destination rows are ordered by neighbour bitmask, a workgroup owns a tile of them and
 * accumulates the offsets k in ascending order in registers. */
/* nbr[8][n_fine] for Deconvolution / d(Convolution)/d(input): nbr[octant(i)][i] = parent of fine row i, else -1 */
int mm_up_neighbors(const int32_t* vox_coords_fine, int64_t n_fine, const int32_t* fine2coarse, int32_t* nbr,
                    mm_stream_t stream);
size_t mm_os_table_ws_bytes(int64_t n, int K);
/* nbr[K][n] -> dst[npad] (rows sorted by neighbour bitmask, -1 = padding), nbrp[K][npad], tmask[nt];
 * nt = ceil(n / tile_rows), npad = nt * tile_rows, tile_rows a multiple of 64 (the engine takes 64) */
/* sort_merge: 0 = rocPRIM Onesweep radix sort (default), 1 = merge sort (identical result; its workgroups do not wait for each
 * other, which makes the build safe on a stream that runs beside grid-barrier kernels, see MM_OPT_BN2D_FUSED) */
int mm_os_table_build(const int32_t* nbr, int K, int64_t n, int tile_rows, int sort_merge, int32_t* dst, int32_t* nbrp,
                      uint32_t* tmask, void* ws, size_t ws_bytes, mm_stream_t stream);
/* three-term bf16 MFMA fragments of a weight tensor: element (k,ci,co) = W[kk*w_kstride + ci*s_ci + co*s_co],
 * kk = kflip ? K-1-k : k */
size_t mm_spconv_os_pack_bytes(int K, int Cin, int Cout);
int64_t mm_spconv_os_pack_blocks(int K, int Cin, int Cout);
int mm_spconv_os_pack_desc_fields(void);
int mm_spconv_os_pack(const float* W, int64_t w_kstride, int s_ci, int s_co, int kflip, int K, int Cin, int Cout, void* Wf,
                      mm_stream_t stream);
/* descs_dev [n_desc][12] int64 (device) = {W, Wf, K, Cin, Cout, nq, ncb, w_kstride, s_ci, s_co, kflip, blk_end}: one launch
 * packs every weight of a net after an optimiser step */
int mm_spconv_os_pack_batch(const int64_t* descs_dev, int n_desc, int64_t total_blocks, mm_stream_t stream);
/* out[dst[j]] = sum over present k (ascending) of in[nbrp[k][j]] . W[k];  Cin, Cout multiples of 16, rows 16-B aligned */
int mm_spconv_os_apply(const float* in, int ld_in, int Cin, float* out, int ld_out, int Cout, const void* Wf, int K,
                       const int32_t* dst, const int32_t* nbrp, const uint32_t* tmask, int64_t n_tiles, int tile_rows,
                       mm_stream_t stream);

/* 16-bit activation mode (BASELINE.json configs[4]): the sparse rows are bf16 (in and out), the
 * weights one bf16 term per element, accumulation fp32 in ascending k.  Same tables as above, tile_rows = 64. */
size_t mm_spconv_os_pack_bytes_bf16(int K, int Cin, int Cout);
int mm_spconv_os_pack_bf16(const float* W, int64_t w_kstride, int s_ci, int s_co, int kflip, int K, int Cin, int Cout, void* Wf,
                           mm_stream_t stream);
int mm_spconv_os_pack_batch_bf16(const int64_t* descs_dev, int n_desc, int64_t total_blocks, mm_stream_t stream);
int mm_spconv_os_apply_bf16(const void* in, int ld_in, int Cin, void* out, int ld_out, int Cout, const void* Wf, int K,
                            const int32_t* dst, const int32_t* nbrp, const uint32_t* tmask, int64_t n_tiles, int tile_rows,
                            mm_stream_t stream);
/* dW[k][ci][co] (+)= sum over the rules of bucket k of in[src][ci] * dout[dst][co]; in / dout bf16 rows, dW fp32;
 * workspace of mm_spconv_dw_ws_bytes.  Cin, Cout multiples of 16; unless mode has MM_SPCONV_DW16_ELEM the rows are read 16 bytes
 * at a time: in / dout 16-B aligned, ld_in / ld_do multiples of 8, else MM_ERR_ARG before any launch (_f16 and
 * mm_spconv_dw_partial with 16-bit rows alike).  Every row kind: ld_in >= Cin, ld_do >= Cout. */
int mm_spconv_dw_bf16(const void* in, int ld_in, int Cin, const void* dout, int ld_do, int Cout, const int32_t* src,
                      const int32_t* dst, const int32_t* offsets_host, int K, float* dW, int accumulate, int mode, void* ws,
                      size_t ws_bytes, mm_stream_t stream);
/* The fp16 kind of the 16-bit activation mode (BASELINE.json configs[4] "fp16 activations"; the reference trains with
 * ``precision: 16`` = fp16 autocast + GradScaler, train.yaml:11): the sparse rows are IEEE fp16, the weights one fp16 term per
 * element (fragment sizes: mm_spconv_os_pack_bytes_bf16), products on v_mfma_f32_16x16x32_f16, accumulation fp32 in
 * ascending k.  Gradient rows need loss scaling (mm2d3d_amd/amp.py). */
int mm_spconv_os_pack_f16(const float* W, int64_t w_kstride, int s_ci, int s_co, int kflip, int K, int Cin, int Cout, void* Wf,
                          mm_stream_t stream);
int mm_spconv_os_pack_batch_f16(const int64_t* descs_dev, int n_desc, int64_t total_blocks, mm_stream_t stream);
int mm_spconv_os_apply_f16(const void* in, int ld_in, int Cin, void* out, int ld_out, int Cout, const void* Wf, int K,
                           const int32_t* dst, const int32_t* nbrp, const uint32_t* tmask, int64_t n_tiles, int tile_rows,
                           mm_stream_t stream);
int mm_spconv_dw_f16(const void* in, int ld_in, int Cin, const void* dout, int ld_do, int Cout, const int32_t* src,
                     const int32_t* dst, const int32_t* offsets_host, int K, float* dW, int accumulate, int mode, void* ws,
                     size_t ws_bytes, mm_stream_t stream);
/* The weight gradient in two calls: mm_spconv_dw_partial writes the partial slabs of ONE layer (fp32 rows; bf16 rows when
 * bf16 == 1, IEEE fp16 rows when bf16 == 2) into ``partial`` (mm_spconv_dw_ws_bytes; must stay untouched until the reduce) and the 33 slab offsets of the
 * layer into ``blk_start_host``; mm_spconv_dw_reduce_batch sums the slabs of n layers in ONE launch.  descs_dev: n rows of
 * mm_spconv_dw_desc_bytes() bytes {const float* partial; float* dW; int32 ne = Cin*Cout, K, accumulate, blk_first;
 * int32 blk_start[33]}, blk_first = sum of mm_spconv_dw_reduce_blocks(ne, K) over the preceding rows, total_blocks = that sum over all rows.
 * Bit-identical to mm_spconv_dw (same slabs, same order).  Replaces the per-layer tail of scn's ConvolutionFunction /
 * SubmanifoldConvolutionFunction backward (reference call sites scn_unet.py:43-52,68-77,114). */
int mm_spconv_dw_partial(int bf16, const void* in, int ld_in, int Cin, const void* dout, int ld_do, int Cout, const int32_t* src,
                         const int32_t* dst, const int32_t* offsets_host, int K, int mode, void* partial, size_t partial_bytes,
                         int32_t* blk_start_host, mm_stream_t stream);
int mm_spconv_dw_desc_bytes(void);
int64_t mm_spconv_dw_reduce_blocks(int ne, int K);
int mm_spconv_dw_reduce_batch(const void* descs_dev, int n, int64_t total_blocks, mm_stream_t stream);

/* ---------------------------------------------------------------- batch norm + (leaky) ReLU (csrc/bn.hip)
 * scn.BatchNormReLU / BatchNormLeakyReLU (scn_unet.py:42,44,51,66,73,116); momentum = keep fraction (0.9). */
/* Row sets that fit on chip take single-launch training kernels (one workgroup per CU, rows kept on chip across two grid
 * barriers) when the handle allows it: mm_set_option(h, MM_OPT_BN3D_FUSED, mask), bit 0 = forward, bit 1 = backward. */
size_t mm_bn_ws_bytes(int C);
/* Which path a call takes: R, the rows per thread (1..36), when mm_bn_fwd_train (backward = 0) or mm_bn_bwd (backward != 0) over
 * N fp32 rows of C channels in 16-byte pieces (C, every pitch and every pointer a multiple of 4 floats) would take the
 * single-launch kernel through this handle now; 0 when it would run reduce / finalize / apply.  The same decision code as the
 * launch (option bits, device probe, C limits, grid shape); it registers no stream and touches neither the handle nor the
 * device.  Two things it cannot see: a handle whose 64 stream slots are all taken sends further streams to the three-kernel
 * path, and the 2 GiB limit on N * pitch * 4 is evaluated for contiguous rows (pitch = C).  MM_ERR_ARG for what is no handle. */
int mm_bn_fused_rows(mm_handle_t h, int64_t N, int64_t Ns, int C, int backward);
/* Arguments, all nine entry points: C in [1, 1024] and at most 256 threads wide (C <= 256, or C % 4 == 0 with 16-byte aligned
 * pointers and pitches), every pitch >= C, N >= 0, ws_bytes >= mm_bn_ws_bytes(C), running_mean and running_var both null or both
 * given (eval: both given), x / y / dy / dx / save_mean / save_invstd not null; weight, bias, dweight, dbias may each be null
 * (weight 1, bias 0, gradient not wanted).  A refused call (MM_ERR_ARG, MM_ERR_WORKSPACE) has launched and written nothing.
 * N == 0: the forward calls return MM_OK and write nothing (the running buffers stay as they are); the backward zeroes a
 * non-null dweight / dbias when accumulate == 0 and writes nothing otherwise.
 * A statistics group of ONE row: mean = x, variance 0, save_invstd = 1 / sqrt(eps), and no unbiased correction exists
 * (Ng / (Ng - 1) with Ng = 1), so the biased value is used: running_var = momentum * running_var + (1 - momentum) * 0.
 * Results are bit-stable: repeating a call on the same operands through the same handle gives the same bits. */
/* Ns: rows [0,Ns) and [Ns,N) (the active sites of the source and of the target scenes of a jointly batched step;
 * train.py:186-292 calls the net once per domain) are normalised with their OWN batch statistics and the running
 * buffers are updated group 0 first, then group 1.  Ns = N (or 0): single batch.  save_mean/save_invstd: [G][C]. */
int mm_bn_fwd_train(mm_handle_t h, const float* x, int ld_x, int64_t N, int64_t Ns, int C, const float* weight, const float* bias,
                    float* running_mean, float* running_var, float eps, float momentum, float leak, float* y, int ld_y,
                    float* save_mean, float* save_invstd, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_bn_fwd_eval(const float* x, int ld_x, int64_t N, int C, const float* weight, const float* bias,
                   const float* running_mean, const float* running_var, float eps, float leak, float* y, int ld_y,
                   mm_stream_t stream);
int mm_bn_bwd(mm_handle_t h, const float* x, int ld_x, const float* dy, int ld_dy, int64_t N, int64_t Ns, int C, const float* weight,
              const float* bias, const float* save_mean, const float* save_invstd, float leak, float* dx, int ld_dx,
              float* dweight, float* dbias, int accumulate, void* ws, size_t ws_bytes, mm_stream_t stream);
/* the same three entry points over bf16 rows (16-bit activation mode): x / y / dy / dx bf16 [N, C] (ld in elements),
 * statistics and parameters fp32 */
int mm_bn_fwd_train_bf16(mm_handle_t h, const void* x, int ld_x, int64_t N, int64_t Ns, int C, const float* weight, const float* bias,
                         float* running_mean, float* running_var, float eps, float momentum, float leak, void* y, int ld_y,
                         float* save_mean, float* save_invstd, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_bn_fwd_eval_bf16(const void* x, int ld_x, int64_t N, int C, const float* weight, const float* bias,
                        const float* running_mean, const float* running_var, float eps, float leak, void* y, int ld_y,
                        mm_stream_t stream);
int mm_bn_bwd_bf16(mm_handle_t h, const void* x, int ld_x, const void* dy, int ld_dy, int64_t N, int64_t Ns, int C, const float* weight,
                   const float* bias, const float* save_mean, const float* save_invstd, float leak, void* dx, int ld_dx,
                   float* dweight, float* dbias, int accumulate, void* ws, size_t ws_bytes, mm_stream_t stream);
/* ... and over IEEE fp16 rows (the fp16 kind of the 16-bit activation mode: train.yaml:11 ``precision: 16``) */
int mm_bn_fwd_train_f16(mm_handle_t h, const void* x, int ld_x, int64_t N, int64_t Ns, int C, const float* weight, const float* bias,
                        float* running_mean, float* running_var, float eps, float momentum, float leak, void* y, int ld_y,
                        float* save_mean, float* save_invstd, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_bn_fwd_eval_f16(const void* x, int ld_x, int64_t N, int C, const float* weight, const float* bias,
                       const float* running_mean, const float* running_var, float eps, float leak, void* y, int ld_y,
                       mm_stream_t stream);
int mm_bn_bwd_f16(mm_handle_t h, const void* x, int ld_x, const void* dy, int ld_dy, int64_t N, int64_t Ns, int C, const float* weight,
                  const float* bias, const float* save_mean, const float* save_invstd, float leak, void* dx, int ld_dx,
                  float* dweight, float* dbias, int accumulate, void* ws, size_t ws_bytes, mm_stream_t stream);

/* ---------------------------------------------------------------- per-point rows (csrc/point.hip) */
size_t mm_point_ws_bytes(int Cin, int Cout);
/* y = x * sigmoid(x.w + b), mask = sigmoid(...)   (EXP/3d_net/model.py:46-48) */
int mm_gate_fwd(const float* x, int64_t N, int C, const float* w, const float* b, float* y, float* mask,
                mm_stream_t stream);
int mm_gate_bwd(const float* x, const float* mask, const float* dy, int64_t N, int C, const float* w, float* dx,
                float* dw, float* db, int accumulate, void* ws, size_t ws_bytes, mm_stream_t stream);
/* site rows = mean (or sum) of their items' rows: InputLayer mode 4 / 3 forward, OutputLayer backward */
int mm_segment_reduce(const float* feats, int ld_f, int C, const int32_t* csr_off, const int32_t* csr_items,
                      int64_t n_vox, int mean, float* out, int ld_o, mm_stream_t stream);
/* item rows = their site's row (optionally / count): OutputLayer forward (scn_unet.py:117), InputLayer backward */
int mm_row_gather(const float* vox, int ld_v, int C, const int32_t* p2v, const int32_t* csr_off, int div_count,
                  int64_t N, float* out, int ld_o, mm_stream_t stream);
/* y = x W^T + b with torch nn.Linear layout W [Cout, Cin]  (EXP/3d_net/model.py:50,85) */
int mm_linear_fwd(const float* x, int ld_x, int64_t N, int Cin, int Cout, const float* w, const float* b, float* y,
                  int ld_y, mm_stream_t stream);
int mm_linear_bwd(const float* x, int ld_x, const float* dy, int ld_dy, int64_t N, int Cin, int Cout, const float* w,
                  float* dx, int ld_dx, int accumulate_dx, float* dw, float* db, int accumulate_w, void* ws,
                  size_t ws_bytes, mm_stream_t stream);

/* ---------------------------------------------------------------- losses, lifting, evaluation (csrc/loss.hip) */
size_t mm_loss_ws_bytes(void);
/* weighted cross entropy, ignore_index, weighted-mean reduction (lib/losses.py:55-68 -> F.cross_entropy).
 * stats[0] = loss, stats[1] = sum of the class weights of the counted rows.  This is mm_ce2_* below with P = N (the tail
 * unlabelled, zero_if_empty = 0), bit for bit: loss, weight sum and gradient. */
int mm_ce_fwd(const float* logits, int ld, const int64_t* labels, const float* weight, int64_t N, int C,
              int64_t ignore_index, float* stats, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_ce_bwd(const float* logits, int ld, const int64_t* labels, const float* weight, int64_t N, int C,
              int64_t ignore_index, const float* stats, const float* grad_out, float* dlogits, int ld_d,
              mm_stream_t stream);
/* Two cross entropies over ONE logits tensor: rows [0, P) against (labels0, weight0), rows [P, N) against (labels1 [N - P],
 * weight1), each a weighted mean over its own counted rows (the joined [source | target] pass: supervised loss on the source
 * rows, pseudo-label loss on the target rows).  A NULL labels pointer = an unlabelled segment: loss 0, sum_w 0, zero gradient
 * rows.  zero_if_empty bit s: segment s reports loss 0 instead of 0/0 when its counted weights sum to 0.  P == 0 and P == N are
 * legal.  stats[4] = loss0, sum_w0, loss1, sum_w1.  The backward writes every one of the N rows exactly once; a row of segment s
 * gets grad_out[s] * w[y] / sum_w_s * (softmax - onehot).  No atomics: bit-stable run to run. */
size_t mm_ce2_ws_bytes(void);
int mm_ce2_fwd(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
               const int64_t* labels1, const float* weight1, int64_t ignore_index, int zero_if_empty, float* stats,
               void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_ce2_bwd(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
               const int64_t* labels1, const float* weight1, int64_t ignore_index, const float* stats,
               const float* grad_out, float* dlogits, int ld_d, mm_stream_t stream);
/* The same pair with a weight per TAIL row: row_w [N - P] fp32 on the device (mm_pl_agree's weights; any finite values >= 0).
 *   loss1 = (1 / sum_w1) * sum over the counted tail rows of row_w_i * weight1[y_i] * ce_i;
 *   gradient row of a counted tail row: grad_out[1] * row_w_i * weight1[y_i] / sum_w1 * (softmax - onehot).
 * sum_w1 (stats[3]) is what mm_ce2_fwd reports, the class weights of the counted rows: the row weights are NOT in the denominator,
 * so a batch of uniformly uncertain rows pulls less instead of being renormalised.  A row with row_w == 0 is still counted and
 * still written (a zero gradient row).  The head segment, stats[], zero_if_empty and the every-row-written-once rule are those of
 * mm_ce2_*.  row_w == NULL launches mm_ce2_*'s kernels: the same bits; row_w all 1.0f gives the same bits too (x * 1.0f is exact).
 * The weights are constants of the gradient.  One kernel family: the row weight is a compile-time flag of k_ce_fwd / k_ce_bwd. */
int mm_ce2_fwd_w(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                 const int64_t* labels1, const float* weight1, int64_t ignore_index, int zero_if_empty, const float* row_w,
                 float* stats, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_ce2_bwd_w(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                 const int64_t* labels1, const float* weight1, int64_t ignore_index, const float* row_w, const float* stats,
                 const float* grad_out, float* dlogits, int ld_d, mm_stream_t stream);
/* Two-segment cross entropy with a SOFT tail (mean-teacher targets).  Rows [0, P) of logits [N, C] are the head of mm_ce2_*:
 * int64 labels0, optional class weights, ignore_index, labels outside [0, C) skipped, weighted mean (0/0 = nan when nothing is
 * counted); labels0 == NULL = an unlabelled head, loss 0 and zero gradient rows.  Rows [P, N) are compared with the teacher
 * logits ta [N - P, C] (row pitch ld_a) and, if tb != NULL, tb [N - P, C] (row pitch ld_b):
 *   target      q = softmax(ta / T), or with tb the ensemble q = 0.5 * (softmax(ta / T) + softmax(tb / T));
 *   confidence  always at T = 1: max_c softmax(ta)_c, or with tb max_c 0.5 * (softmax(ta) + softmax(tb))_c - the float32 values
 *               pa / pe of the device function behind mm_pselab_predict and mm_teacher_labels, bit for bit;
 *   kept        a row is kept iff confidence >= thr in float32 (thr in [0, 1]; 0 = the caller gave no threshold), so a teacher
 *               row with non-finite logits (a NaN confidence, or the ensemble's -1) is never kept;
 *   loss        (1 / K) * sum over the K kept rows of sum_c q_c * (logsumexp(x) - x_c); K == 0 gives loss 0 and a zero gradient.
 *               There is NO T^2 factor: a caller who wants the gradient scale of the distillation literature multiplies by T^2.
 * stats[4] = head loss, head weight sum, tail loss, K as a float (read by the backward); kept (may be NULL) receives K as an exact
 * int64.  The backward writes every one of the N rows exactly once: head rows as mm_ce2_bwd with grad_out[0], kept tail rows
 * grad_out[1] / K * (softmax(x) - q) with q recomputed from the teacher logits (no [N, C] buffer is saved), all other rows zeros.
 * ta may be NULL only when P == N.  C <= 32.  No atomics; fp64 partial sums combined in a fixed order: bit-stable run to run. */
size_t mm_ce2s_ws_bytes(void);
int mm_ce2s_fwd(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                int64_t ignore_index, const float* ta, int ld_a, const float* tb, int ld_b, float temperature, float thr,
                float* stats, int64_t* kept, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_ce2s_bwd(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                int64_t ignore_index, const float* ta, int ld_a, const float* tb, int ld_b, float temperature, float thr,
                const float* stats, const float* grad_out, float* dlogits, int ld_d, mm_stream_t stream);
/* The same pair with one threshold per class, thr_cls[C] fp32 on the device, in place of the scalar: a tail row is kept iff its
 * confidence >= thr_cls[y] in float32, y the arg-max the confidence belongs to (of softmax(ta), or with tb of the ensemble; the
 * first maximum wins).  A NaN threshold keeps nothing of its class.  Everything else, the return codes included, is as above; the
 * scalar entry points run the same kernels and keep their results bit for bit. */
int mm_ce2s_fwd_cls(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                    int64_t ignore_index, const float* ta, int ld_a, const float* tb, int ld_b, float temperature,
                    const float* thr_cls, float* stats, int64_t* kept, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_ce2s_bwd_cls(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                    int64_t ignore_index, const float* ta, int ld_a, const float* tb, int ld_b, float temperature,
                    const float* thr_cls, const float* stats, const float* grad_out, float* dlogits, int ld_d, mm_stream_t stream);
/* The soft pair with a weight per TAIL row, row_w [N - P] fp32 on the device, and both kinds of threshold in one entry point: a
 * non-NULL thr_cls [C] wins (the rule of mm_ce2s_*_cls), else the scalar thr (the rule of mm_ce2s_*).
 *   loss = (1 / K) * sum over the K kept rows of row_w_i * sum_c q_c * (logsumexp(x) - x_c);
 *   gradient row of a kept row: grad_out[1] * row_w_i / K * (softmax(x) - q).
 * K (stats[3], kept) ignores row_w: thresholds decide which rows are kept, the weight scales the rows that remain; a kept row with
 * row_w == 0 is counted and written as a zero gradient row.  Everything else is as above.  row_w == NULL launches the kernels of
 * mm_ce2s_* / mm_ce2s_*_cls: the same bits; row_w all 1.0f gives the same bits too.  The weights are constants of the gradient. */
int mm_ce2s_fwd_w(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                  int64_t ignore_index, const float* ta, int ld_a, const float* tb, int ld_b, float temperature, float thr,
                  const float* thr_cls, const float* row_w, float* stats, int64_t* kept, void* ws, size_t ws_bytes,
                  mm_stream_t stream);
int mm_ce2s_bwd_w(const float* logits, int ld, int64_t N, int64_t P, int C, const int64_t* labels0, const float* weight0,
                  int64_t ignore_index, const float* ta, int ld_a, const float* tb, int ld_b, float temperature, float thr,
                  const float* thr_cls, const float* row_w, const float* stats, const float* grad_out, float* dlogits, int ld_d,
                  mm_stream_t stream);
/* Lovasz-softmax loss (Berman et al., CVPR 2018) of logits [N, C] (row pitch ld) against int64 labels (csrc/lovasz.hip).
 * Counted rows: label != ignore_index and 0 <= label < C, as in mm_ce2_*; p = softmax(x) per row.  For every class c:
 * fg_i = [y_i == c], e_i = |fg_i - p_ic|; the counted rows are ordered by e descending, stable in the row index.  With G = sum fg,
 * r_i the 1-based rank of row i and f_i the foreground rows among ranks 1 .. r_i: U = G + r_i - f_i, I = G - f_i, and the weight
 * of row i is the increment of the Jaccard loss 1 - I / U at its rank in closed form: g_i = 1 / U for a foreground row,
 * I / (U * (U - 1)) for a background row, and 1 for the rank-1 row of a class with G == 0.  loss_c = sum_i e_i * g_i; the loss
 * is the mean of loss_c over the included classes: those with G > 0, or with classes_all != 0 every class as soon as one row
 * is counted.  Nothing counted: loss 0, n_included 0, coef 0.
 *   err, coef   class-major [C][N], indexed by the original row; an uncounted row has err = -1 and coef = 0;
 *               coef[c][i] = dloss / dp_ic = (fg ? -1 : +1) * g_i / n_included (g is a constant of the gradient);
 *   stats[3]    the loss, n_included, the number of counted rows.
 * The backward recomputes the softmax: dlogits_ik = grad_out[0] * p_ik * (coef[k][i] - sum_c coef[c][i] * p_ic), every one of the
 * N rows written once (zeros where every coefficient of the row is zero); grad_out is read on the device.
 * 1 <= C <= 32, ld >= C, ld_d >= C, 0 <= N <= 2^24 (U <= N is then exact in float32, and N * C < 2^31); anything else is
 * refused before a launch.  The sort is a stable three-digit radix sort, every class in one grid; no workgroup waits for another
 * (no look-back, no spin, no grid barrier) and no float atomics: fp64 partial sums in a fixed order, bit-stable run to run.
 * mm_lovasz_ws_bytes returns 0 for a C or N outside these limits. */
size_t mm_lovasz_ws_bytes(int64_t N, int C);
int mm_lovasz_fwd(const float* logits, int ld, int64_t N, int C, const int64_t* labels, int64_t ignore_index, int classes_all,
                  float* err, float* coef, float* stats, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_lovasz_bwd(const float* logits, int ld, int64_t N, int C, const float* coef, const float* grad_out, float* dlogits,
                  int ld_d, mm_stream_t stream);
/* Target-domain entropy (MinEnt) and diversity (the batch-mean term of information maximisation) of rows [P, N) of logits [N, C]
 * (row pitch ld; csrc/infomax.hip).  Counted rows: the rows i of [P, N) whose C logits are all finite; n of them.  Per counted row
 * p_i = softmax(x_i), log p_ic = (x_ic - max_i) - logf(sum_i) in float32, H_i = -sum_c p_ic log p_ic.  Then, summed in fp64:
 *   ent     = sum_i H_i / (n ln C)                      the normalised entropy, in [0, 1];
 *   mass_c  = (1 / n) sum_i p_ic                        the batch-mean prediction;
 *   div     = sum_c mass_c (ln mass_c - ln pi_c) / ln C  = KL(mass || pi) / ln C >= 0; a class with mass_c == 0 contributes 0.
 * prior: pi, fp32 [C] on the device, positive and summing to 1 (the caller's duty); NULL = uniform.  n == 0: ent = div = 0,
 * mass = 0 and an all-zero gradient.  Outputs of the forward: stats[2] = ent, div; mass[C]; count[1] = n, exact; aux[C + 1] =
 * g_c = ln(mass_c / pi_c) (0 where mass_c == 0), then 1 / (n ln C) (0 when n == 0) - what the backward reads, so it needs no second
 * statistics pass.  The backward writes every one of the N rows exactly once, rows [0, P) and uncounted rows as +0, counted rows
 *   dlogits_ik = grad_out[0] * (-p_ik (log p_ik + H_i)) / (n ln C) + grad_out[1] * p_ik (g_k - sum_c p_ic g_c) / (n ln C);
 * grad_out[2], aux are read on the device: no host read anywhere.  2 <= C <= 32, ld >= C, ld_d >= C, 0 <= P <= N, N * C < 2^31;
 * anything else is refused before a launch.  N == 0 and P == N are legal (the forward then runs its one-workgroup finalise alone).
 * Two launches forward (fp64 column sums and integer row counts per workgroup of a capped grid, then one workgroup that combines
 * them in a fixed order), one backward.  No atomics, no workgroup waits for another: bit-stable run to run. */
size_t mm_im_ws_bytes(void);
int mm_im_fwd(const float* logits, int ld, int64_t N, int64_t P, int C, const float* prior, float* stats, float* mass,
              int64_t* count, float* aux, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_im_bwd(const float* logits, int ld, int64_t N, int64_t P, int C, const float* aux, const float* grad_out, float* dlogits,
              int ld_d, mm_stream_t stream);
/* Correlation alignment of two row segments (Deep CORAL, Sun & Saenko, ECCV-W 2016; Deep LogCORAL, Morerio et al., ICLR 2018;
 * csrc/coral.hip).  x: fp32 [N, d], row pitch ld, 2 <= d <= 32.  Rows [0, P) are segment s (source), rows [P, N) segment t (target).
 * A row is counted when its d values are all finite; n_s, n_t of them.  Per segment a, in fp64 from fp64 sums of x and of x xT:
 *   m_a = the mean of the counted rows (0 when there is none);
 *   C_a = 1 / (n_a - 1) * sum_i (x_i - m_a)(x_i - m_a)T      (0 when n_a < 2).
 * mode 0 (plain, Deep CORAL):    L = || C_s - C_t ||_F^2 / (4 d^2);
 * mode 1 (log, Deep LogCORAL):   L = || log(C_s + eps I) - log(C_t + eps I) ||_F^2 / d^2, log the matrix logarithm through the
 *   symmetric eigendecomposition C_a + eps I = V diag(lambda) VT (cyclic Jacobi in fp64, in the kernel), eps > 0 a ridge: a
 *   segment with fewer counted rows than d, or a constant column, has a singular covariance.  An eigenvalue that rounding has
 *   pushed below eps is taken as eps.  Eigenvector signs and order do not enter the result.
 * n_s < 2 or n_t < 2: L = 0 and the gradient is zero (never 0 / 0).
 * Gradient, for both segments: dL/dx_i = 2 / (n_a - 1) * (x_i - m_a) * G_a for a counted row, +0 in every bit for any other row
 * (the derivative of the mean drops out: the centred rows sum to zero).  plain: G_s = -G_t = (C_s - C_t) / (2 d^2).  log, with
 * Delta = log(C_s + eps I) - log(C_t + eps I): G_a = +- (2 / d^2) * V [(VT Delta V) o K] VT (+ for s, - for t; Daleckii-Krein),
 * K_ii = 1 / lambda_i (0 for an eigenvalue that was raised to eps), K_ij = (log lambda_i - log lambda_j) / (lambda_i - lambda_j),
 * evaluated as log1p(t) / (t lambda_j), t = (lambda_i - lambda_j) / lambda_j, from the smaller eigenvalue, with its series for
 * tiny t: close or equal eigenvalues lose no digits and never divide by zero.
 * Outputs of the forward: loss[1]; count[2] = n_s, n_t (int64, exact); mean[2][d], cov[2][d][d] (fp32, for callers and logs);
 * aux[4 d + 2 d^2] = m_s, m_t in fp32, then what that rounding left of the fp64 means (so that x_i - m_a rounds once in the
 * backward, also for a row close to the mean), then the two matrices 2 / (n_a - 1) * G_a, row-major - what the backward reads.
 * The backward writes every one of the N rows once: dx_i = grad_out[0] * (x_i - m_a) * aux_a in fp32.  grad_out and aux are read on the
 * device: no host read anywhere.  Refused before any launch, with no output touched: d outside [2, 32], ld or ld_dx below d,
 * P outside [0, N], N * d >= 2^31, a null operand, a missing or short workspace, eps not finite or <= 0, an unknown mode.
 * N == 0 and P == N are legal and give loss 0.  mm_coral_ws_bytes returns 0 for a d outside the limits.  Two launches forward
 * (fp64 sums and integer row counts per workgroup of a capped grid; one workgroup that totals them in a fixed order, diagonalises
 * and writes the outputs), one backward.  No atomics, no workgroup waits for another: bit-stable run to run. */
size_t mm_coral_ws_bytes(int d);
int mm_coral_fwd(const float* x, int ld, int64_t N, int64_t P, int d, int mode, float eps, float* loss, int64_t* count, float* mean,
                 float* cov, float* aux, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_coral_bwd(const float* x, int ld, int64_t N, int64_t P, int d, const float* aux, const float* grad_out, float* dx, int ld_dx,
                 mm_stream_t stream);
/* Adversarial alignment in the output space with a point-wise discriminator (AdaptSegNet, Tsai et al., CVPR 2018; AdvEnt, Vu et
 * al., CVPR 2019; csrc/adv.hip).  x: fp32 [N, C], row pitch ld, 2 <= C <= 32.  Rows [0, P) are source (domain 0), rows [P, N) target
 * (domain 1).  A row is counted when its C logits are all finite; n_s, n_t of them.  Per counted row, in fp32: p = softmax(x_i)
 * (m = max_c x_c, s = sum_c expf(x_c - m), p_c = expf(x_c - m) / s), and the discriminator's input
 *   mode 0 (softmax, AdaptSegNet):  u_c = p_c;
 *   mode 1 (selfinfo, AdvEnt):      u_c = -p_c ln p_c / ln C, ln p_c taken as (x_c - m) - logf(s); p_c == 0 gives u_c = 0, never NaN.
 * The discriminator: a = w3 . lrelu(W2 lrelu(W1 u + b1) + b2) + b3, lrelu(z) = z > 0 ? z : 0.2 z (its derivative at 0 is 0.2),
 * hidden width H = 16, 32 or 64.  params: ONE flat fp32 buffer of mm_adv_param_count(C, H) = H C + H H + 3 H + 1 floats, in this
 * order: W1 [H][C] row-major, b1 [H], W2 [H][H] row-major, b2 [H], w3 [H], b3.  With softplus(a) = max(a, 0) + log1p(exp(-|a|)):
 *   loss_D = 0.5 / n_s * sum_src softplus(a_i) + 0.5 / n_t * sum_trg softplus(-a_i)     (a domain without a counted row adds 0);
 *   loss_G = 1 / n_t * sum_trg softplus(a_i)          (the target rows called "source"; 0 when n_t == 0).
 * Outputs of mm_adv_fwd: stats[2] = loss_D, loss_G (fp32); count[2] = n_s, n_t (int64, exact); correct[2] (int64) = the counted
 * source rows with a <= 0 and the counted target rows with a > 0; dparams[param_count] = dloss_D / dparams in the order of params,
 * written, not accumulated; gx [N, C], row pitch ld_gx: dloss_G / dx_i on the counted target rows, +0 in every bit on any other
 * row, every row written exactly once.  Through the input transform dL/dx_k = p_k (v_k - sum_c p_c v_c) with v_c = dL/du_c (mode
 * 0) or dL/du_c * (-(ln p_c + 1) / ln C) (mode 1); a class with p_c == 0 contributes exactly 0.
 * mm_adv_bwd: dx = grad_out[0] * gx for every row (a zero stays +0); grad_out is read on the device: no host read anywhere.
 * Products are fp32: the layers' dot products have C and H terms, and an entry of a weight gradient is summed in fp32 over the at
 * most 128 rows of a tile, rows ascending; across the tiles of a workgroup, across workgroups, and for the softplus sums, fp64 in a
 * fixed order.  Refused before any launch, with no output touched: C outside [2, 32], H not 16, 32 or 64, a pitch below C, P
 * outside [0, N], N * C >= 2^31, a null operand (x and gx may be null when N == 0), a missing or short workspace, an unknown mode.
 * N == 0 and P == N are legal.  mm_adv_ws_bytes and mm_adv_param_count return 0 for a C or H outside the limits.  Three launches
 * forward: the row counts per workgroup of a capped grid - 1 / n_s and 1 / n_t enter every row's share of dparams and gx, and a row
 * of gx is written once, so the counts come first -; the row pass over a capped grid, which stages the parameters into LDS once per
 * workgroup and leaves a slab of fp64 sums each; the pass that totals the slabs.  One launch backward.  No atomics, no workgroup
 * waits for another: bit-stable run to run. */
int64_t mm_adv_param_count(int C, int H);
size_t mm_adv_ws_bytes(int C, int H);
int mm_adv_fwd(const float* x, int ld, int64_t N, int64_t P, int C, int H, int mode, const float* params, float* stats, int64_t* count,
               int64_t* correct, float* dparams, float* gx, int ld_gx, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_adv_bwd(const float* gx, int ld_gx, int64_t N, int C, const float* grad_out, float* dx, int ld_dx, mm_stream_t stream);
/* Fourier domain adaptation of the source images (FDA, Yang & Soatto, CVPR 2020; csrc/fda.hip).  src: fp32 [Bs, C, H, W], trg: fp32
 * [Bt, C, H, W], out: fp32 [Bs, C, H, W], all dense.  Per channel, source image i takes the amplitudes of target image i mod Bt on
 * the (2 band + 1) x (2 band + 1) lowest frequencies and keeps its own phases; with F the 2D DFT,
 *   dF[k] = F_src[k] (|F_trg[k]| / |F_src[k]| - 1),  or |F_trg[k]| where F_src[k] is exactly 0 (angle(0) = 0),  |ky|, |kx| <= band,
 *   out[y, x] = src[y, x] + 1 / (H W) * Re sum_k dF[k] e^{+2 pi i (ky y / H + kx x / W)}:
 * what fft2, fftshift, the window [n / 2 - band, n / 2 + band] on both axes, ifftshift, ifft2 and the real part give.  band = 0
 * swaps the DC term alone.  mean, std: fp32 [C] on the device, or both null.  Given, the tensors hold (pixel - mean) / std and the swap
 * is that of the pixels: every term but the DC term scales by 1 / std on both sides, the DC term is taken as std F[0] + mean H W; no
 * de-normalised image is formed.  A non-finite pixel is not special-cased: it spoils its image-channel.
 * mse: fp32 [Bs], the mean over C H W of (out - src)^2 before out is rounded, by Parseval: sum_k |dF[k]|^2 / (H W)^2, averaged over
 * the channels; no pass over the images.  Every sum and every twiddle factor is fp64, phases are reduced in integers, every sum has a
 * fixed order: no atomics, no host read, the same bits on every call.  Three launches: the row DFT of all images onto the
 * band's column frequencies with each row tile's share of the column DFT, one workgroup per (source image, channel) that totals
 * the shares and makes the swap, and the apply pass, which takes the inverse column transform of its own rows first.  Refused before any launch, with no output touched: a null src, trg, out or mse; mean and std not
 * both null or both set; Bs, Bt, H or W < 1; Bs or Bt > 2^20; C outside [1, 4]; H or W > 2048 (the LDS twiddle tables); band outside
 * [0, 32] or 2 band + 1 > min(H, W); a missing or short workspace.  mm_fda_ws_bytes returns 0 for sizes outside these limits. */
size_t mm_fda_ws_bytes(int Bs, int Bt, int C, int H, int W, int band);
int mm_fda_transfer(const float* src, int Bs, const float* trg, int Bt, int C, int H, int W, int band, const float* mean,
                    const float* std, float* out, float* mse, void* ws, size_t ws_bytes, mm_stream_t stream);
/* mean_i sum_c softmax(tgt)_ic (log softmax(tgt)_ic - log softmax(pred)_ic)  (EXP/train.py:157-184) */
int mm_kl_fwd(const float* pred, int ld_p, const float* tgt, int ld_t, int64_t N, int C, float* loss, void* ws,
              size_t ws_bytes, mm_stream_t stream);
int mm_kl_bwd(const float* pred, int ld_p, const float* tgt, int ld_t, int64_t N, int C, const float* grad_out,
              float* dpred, int ld_d, mm_stream_t stream);
/* The lifting index built on the device in three launches (csrc/lift.hip; round 4).  rc: device int64 [n, 2] (row, col) of every
 * point, scenes concatenated (img_indices of lib/dataset/__init__.py:74,111); counts: device int64 [nb] points per scene.
 * key [n] = pixel id (b*H + row)*W + col (rows / cols clamped into the map; err[0] = 1 if one was outside - the reference asserts
 * these bounds in its loader, nuscenes_dataloader.py:280-283); skey / order [n] = the keys ascending and the point at each sorted
 * position (stable radix sort).  no_spin: see mm_voxel_dedupe. */
size_t mm_lift_index_ws_bytes(int64_t n);
int mm_lift_index(const int64_t* rc, const int64_t* counts, int nb, int64_t n, int H, int W, int no_spin, int32_t* key, int32_t* skey,
                  int32_t* order, int32_t* err, void* ws, size_t ws_bytes, mm_stream_t stream);
/* The stable sort of mm_lift_index alone, over keys the caller supplies, each in [0, nkeys) (the matched pixels of mm_xm_search
 * change every step): skey / order [n] as above.  Same radix configuration, workspace (mm_lift_index_ws_bytes(n)) and no_spin rule. */
int mm_lift_sort_keys(const int32_t* key, int64_t n, int64_t nkeys, int no_spin, int32_t* skey, int32_t* order, void* ws,
                      size_t ws_bytes, mm_stream_t stream);
/* Sparse-to-dense cross-modal matching (the window search of DsCML, Peng et al., ICCV 2021; csrc/xmdense.hip).  seg: a dense fp32
 * logit map of B images, H x W pixels, C classes (2 <= C <= 32), element (b, y, x, c) at seg[b*sb + y*sy + x*sx + c*sc] - a channel
 * slice of a wider NHWC buffer or an NCHW map alike.  key [N]: the pixel id (b*H + y)*W + x of every point (mm_lift_index);
 * rows: fp32 [N, C] with row pitch ld, the points' own logits.  The candidates of point i are the pixels (b, y+dy, x+dx) with
 * |dy|, |dx| <= r (0 <= r <= 3) inside image b, in the order: the centre, then the others row-major (dy ascending, then dx).
 *   direction 0: value_j = KL(softmax(rows_i) || softmax(seg_j))   (the point row teaches the map);
 *   direction 1: value_j = KL(softmax(seg_j) || softmax(rows_i))   (the map teaches the point row);
 * in fp32, sum_c exp(lq_c) * (lq_c - lp_c) over the two log-softmax rows, as mm_kl_fwd forms it.  sel [N] = the key of the candidate
 * with the smallest value, the earliest among equal ones; a NaN value is skipped; nothing left: the centre.  klmin [N] = that
 * candidate's value.  A key outside [0, B*H*W) reads nothing: sel = key, klmin = NaN.  counts (int64 [4]): the number of rows of
 * [0, P) and of [P, N) whose match left the centre, then the sums of their Chebyshev displacements max(|dy|, |dx|).
 * r = 0 is legal: sel == key, klmin the centre's value.  Refused before any launch: r outside [0, 3], C outside [2, 32], a
 * direction other than 0 / 1, P outside [0, N], N * C >= 2^31, ld < C, a map of 2^31 pixels or more, a null operand, a short
 * workspace.  Two launches; no atomics, no host read: bit-stable run to run. */
size_t mm_xm_search_ws_bytes(void);
int mm_xm_search(const float* seg, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int B, int H, int W, int C, const int32_t* key,
                 const float* rows, int ld, int64_t N, int64_t P, int r, int direction, int32_t* sel, float* klmin, int64_t* counts,
                 void* ws, size_t ws_bytes, mm_stream_t stream);
/* out[p][c] = seg[b*sb + row*sy + col*sx + c*sc] at the pixel of point p (2d_net/model.py:131-137) */
int mm_lift_gather_key(const float* seg, int64_t sb, int64_t sy, int64_t sx, int64_t sc, const int32_t* key, int64_t N, int C, int H,
                       int W, float* out, mm_stream_t stream);
/* its backward: dseg (zero-filled by the caller) at every pixel with points = the sum of dout over them, ascending point order */
int mm_lift_scatter_key(const float* dout, int C, const int32_t* order, const int32_t* skey, int64_t N, int H, int W, int64_t sb,
                        int64_t sy, int64_t sx, int64_t sc, float* dseg, mm_stream_t stream);
/* evaluation (EXP/train.py:297-339): confusion matrices [3][C][C] int64 of argmax(2D), argmax(3D), argmax(softmax mean) */
int mm_eval_confusion(const float* logits2d, int ld2, const float* logits3d, int ld3, const int64_t* labels, int64_t N,
                      int C, int64_t ignore_index, int64_t* cm, mm_stream_t stream);
/* ---------------------------------------------------------------- pseudo labels (csrc/pselab.hip)
 * mm_pselab_predict: what a self-training round stores per point (the files lib/dataset/*_dataloader.py read back): for the 2D
 * logits, the 3D logits and the softmax average 0.5 * (softmax2d + softmax3d) (EXP/train.py:315-318) the largest probability
 * (fp32 [N]) and its class (uint8 [N], the first maximum wins).  Same arithmetic as mm_eval_confusion (one shared device function):
 * the exported labels are the labels evaluation counts.  logits [N, C] fp32 with row pitches ld2 / ld3 >= C, C <= 32.
 * logits3d may be NULL (2D-only export): then only probs_2d / label_2d are written and the other four may be NULL. */
int mm_pselab_predict(const float* logits2d, int ld2, const float* logits3d, int ld3, int64_t N, int C, float* probs_2d,
                      uint8_t* label_2d, float* probs_3d, uint8_t* label_3d, float* probs_ensemble, uint8_t* label_ensemble,
                      mm_stream_t stream);
/* The labels a mean teacher gives a target batch inside the training step: ONE launch over N rows of both logit matrices, each row
 * through the device expression of mm_pselab_predict (an online label is the label an export would have written).  ensemble == 0:
 * label_2d = argmax of the 2D softmax with its confidence, label_3d = the 3D one; ensemble != 0: both outputs get the argmax of the
 * softmax average and its confidence.  thr >= 0: a label whose confidence p does not satisfy p >= thr (float32; a non-finite
 * confidence fails it) becomes ignore_label; thr < 0 keeps every label.  prob_2d / prob_3d (fp32 [N], may be NULL) receive the
 * confidences; kept (may be NULL) receives the number of kept labels per output in kept[0] / kept[1]: zeroed on the stream here,
 * summed per workgroup and added with 64-bit integer atomics (exact in any order).  logits [N, C] fp32 with row pitches >= C,
 * C <= 32; N == 0 launches nothing and writes nothing. */
int mm_teacher_labels(const float* logits2d, int ld2, const float* logits3d, int ld3, int64_t N, int C, int ensemble, float thr,
                      int64_t ignore_label, int64_t* label_2d, int64_t* label_3d, float* prob_2d, float* prob_3d,
                      unsigned long long* kept, mm_stream_t stream);
/* mm_teacher_labels with one threshold per output and class: thr_cls[2][C] fp32 on the device (row 0 the 2D output's, row 1 the
 * 3D output's) in place of thr.  Output o keeps a row iff p >= thr_cls[o][y] in float32, y the row's label of that output; there
 * is no "keep all" value.  The same kernel: labels, confidences and counts are otherwise those of mm_teacher_labels. */
int mm_teacher_labels_cls(const float* logits2d, int ld2, const float* logits3d, int ld3, int64_t N, int C, int ensemble,
                          const float* thr_cls, int64_t ignore_label, int64_t* label_2d, int64_t* label_3d, float* prob_2d,
                          float* prob_3d, unsigned long long* kept, mm_stream_t stream);
/* Self-adaptive per-class pseudo-label thresholds (FreeMatch, Wang et al., ICLR 2023), state on the device, no host read.
 * Per output o (0: 2D, 1: 3D): state[o][0] = tau_o, state[o][1 + c] = pt_o[c] (fp64, the caller initialises all to 1 / C),
 * count[o] = updates taken.  With p, y the confidence and label mm_teacher_labels gives the row for that output and q[c] the
 * float32 per-class values behind them (softmax of the output's logits, or with ensemble != 0 the softmax average for both):
 *   counted    a row enters output o's statistics iff p >= 0 in float32 (a NaN confidence, or the ensemble's -1 of a non-finite
 *              row, fails: the rows threshold 0 refuses); n_o = the counted rows;
 *   update     if n_o > 0: m_t = momentum, or with warmup != 0 min(momentum, (1 + count[o]) / (10 + count[o]));
 *              tau_o <- m_t * tau_o + (1 - m_t) * mean p;  pt_o[c] <- m_t * pt_o[c] + (1 - m_t) * mean q[c];  count[o] += 1.
 *              n_o == 0 leaves state and count as they are;
 *   thr        thr[o][c] = (float)((pt_o[c] / max_c pt_o[c]) * tau_o), in fp64 in this order, always written from the (possibly
 *              unchanged) state: what mm_teacher_labels_cls and mm_ce2s_*_cls take.
 * Two launches: fp64 partial sums and integer row counts per workgroup of a capped grid, then one workgroup that sums them in a
 * fixed order, updates the state in place and writes thr.  No atomics: bit-stable run to run.  N == 0 runs the second launch
 * alone.  momentum in [0, 1); C <= 32; every argument check is made before the first launch. */
size_t mm_pl_adapt_ws_bytes(void);
int mm_pl_adapt(const float* logits2d, int ld2, const float* logits3d, int ld3, int64_t N, int C, int ensemble, double momentum,
                int warmup, double* state, int64_t* count, float* thr, void* ws, size_t ws_bytes, mm_stream_t stream);
/* Row weights from the agreement of the two modalities (the uncertainty weighting of Zheng & Yang, IJCV 2021, between the 2D and
 * the 3D prediction of a row).  For row i with logit rows a (2D) and b (3D) of C classes, p = softmax(a), q = softmax(b),
 * lp_c = a_c - logsumexp(a), lq_c = b_c - logsumexp(b) (no log of a probability is taken), all in float32:
 *   D_i = 0.5 * sum_c (p_c - q_c) * (lp_c - lq_c)   half the Jeffreys divergence 0.5 * (KL(p||q) + KL(q||p)): >= 0, symmetric;
 *         a term with p_c == q_c is 0; the sum runs ascending in c and is clamped at 0 from below;
 *   w_i = expf(-beta * D_i)                          in [0, 1]; exactly 1 for identical rows.
 * A row with a non-finite logit in either matrix gets w_i = 0 and is left out of the mean of D.  Outputs: w [N];
 * stats[0] = (1 / N) sum_i w_i (0 when N == 0); stats[1] = the mean of D over the n finite rows (0 when n == 0); finite (may be
 * NULL) receives n, exact.  Two launches: a capped grid stages 128-row tiles through LDS, writes w and leaves two fp64 sums and
 * an integer count per workgroup; one workgroup combines them in a fixed order.  No atomics, no workgroup waits for another, no
 * host read: bit-stable run to run.  N == 0 runs the second launch alone.  2 <= C <= 32, ld2 / ld3 >= C, beta finite and > 0,
 * N * C < 2^31; anything else is refused before the first launch. */
size_t mm_pl_agree_ws_bytes(void);
int mm_pl_agree(const float* logits2d, int ld2, const float* logits3d, int ld3, int64_t N, int C, float beta, float* w,
                float* stats, int64_t* finite, void* ws, size_t ws_bytes, mm_stream_t stream);
/* lib/utils/refine_pseudo_labels.py, exact: for every class c of [0, C) that occurs n_c > 0 times, med_c = the element of rank
 * (n_c - 1) / 2 (ascending, 0-based: torch.median's lower median) among the probs of that class, thr_c = min(med_c, 0.9f);
 * labels_out[i] = ignore_label where labels[i] == c and probs[i] < thr_c, else labels[i].  Labels outside [0, C) pass through.
 * An exact radix select (four 8-bit passes, integer counts): deterministic, no host read-back.  probs must be FINITE (a NaN has
 * no place in the order); N < 2^40, C <= 32.  ws: mm_pselab_refine_ws_bytes(C) bytes of device scratch (0 for a bad C). */
size_t mm_pselab_refine_ws_bytes(int C);
int mm_pselab_refine(const float* probs, const int64_t* labels, int64_t N, int C, int64_t ignore_label, int64_t* labels_out,
                     void* ws, size_t ws_bytes, mm_stream_t stream);

/* ---------------------------------------------------------------- AdamW / Adam / SGD / RMSprop over flat arenas (csrc/optim.hip)
 * The four names of the reference's optimiser registry (lib/optimizers.py: adamw, adam, sgd, rmsprop; its trainer runs AdamW,
 * EXP/train.py:627-636), one fused launch per touched range: fp32 arithmetic in the op order of torch.optim.{SGD, Adam, AdamW,
 * RMSprop}'s single-tensor paths, g is multiplied by grad_scale.  skip_dev / nskip (0 .. 16, may be NULL / 0): device words - the
 * update is a no-op when any of them is nonzero (the data-parallel reducer's collective "this step's gradients are invalid" flags:
 * decided on the device, no read-back).  A state array that the hyper-parameters do not need is NULL and is neither read nor
 * written; a non-NULL pointer selects the variant:
 *   mm_sgd_step      buf = momentum buffer (NULL: no momentum); nesterov needs it.  ``step`` counts the optimiser's taken steps
 *                    from 1: on step 1 buf = g (torch's rule, no dampening), afterwards buf = momentum*buf + (1-dampening)*g.
 *   mm_adam_step     m, v; vmax = amsgrad's running maximum of v (NULL: amsgrad off).  decoupled = 0: weight decay is L2
 *                    (torch.optim.Adam); 1: p *= 1 - lr*wd (torch.optim.AdamW).  ``step`` (from 1) drives the bias corrections.
 *   mm_rmsprop_step  sq; gavg = gradient average (NULL: not centered); buf = momentum buffer (NULL: no momentum).
 * Loss-scaled form (the fp16 kind of the 16-bit activation mode; torch.cuda.amp.GradScaler semantics as driven by the reference's
 * ``precision: 16`` trainer, train.yaml:11) WITHOUT a read-back: scale, non-finite flags, clean-step tracker and step counter
 * live on the device.  mm_grad_nonfinite: found_dev[0] = 1 if any gradient is inf / nan (the caller zeroes it).  mm_*_prepare
 * (one thread) writes one parameter group's coefficients (mm_optim_coef_bytes bytes: 1 / scale, Adam's bias corrections, SGD's
 * first-step rule, and "skip") from the device-resident scale, flag words and step counter.  "skip" = any of
 * found_dev[0 .. nfound) set: ONE decision from the flags of EVERY optimiser of the step (the reference's HybridOptim is one
 * optimiser to the GradScaler, EXP/train.py:627-636: an overflow in either network skips both updates) plus the caller's extra
 * skip words.  The counter advances only when the step is taken and ``advance`` is set; ``advance`` is 1 for the first parameter
 * group of an optimiser and 0 for the others, which read the step the first one committed.  mm_*_step_dev applies the
 * coefficients and is a no-op when they say "skip"; mm_amp_update: GradScaler.update() on the real scale. */
int mm_grad_nonfinite(const float* g, int64_t n, int* found_dev, mm_stream_t stream);
int mm_amp_update(float* scale_dev, int* tracker_dev, const int* found_dev, int nfound, double growth, double backoff, int interval,
                  mm_stream_t stream);
int mm_optim_coef_bytes(void);
int mm_sgd_step(float* p, const float* g, float* buf, int64_t n, double lr, double momentum, double dampening, double weight_decay,
                int nesterov, int64_t step, double grad_scale, const int* skip_dev, int nskip, mm_stream_t stream);
int mm_adam_step(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, double lr, double beta1, double beta2,
                 double eps, double weight_decay, int decoupled, int64_t step, double grad_scale, const int* skip_dev, int nskip,
                 mm_stream_t stream);
int mm_rmsprop_step(float* p, const float* g, float* sq, float* gavg, float* buf, int64_t n, double lr, double alpha, double eps,
                    double weight_decay, double momentum, double grad_scale, const int* skip_dev, int nskip, mm_stream_t stream);
int mm_sgd_prepare(const float* scale_dev, const int* found_dev, int nfound, int64_t* step_dev, int advance, double lr,
                   double momentum, double dampening, double weight_decay, double grad_scale, void* coef_dev, mm_stream_t stream);
int mm_adam_prepare(const float* scale_dev, const int* found_dev, int nfound, int64_t* step_dev, int advance, double lr,
                    double beta1, double beta2, double eps, double weight_decay, int decoupled, double grad_scale, void* coef_dev,
                    mm_stream_t stream);
int mm_rmsprop_prepare(const float* scale_dev, const int* found_dev, int nfound, int64_t* step_dev, int advance, double lr,
                       double alpha, double eps, double weight_decay, double momentum, double grad_scale, void* coef_dev,
                       mm_stream_t stream);
int mm_sgd_step_dev(float* p, const float* g, float* buf, int64_t n, int nesterov, const void* coef_dev, mm_stream_t stream);
int mm_adam_step_dev(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, int decoupled, const void* coef_dev,
                     mm_stream_t stream);
int mm_rmsprop_step_dev(float* p, const float* g, float* sq, float* gavg, float* buf, int64_t n, const void* coef_dev,
                        mm_stream_t stream);

/* ---------------------------------------------------------------- mean-teacher weights over the flat arenas (csrc/optim.hip)
 * An exponential moving average of the weights (mm2d3d_amd/ema.py WeightEMA), gated ON THE DEVICE by the decision that gated the
 * optimiser update of the same step, so a skipped step is neither averaged in nor counted.  table_dev: nrows rows of
 * mm_ema_row_bytes() bytes in device memory, one per tensor pair:
 *     { float* dst; float* src; int64 n; int64 first; }
 * dst = the teacher's tensor, src = the live one, n = elements (0 is legal), first = the number of the row's first workgroup =
 * the sum of ceil(n / 1024) over the rows before it; nblocks = that sum over all rows.  A workgroup finds its row by binary
 * search over ``first``; a thread owns four consecutive elements and uses 16-byte accesses when both pointers of the row are
 * 16-byte aligned and the four elements fit.  The pairs must not overlap.
 *   mm_ema_update  dst = lerp(dst, src, w) in fp32 (d = src - dst; w < 0.5 ? dst + w*d : src - d*(1 - w)), w = (float)(1 - decay_t),
 *                  decay_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay in double, t = *step_dev (device int64) when step_dev
 *                  is not NULL, else t_host: the optimiser's count of TAKEN steps after this step's update.  Nothing is written
 *                  when any of skip_dev[0 .. nskip) (nskip 0 .. 16) is nonzero, or when coef_dev is not NULL and the coefficients
 *                  it points to (mm_optim_coef_bytes, written by mm_*_prepare) say "skip".  0 <= decay < 1.
 *   mm_ema_swap    exchanges the CONTENTS of dst and src of every row (pointers stay: parameters are views into the arenas). */
int mm_ema_row_bytes(void);
int mm_ema_update(const void* table_dev, int nrows, int64_t nblocks, double decay, int warmup, int64_t t_host, const int64_t* step_dev,
                  const void* coef_dev, const int* skip_dev, int nskip, mm_stream_t stream);
int mm_ema_swap(const void* table_dev, int nrows, int64_t nblocks, mm_stream_t stream);

/* ---------------------------------------------------------------- gradient clipping for the flat optimisers (csrc/clip.hip)
 * torch.nn.utils.clip_grad_norm_ (norm_type 2) / clip_grad_value_ on the TRUE gradient g * grad_scale / scale of arenas that hold
 * loss-scaled, un-averaged gradients (Lightning's gradient_clip_val / gradient_clip_algorithm, EXP/run.py:262-288).  No read-back.
 *   mm_grad_sqnorm     sum of squares of one fp32 arena in double (a finite arena never gives a non-finite sum): one double
 *                      partial per workgroup into partial_ws[slot .. slot + mm_grad_sqnorm_ws_bytes(n) / 8).  Which workgroup
 *                      sums which elements depends on n and on g's offset from a 16-byte boundary only, never on the device.
 *                      found_dev (may be NULL): found_dev[0] = 1 if an element is inf / nan, as mm_grad_nonfinite sets it.
 *   mm_clip_finalize   one workgroup: adds counts[0] + .. + counts[narenas - 1] consecutive partials (the arenas of EVERY
 *                      optimiser of the step: one joint norm) in a fixed order, so the result is the same bits on every run;
 *                      norm_out_dev[0] = sqrt(sum) * grad_scale / scale_dev[0] (fp32), c = min(1, max_norm / (norm + 1e-6)) as
 *                      torch forms it (NaN for a NaN norm), eff_scale_out_dev[0] = scale_dev[0] / c.  Passed as scale_dev to
 *                      mm_*_prepare, the effective scale makes the update kernels apply grad_scale * c / scale.
 *                      mm_amp_update keeps the real scale.
 *   mm_grad_clip_value clamps g in place to +-clip_value * scale_dev[0] / grad_scale, i.e. the true gradient to +-clip_value;
 *                      a NaN passes through, as in torch.clamp. */
size_t mm_grad_sqnorm_ws_bytes(int64_t n);
int mm_grad_sqnorm(const float* g, int64_t n, void* partial_ws, int64_t slot, int* found_dev, mm_stream_t stream);
int mm_clip_finalize(const void* partial_ws, const int64_t* counts, int narenas, const float* scale_dev, double grad_scale,
                     double max_norm, float* norm_out_dev, float* eff_scale_out_dev, mm_stream_t stream);
int mm_grad_clip_value(float* g, int64_t n, double clip_value, const float* scale_dev, double grad_scale, mm_stream_t stream);

/* ---------------------------------------------------------------- dense 2D convolutions (csrc/conv2d.hip)
 * torch.nn.Conv2d / ConvTranspose2d of EXP/2d_net/backbones.py:43-65 and EXP/2d_net/model.py:64-82,104-123.
 * NHWC bf16 activations, fp32 accumulate.  mm_conv2d_gemm: out[m][n] = sum_{tap,k} A[src(m,tap)][k] * Wp[n][tap][k]
 * with m -> (b,gy,gx) on the base grid Hg x Wg, src = ((gy*sa+ty)/fr, (gx*sa+tx)/fr), out pixel = (gy*so+ooy(+z>>1),
 * gx*so+oox(+z&1)); covers Conv2d fwd / dgrad (stride 1, 2) and ConvTranspose2d(k2,s2) fwd / dgrad. */
int mm_conv2d_gemm(const void* A, int B, int Hi, int Wi, int Ca, int lda, void* O, int Ho, int Wo, int Cn, int ldo,
                   int out_f32, int Hg, int Wg, int so, int ooy, int oox, int sa, int fr, int ntaps, const int* ty,
                   const int* tx, const void* Wp, int nz, int64_t wz, int zpar, const float* bias, float* stats,
                   int64_t split_m, const void* addend, int ld_add, mm_stream_t stream);
/* ``addend`` (16-bit output only): a 16-bit map of the output's shape (pixel pitch ld_add) added to the result, element by element
 * as an add of the two maps would - the second gradient contribution of a map with two consumers (a BasicBlock input read by conv1
 * and by the 1x1 downsample; the decoder's concat slice) joins here instead of in an add kernel. */
/* The data gradient of a STRIDE-2 convolution (k = 1 or 3; EXP/2d_net/backbones.py layer2-4.0: conv1 and the 1x1 downsample) by output
 * parity: an input pixel of parity (py, px) receives only the taps with kh = py + pad, kw = px + pad (mod 2) - 1 + 2 + 2 + 4 of a 3x3
 * filter's nine, 1 + 0 + 0 + 0 of a 1x1's - so the four parities run as four tap windows of one launch instead of every tap for
 * every pixel with three quarters of them multiplying zeros (mm_conv2d_gemm with fr = 2).  dY [B,Ho,Wo,Cout] (pitch ldy), dX
 * [B,H,W,Cin] (pitch ldx; H, W even), Wd [Cin][k*k][Cout]; addend as in mm_conv2d_gemm.  Bit-identical with the generic form. */
int mm_conv2d_dgrad_s2(const void* dY, int B, int Ho, int Wo, int Cout, int ldy, void* dX, int H, int W, int Cin, int ldx, const void* Wd,
                       int k, int pad, const void* addend, int ld_add, mm_stream_t stream);
/* BatchNorm statistics in the epilogue (``stats`` non-NULL; 16-bit output only): the convolution also files, per 64-pixel
 * sub-block of its output and per statistics group, the per-channel sum and sum of squares of the ROUNDED outputs in
 *     stats[2 * sub + g][q][Cn] fp32   (q = 0: sum, 1: sum of squares; rows = mm_conv2d_gemm_stat_rows / _3x3s1_stat_rows)
 * every element of which is written by exactly one lane (no atomics, no zero fill needed).  Group 0 = GEMM rows [0, split_m)
 * (mm_conv2d_gemm, rows within one z slice) / batch entries [0, split_b) (mm_conv2d_3x3s1), group 1 = the others: the
 * [source | target] halves of the joint pass (xmuda.py:45-46 calls the network once per domain).  mm_bn2d_fwd_train_pre turns
 * the slab into batch statistics - the training BatchNorm2d behind a convolution then never reads the map for its sums. */
int64_t mm_conv2d_gemm_stat_rows(int64_t M, int nz);
int64_t mm_conv2d_3x3s1_stat_rows(int B, int H, int W);
/* 3x3 stride-1 pad-1 convolution (flip 0) or its data gradient (flip 1, Wp = [ci][tap][co]) from a halo tile staged once
 * for all 9 taps (EXP/2d_net/backbones.py ResNet34 BasicBlocks; EXP/2d_net/model.py:68-71 decoder convolutions).
 * flip | 2: a ragged last round of work items is NOT cut into half items (A/B measurements; results are the same sums).
 * flip bits 2-3 choose the kernel (A/B measurements and the identity tests; the results are the same sums):
 *   0  the round-6 kernels: k_conv3x3s (four multiplying + four loader waves, 16x16x32 MFMAs; 64 -> 64 layers with the nine weight
 *      tiles resident in LDS) - equal to the others up to the fp32 summation order inside one 32-deep product;
 *   4  the round-2 kernel k_conv3x3w (16 waves, 32x32x16 MFMAs; 64 -> 64: the round-3 weights-resident k_conv3x3r);
 *   8  k_conv3x3v (the 8-wave layout on 32x32x16 MFMAs): bit-identical with 4;
 *  12  k_conv3x3s in its streaming form also for 64 -> 64. */
int mm_conv2d_3x3s1(const void* A, int B, int H, int W, int Ca, int lda, void* O, int Cn, int ldo, const void* Wp,
                    const float* bias, int flip, float* stats, int split_b, mm_stream_t stream);
/* Two such convolutions (or data gradients) of ONE shape - the same layer of the RGB and of the depth encoder, EXP/2d_net/model.py:43-46 -
 * in one launch: one work-item list over both problems, so the persistent kernel's partly filled last round is shared (at the
 * bench's sizes a 256-channel layer alone leaves half the chip idle for a third of its time).  Same results as two calls. */
int mm_conv2d_3x3s1_pair(const void* A0, const void* A1, int B, int H, int W, int Ca, int lda, void* O0, void* O1, int Cn, int ldo,
                         const void* Wp0, const void* Wp1, int flip, float* stats0, float* stats1, int split_b, mm_stream_t stream);
size_t mm_conv2d_wgrad_ws_bytes(int64_t M, int Cn, int Ck, int ntaps);
/* dW[n*sn + t*st + k*sk] (+)= sum_m dY[m][n] * X[src(m,t)][k], base grid = dY pixels */
int mm_conv2d_wgrad(const void* X, int B, int Hi, int Wi, int Ck, int ldx, const void* dY, int Hg, int Wg, int Cn,
                    int ldy, int sa, int ntaps, const int* ty, const int* tx, float* dW, int64_t sn, int64_t st,
                    int64_t sk, int accumulate, void* ws, size_t ws_bytes, mm_stream_t stream);
/* The weight gradients of TWO 3x3 stride-1 pad-1 convolutions of one shape (the same layer of the two encoders) in the two launches
 * one of them takes: twice the pixels per workgroup, half the partial slabs per problem.  ws: mm_conv2d_wgrad_ws_bytes(B*H*W, Cn, Ck, 9). */
int mm_conv2d_wgrad3x3_pair(const void* X0, const void* X1, int B, int H, int W, int Ck, int ldx, const void* dY0, const void* dY1, int Cn,
                            int ldy, float* dW0, float* dW1, int64_t sn, int64_t st, int64_t sk, int accumulate, void* ws, size_t ws_bytes,
                            mm_stream_t stream);
/* The same two weight-gradient forms WITHOUT their slab sums (round 5): ``slabs`` (mm_conv2d_wgrad_ws_bytes bytes; the caller keeps
 * it until the sum has run) receives the fp32 partial slabs [*nsplit][Cn][ntaps][Ck] (pair: [2][*nsplit][Cn][9][Ck]), and ONE
 * mm_conv2d_wgrad_reduce_batch launch later sums the slabs of every layer of a backward pass into their gradients - the per-layer
 * sums were ~50 launches of ~14 us per training step.  Same sums in the same order: bit-identical with mm_conv2d_wgrad.
 * descs_dev: n descriptors of mm_conv2d_wgrad_reduce_desc_bytes() bytes on the device: {const float* slabs; float* dW; float* dW1
 * (the pair's second gradient, else NULL); int64 sn, st, sk; int32 nsplit, Cn, ntaps, Ck, accumulate, blk_first}, blk_first = the
 * running sum of mm_conv2d_wgrad_reduce_blocks(Cn, Ck, pair) over the preceding descriptors, total_blocks = the sum over all. */
int mm_conv2d_wgrad_slabs(const void* X, int B, int Hi, int Wi, int Ck, int ldx, const void* dY, int Hg, int Wg, int Cn, int ldy,
                          int sa, int ntaps, const int* ty, const int* tx, void* slabs, size_t slab_bytes, int* nsplit,
                          mm_stream_t stream);
int mm_conv2d_wgrad3x3_pair_slabs(const void* X0, const void* X1, int B, int H, int W, int Ck, int ldx, const void* dY0, const void* dY1,
                                  int Cn, int ldy, void* slabs, size_t slab_bytes, int* nsplit, mm_stream_t stream);
int mm_conv2d_wgrad_reduce_desc_bytes(void);
int64_t mm_conv2d_wgrad_reduce_blocks(int Cn, int Ck, int pair);
int mm_conv2d_wgrad_reduce_batch(const void* descs_dev, int n, int64_t total_blocks, mm_stream_t stream);
/* The 7x7 stride-1 stems (EXP/2d_net/backbones.py:23-25) on the staged image of mm_stem_prep: xb [B][Hb][Wb][8] with R = 8 / C image
 * rows stacked per buffer pixel, T = ceil(7 / R) taps of 8 pixels x 8 slots, Wp [64][T][64]; output O [B][H][W][64] (pitch ldo).
 * One persistent kernel with the weights resident in LDS and the RAW strip of a 16 x 16 tile staged once - the generic implicit GEMM
 * fetched 128 bytes per output pixel and tap, 16 times the strip's bytes.  stats / split_b: BatchNorm statistics slab as for
 * mm_conv2d_3x3s1, mm_conv2d_stem7_stat_rows(B, H, W) rows. */
int64_t mm_conv2d_stem7_stat_rows(int B, int H, int W);
int mm_conv2d_stem7(const void* xb, int B, int Hb, int Wb, int H, int W, int R, int T, void* O, int ldo, const void* Wp, float* stats,
                    int split_b, mm_stream_t stream);
/* stem input (EXP/2d_net/backbones.py:23-25, 7x7 stride-1 conv on 3 / 1 channels): NCHW fp32 -> zero-bordered NHWC8 bf16 */
int mm_stem_prep(const float* in, int B, int C, int H, int W, int pad, int Hb, int Wb, int R, void* out, mm_stream_t stream);
/* out[((z*N+n)*T+t)*K+k] = bf16(in[z*sz + n*sn + t*st + k*sk]) : fp32 master weights -> kernel layouts */
int mm_pack_weights_bf16(const float* in, void* out, int Z, int N, int T, int K, int64_t sz, int64_t sn, int64_t st,
                         int64_t sk, mm_stream_t stream);
/* One launch for a table of weights (every conv layer of a model after an optimiser step).  desc (device memory):
 * ndesc rows of 11 int64 {in, out, Z, N, T, K, sz, sn, st, sk, first_block}; first_block = running sum of
 * ceil(Z*N*T*K / 4096) over the preceding rows (Z*N*T*K < 2^31 per row), total_blocks = the sum over all rows. */
int mm_pack_weights_bf16_batch(const int64_t* desc, int ndesc, int64_t total_blocks, mm_stream_t stream);

/* ---------------------------------------------------------------- BatchNorm2d (+residual) (+ReLU), NHWC bf16 (csrc/bn2d.hip) */
size_t mm_bn2d_ws_bytes(int C);
/* Maps that fit on chip (every map of the headline step but the largest ones) take single-launch training kernels:
 * one workgroup per CU keeps its rows in registers / LDS across two grid barriers, so x (and dy) are read once - when the handle
 * allows it: mm_set_option(h, MM_OPT_BN2D_FUSED, mask), bit 0 = mm_bn2d_fwd_train, bit 1 = mm_bn2d_bwd, 0 = always the
 * reduce / finalize / apply kernels (see mm_set_option for when). */
/* Ns: rows [0,Ns) and [Ns,N) are normalised with their OWN batch statistics (the source / target halves of a jointly
 * batched step; train.py:186-292 calls each net once per domain) and the running buffers are updated group 0 first,
 * then group 1, as two consecutive calls would.  Ns = N (or 0): ordinary single batch.  save_mean/save_invstd: [G][C]. */
int mm_bn2d_fwd_train(mm_handle_t h, const void* x, int ld_x, const void* res, int ld_r, int64_t N, int64_t Ns, int C, const float* weight,
                      const float* bias, float* running_mean, float* running_var, int64_t* num_batches_tracked, float eps,
                      float momentum, int relu, void* y, int ld_y, float* save_mean, float* save_invstd, void* ws,
                      size_t ws_bytes, mm_stream_t stream);
/* The same with the batch statistics taken from the slab the producing convolution filled (mm_conv2d_gemm / mm_conv2d_3x3s1
 * ``stats``, slab_rows = its *_stat_rows): a finalize launch (fp64 sums in a fixed order) + one streaming apply pass.  No pass
 * over x for the sums, no grid barrier, hence no handle and no residency rule. */
/* 1 when mm_bn2d_fwd_train (backward = 0) / mm_bn2d_bwd (1) would run as ONE launch for N rows of C channels under the handle's
 * present options (shape rule only).  The Python layer asks before a convolution: maps too large for one launch get their
 * statistics from the convolution's epilogue (mm_bn2d_fwd_train_pre), the others are read once by the single-launch kernel anyway. */
int mm_bn2d_single_launch(mm_handle_t h, int64_t N, int64_t Ns, int C, int backward);
int mm_bn2d_fwd_train_pre(const void* x, int ld_x, const void* res, int ld_r, int64_t N, int64_t Ns, int C, const float* weight,
                          const float* bias, float* running_mean, float* running_var, int64_t* num_batches_tracked, float eps,
                          float momentum, int relu, void* y, int ld_y, float* save_mean, float* save_invstd, const float* slab,
                          int64_t slab_rows, void* ws, size_t ws_bytes, mm_stream_t stream);
/* Two BatchNorm2d problems of ONE shape (N, Ns, C and the scalars shared) - the same layer of the RGB and of the depth encoder,
 * EXP/2d_net/model.py:43-46 - as ONE single-launch kernel where the maps allow it: half the CUs per problem, one pair of grid barriers
 * and one statistics exchange for both (the small maps of the encoders' layers 2-4 are bound by those fixed costs, not by bytes);
 * otherwise the two problems run one after the other exactly as mm_bn2d_fwd_train / mm_bn2d_bwd run them.  Same results either way. */
typedef struct mm_bn2d_fwd_args {
  const void* x; int ld_x; const void* res; int ld_r; const float* weight; const float* bias; float* running_mean; float* running_var;
  int64_t* num_batches_tracked; void* y; int ld_y; float* save_mean; float* save_invstd;
} mm_bn2d_fwd_args;
typedef struct mm_bn2d_bwd_args {
  const void* x; int ld_x; const void* dy; int ld_dy; const void* dy2; int ld_dy2; const void* yout; int ld_y;
  const float* weight; const float* bias; const float* save_mean; const float* save_invstd; void* dx; int ld_dx; void* dres; int ld_dr;
  float* dweight; float* dbias;
} mm_bn2d_bwd_args;
int mm_bn2d_fwd_train_pair(mm_handle_t h, const mm_bn2d_fwd_args* a, const mm_bn2d_fwd_args* b, int64_t N, int64_t Ns, int C, float eps,
                           float momentum, int relu, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_bn2d_bwd_pair(mm_handle_t h, const mm_bn2d_bwd_args* a, const mm_bn2d_bwd_args* b, int relu, int64_t N, int64_t Ns, int C, int accumulate,
                     void* ws, size_t ws_bytes, mm_stream_t stream);
/* The stems' BatchNorm2d + ReLU + MaxPool2d(3, 2, 1) (EXP/2d_net/backbones.py:43-47) as ONE pass over the map (after the slab reduce +
 * finalize of mm_bn2d_fwd_train_pre): y = the normalised map [B][H][W][C] (pitch ld_y), ypool [B][H/2][W/2][C] its pooled version, idx
 * the winning taps (the outputs of mm_maxpool3x3s2_fwd); H, W even; images [0, Bs) are statistics group 0.  Backward
 * (mm_bn2d_bwd_pool): the gradient arrives as the POOLED map's gradient dyp + idx (gathered per pixel inside the reduce / apply passes,
 * so no full-resolution gradient map is written or read) and optionally a second full-resolution contribution dy2; three launches,
 * no grid barrier, same results as mm_maxpool3x3s2_bwd followed by mm_bn2d_bwd. */
int mm_bn2d_fwd_train_pre_pool(const void* x, int ld_x, int B, int H, int W, int Bs, int C, const float* weight, const float* bias,
                               float* running_mean, float* running_var, int64_t* num_batches_tracked, float eps, float momentum, void* y,
                               int ld_y, void* ypool, void* idx, float* save_mean, float* save_invstd, const float* slab,
                               int64_t slab_rows, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_bn2d_bwd_pool(const void* x, int ld_x, const void* dyp, int ld_dyp, const void* idx, int B, int H, int W, int Bs, const void* dy2,
                     int ld_dy2, int C, const float* weight, const float* bias, const float* save_mean, const float* save_invstd, void* dx,
                     int ld_dx, float* dweight, float* dbias, int accumulate, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_bn2d_fwd_eval(const void* x, int ld_x, const void* res, int ld_r, int64_t N, int C, const float* weight,
                     const float* bias, const float* running_mean, const float* running_var, float eps, int relu, void* y,
                     int ld_y, mm_stream_t stream);
/* yout == NULL with relu != 0 (forward without residual): the ReLU mask is recomputed from x and the saved statistics.
 * dy2 != NULL: the incoming gradient is dy + dy2 (a map with two consumers: residual / concat), summed in the kernel. */
int mm_bn2d_bwd(mm_handle_t h, const void* x, int ld_x, const void* dy, int ld_dy, const void* dy2, int ld_dy2, const void* yout, int ld_y,
                int relu, int64_t N, int64_t Ns, int C, const float* weight, const float* bias, const float* save_mean, const float* save_invstd, void* dx,
                int ld_dx, void* dres, int ld_dr, float* dweight, float* dbias, int accumulate, void* ws, size_t ws_bytes,
                mm_stream_t stream);

/* out[c] (+)= sum_rows x[row][c]: the conv bias gradient, torch's dy.sum((0,2,3)) (2d_net/model.py:68-81 convs with bias).
 * ws >= mm_bn2d_ws_bytes(C). */
int mm_colsum_bf16(const void* x, int ld_x, int64_t N, int C, float* out, int accumulate, void* ws, size_t ws_bytes,
                   mm_stream_t stream);

/* ---------------------------------------------------------------- concat, max-pool, fused heads (csrc/misc2d.hip) */
int mm_copy_rows_bf16(const void* src, int64_t ld_s, void* dst, int64_t ld_d, int64_t N, int C, mm_stream_t stream);
/* torch.cat(parts, dim=1) of NHWC bf16 maps in one launch (decoder concat [depth, up, rgb], 2d_net/model.py:104-123);
 * split != 0 is its backward: parts[i] = channel slice i of wide.  Channel counts multiples of 8, 1..4 parts. */
int mm_concat_bf16(void* const* parts, const int* channels, int nparts, void* wide, int64_t N, int split, mm_stream_t stream);
/* MaxPool2d(3, 2, 1): y and idx dense [B, Ho, Wo, C] (Ho = (H - 1) / 2 + 1), idx = winning tap kh * 3 + kw, the first maximum in scan
 * order over the taps inside the image.  C and the pitches multiples of 8 and >= C, map pointers 16-byte aligned, idx 8-byte
 * aligned: anything else is MM_ERR_ARG before any launch. */
int mm_maxpool3x3s2_fwd(const void* x, int ldx, int B, int H, int W, int C, void* y, void* idx, mm_stream_t stream);
/* dy2 (optional): a second gradient of the pooled map (it had two consumers), summed with dy in fp32; ld_dy / ld_dy2 = pixel pitches */
int mm_maxpool3x3s2_bwd(const void* dy, int ld_dy, const void* dy2, int ld_dy2, const void* idx, int B, int H, int W, int C, void* dx,
                        mm_stream_t stream);
size_t mm_head_ws_bytes(int B, int h, int w, int Hp, int Wp, int C, int NJ);
/* AvgPool2d(5,1,2) + Conv2d 1x1 of both heads (EXP/2d_net/model.py:59-60,129-130,158,163-164): out NHWC fp32 [B,h,w,NJ].
 * x: NHWC [B,Hp,Wp,C] with pixel pitch ld, of which the crop [:h, :w] is read; bias may be NULL.  MM_ERR_ARG before any launch
 * unless h <= Hp, w <= Wp, C <= ld, ld % 8 == 0, x (and dx) 16-byte aligned, NJ <= 32, NJ * C * 4 <= 60 KB (backward: C == 64).
 * mm_head_bwd writes +0 to dx outside the crop. */
int mm_head_fwd(const void* x, int B, int Hp, int Wp, int ld, int h, int w, int C, const float* Wj, const float* bias,
                int NJ, float* out, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_head_bwd(const void* x, int B, int Hp, int Wp, int ld, int h, int w, int C, const float* Wj, int NJ,
                const float* dout, void* dx, float* dWj, void* ws, size_t ws_bytes, mm_stream_t stream);

/* ---------------------------------------------------------------- exact-fp32 2D convolutions (csrc/conv2d_f32.hip)
 * The `precision: 32` mode (config/run/test.yaml:8): plain fp32 FMAs in an LDS-tiled implicit GEMM; one kernel pair
 * expresses Conv2d / ConvTranspose2d forward, data and weight gradients through index maps (file header). */
int mm_conv2d_f32(const float* A, int B, int Hi, int Wi, int Ca, int ldA, float* O, int Ho, int Wo, int Cn, int ldO, int KH, int KW,
                  int so, int sgn, int off, int up, const float* W, int64_t w_sn, int64_t w_sc, int64_t w_sy, int64_t w_sx,
                  const float* bias, mm_stream_t stream);
size_t mm_conv2d_f32_wgrad_ws_bytes(int64_t n_pixels, int Cg, int Ca, int KH, int KW);
int mm_conv2d_f32_wgrad(const float* G, int B, int Hg, int Wg, int Cg, int ldG, const float* A, int Hi, int Wi, int Ca, int ldA,
                        int KH, int KW, int so, int sgn, int off, int up, float* dW, int64_t w_sn, int64_t w_sc, int64_t w_sy,
                        int64_t w_sx, int accumulate, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_colsum_f32(const float* x, int ld, int64_t N, int C, float* out, int accumulate, mm_stream_t stream);


/* ---------------------------------------------------------------- the dense 2D kernels over IEEE fp16 maps
 * The reference's 2D branch runs under ``precision: 16`` = fp16 autocast + GradScaler (config/run/train.yaml:11).  The kernels of
 * csrc/conv2d.hip, bn2d.hip and misc2d.hip are built a second time with IEEE fp16 as the 16-bit storage format
 * (v_mfma_f32_32x32x16_f16 / v_mfma_f32_16x16x32_f16; csrc/h16.h) and exported under the suffix _f16: same arguments, same
 * semantics, "bf16" in the descriptions above reads "fp16".  One handle serves both builds (same option, same fault word).  mm_copy_rows_bf16 / mm_concat_bf16 move 2-byte elements and serve both.
 * Gradient maps in fp16 need the loss scale of mm2d3d_amd/amp.py (mm_grad_nonfinite ... mm_amp_update below). */
int mm_conv2d_gemm_f16(const void* A, int B, int Hi, int Wi, int Ca, int lda, void* O, int Ho, int Wo, int Cn, int ldo,
                   int out_f32, int Hg, int Wg, int so, int ooy, int oox, int sa, int fr, int ntaps, const int* ty,
                   const int* tx, const void* Wp, int nz, int64_t wz, int zpar, const float* bias, float* stats,
                   int64_t split_m, const void* addend, int ld_add, mm_stream_t stream);
int mm_conv2d_dgrad_s2_f16(const void* dY, int B, int Ho, int Wo, int Cout, int ldy, void* dX, int H, int W, int Cin, int ldx, const void* Wd,
                       int k, int pad, const void* addend, int ld_add, mm_stream_t stream);
int64_t mm_conv2d_gemm_stat_rows_f16(int64_t M, int nz);
int64_t mm_conv2d_3x3s1_stat_rows_f16(int B, int H, int W);
int mm_conv2d_3x3s1_f16(const void* A, int B, int H, int W, int Ca, int lda, void* O, int Cn, int ldo, const void* Wp,
                    const float* bias, int flip, float* stats, int split_b, mm_stream_t stream);
int mm_conv2d_3x3s1_pair_f16(const void* A0, const void* A1, int B, int H, int W, int Ca, int lda, void* O0, void* O1, int Cn, int ldo,
                         const void* Wp0, const void* Wp1, int flip, float* stats0, float* stats1, int split_b, mm_stream_t stream);
int mm_conv2d_wgrad3x3_pair_f16(const void* X0, const void* X1, int B, int H, int W, int Ck, int ldx, const void* dY0, const void* dY1, int Cn,
                            int ldy, float* dW0, float* dW1, int64_t sn, int64_t st, int64_t sk, int accumulate, void* ws, size_t ws_bytes,
                            mm_stream_t stream);
size_t mm_conv2d_wgrad_ws_bytes_f16(int64_t M, int Cn, int Ck, int ntaps);
int mm_conv2d_wgrad_f16(const void* X, int B, int Hi, int Wi, int Ck, int ldx, const void* dY, int Hg, int Wg, int Cn,
                    int ldy, int sa, int ntaps, const int* ty, const int* tx, float* dW, int64_t sn, int64_t st,
                    int64_t sk, int accumulate, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_conv2d_wgrad_slabs_f16(const void* X, int B, int Hi, int Wi, int Ck, int ldx, const void* dY, int Hg, int Wg, int Cn, int ldy,
                          int sa, int ntaps, const int* ty, const int* tx, void* slabs, size_t slab_bytes, int* nsplit,
                          mm_stream_t stream);
int mm_conv2d_wgrad3x3_pair_slabs_f16(const void* X0, const void* X1, int B, int H, int W, int Ck, int ldx, const void* dY0, const void* dY1,
                                  int Cn, int ldy, void* slabs, size_t slab_bytes, int* nsplit, mm_stream_t stream);
int mm_conv2d_wgrad_reduce_desc_bytes_f16(void);
int64_t mm_conv2d_wgrad_reduce_blocks_f16(int Cn, int Ck, int pair);
int mm_conv2d_wgrad_reduce_batch_f16(const void* descs_dev, int n, int64_t total_blocks, mm_stream_t stream);
int64_t mm_conv2d_stem7_stat_rows_f16(int B, int H, int W);
int mm_conv2d_stem7_f16(const void* xb, int B, int Hb, int Wb, int H, int W, int R, int T, void* O, int ldo, const void* Wp, float* stats,
                    int split_b, mm_stream_t stream);
int mm_stem_prep_f16(const float* in, int B, int C, int H, int W, int pad, int Hb, int Wb, int R, void* out, mm_stream_t stream);
int mm_pack_weights_f16(const float* in, void* out, int Z, int N, int T, int K, int64_t sz, int64_t sn, int64_t st,
                         int64_t sk, mm_stream_t stream);
int mm_pack_weights_f16_batch(const int64_t* desc, int ndesc, int64_t total_blocks, mm_stream_t stream);
size_t mm_bn2d_ws_bytes_f16(int C);
int mm_bn2d_fwd_train_f16(mm_handle_t h, const void* x, int ld_x, const void* res, int ld_r, int64_t N, int64_t Ns, int C, const float* weight,
                      const float* bias, float* running_mean, float* running_var, int64_t* num_batches_tracked, float eps,
                      float momentum, int relu, void* y, int ld_y, float* save_mean, float* save_invstd, void* ws,
                      size_t ws_bytes, mm_stream_t stream);
int mm_bn2d_single_launch_f16(mm_handle_t h, int64_t N, int64_t Ns, int C, int backward);
int mm_bn2d_fwd_train_pre_f16(const void* x, int ld_x, const void* res, int ld_r, int64_t N, int64_t Ns, int C, const float* weight,
                          const float* bias, float* running_mean, float* running_var, int64_t* num_batches_tracked, float eps,
                          float momentum, int relu, void* y, int ld_y, float* save_mean, float* save_invstd, const float* slab,
                          int64_t slab_rows, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_bn2d_fwd_train_pair_f16(mm_handle_t h, const mm_bn2d_fwd_args* a, const mm_bn2d_fwd_args* b, int64_t N, int64_t Ns, int C, float eps,
                           float momentum, int relu, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_bn2d_bwd_pair_f16(mm_handle_t h, const mm_bn2d_bwd_args* a, const mm_bn2d_bwd_args* b, int relu, int64_t N, int64_t Ns, int C, int accumulate,
                     void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_bn2d_fwd_train_pre_pool_f16(const void* x, int ld_x, int B, int H, int W, int Bs, int C, const float* weight, const float* bias,
                               float* running_mean, float* running_var, int64_t* num_batches_tracked, float eps, float momentum, void* y,
                               int ld_y, void* ypool, void* idx, float* save_mean, float* save_invstd, const float* slab,
                               int64_t slab_rows, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_bn2d_bwd_pool_f16(const void* x, int ld_x, const void* dyp, int ld_dyp, const void* idx, int B, int H, int W, int Bs, const void* dy2,
                     int ld_dy2, int C, const float* weight, const float* bias, const float* save_mean, const float* save_invstd, void* dx,
                     int ld_dx, float* dweight, float* dbias, int accumulate, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_bn2d_fwd_eval_f16(const void* x, int ld_x, const void* res, int ld_r, int64_t N, int C, const float* weight,
                     const float* bias, const float* running_mean, const float* running_var, float eps, int relu, void* y,
                     int ld_y, mm_stream_t stream);
int mm_bn2d_bwd_f16(mm_handle_t h, const void* x, int ld_x, const void* dy, int ld_dy, const void* dy2, int ld_dy2, const void* yout, int ld_y,
                int relu, int64_t N, int64_t Ns, int C, const float* weight, const float* bias, const float* save_mean, const float* save_invstd, void* dx,
                int ld_dx, void* dres, int ld_dr, float* dweight, float* dbias, int accumulate, void* ws, size_t ws_bytes,
                mm_stream_t stream);
int mm_colsum_f16(const void* x, int ld_x, int64_t N, int C, float* out, int accumulate, void* ws, size_t ws_bytes,
                   mm_stream_t stream);
int mm_maxpool3x3s2_fwd_f16(const void* x, int ldx, int B, int H, int W, int C, void* y, void* idx, mm_stream_t stream);
int mm_maxpool3x3s2_bwd_f16(const void* dy, int ld_dy, const void* dy2, int ld_dy2, const void* idx, int B, int H, int W, int C, void* dx,
                        mm_stream_t stream);
size_t mm_head_ws_bytes_f16(int B, int h, int w, int Hp, int Wp, int C, int NJ);
int mm_head_fwd_f16(const void* x, int B, int Hp, int Wp, int ld, int h, int w, int C, const float* Wj, const float* bias,
                int NJ, float* out, void* ws, size_t ws_bytes, mm_stream_t stream);
int mm_head_bwd_f16(const void* x, int B, int Hp, int Wp, int ld, int h, int w, int C, const float* Wj, int NJ,
                const float* dout, void* dx, float* dWj, void* ws, size_t ws_bytes, mm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MM2D3D_H */
