// Raw RGB bytes -> the image tensor [N,3,S,S] in ONE launch (vqa_preprocess_images; dl_vqa_amd.preprocess_images): PIL's
// antialiased bilinear resize of the short side, the centre crop, ToTensor, Normalize and the fp16 cast of the reference's
// preprocessing/preprocess_images.py, bit for bit.  The semantics are stated in include/vqa_hip.h; this file holds the
// kernel and the host checks in front of it.
//
// grid = (bands, N): workgroup (b, n) owns output rows [b*BH, b*BH + BH) of image n.
//   pass 1 (horizontal): for the source rows y0 .. y1 that band's vertical taps read, every output column of the crop window
//           -> LDS tile uint8 [y1 - y0][S][3].  Lanes run along x, so a wave reads one contiguous run of one source row
//           (64 * scale * 3 bytes per tap step; neighbouring lanes' taps overlap and are served by the vector cache).
//   pass 2 (vertical): out of LDS; the result byte indexes the 3 x 256 table of the float tail (LDS copy), and the three
//           channel planes are stored with lanes along x.
// Integer arithmetic only: a sum is at most 255 * (2^22 + taps) + 2^21 < 2^31.  Loop bounds depend on the tables alone; a
// pixel value never decides a branch (the clip is min/max).
//
// The host checks every table entry against the image before the launch (pre_check), so no lo + len passes the end of a
// row or column and no band needs more rows than the tile holds; the kernel clamps its row count to the tile all the same.
#include "common.hpp"

namespace vqa {

constexpr int kPreThreads = 256;
constexpr int kPreTileMax = 56 * 1024;        // LDS tile bytes at most: with the table, two workgroups per CU
constexpr int kPreBandMax = 16;               // output rows per workgroup at most

template <class T>   // the output element as raw bits: uint16_t (fp16) or uint32_t (fp32)
__global__ __launch_bounds__(kPreThreads) void preprocess_kernel(const uint8_t* __restrict__ src,
                                                                 const vqa_pre_image_t* __restrict__ images,
                                                                 const int32_t* __restrict__ coef, const T* __restrict__ lut,
                                                                 T* __restrict__ out, int S, int BH, int tile_rows) {
  extern __shared__ __align__(16) uint8_t tile[];       // [rows][S][3]
  __shared__ T lut_s[3 * 256];
  const int tid = threadIdx.x;
  const vqa_pre_image_t d = images[blockIdx.y];
  const int r0 = blockIdx.x * BH, r1 = min(S, r0 + BH);
  const int32_t* hlo = coef + d.h_off;
  const int32_t* hlen = hlo + S;
  const int32_t* hk = hlen + S;
  const int32_t* vlo = coef + d.v_off;
  const int32_t* vlen = vlo + S;
  const int32_t* vk = vlen + S;
  for (int i = tid; i < 3 * 256; i += kPreThreads) lut_s[i] = lut[i];

  int y0 = vlo[r0], y1 = y0;
  for (int r = r0; r < r1; ++r) {
    const int lo = vlo[r];
    y0 = min(y0, lo);
    y1 = max(y1, lo + vlen[r]);
  }
  const int nrows = min(y1 - y0, tile_rows);

  // ---- pass 1: source rows y0 .. y0 + nrows, window columns -> tile
  const uint8_t* base = src + d.src_offset + (int64_t)y0 * d.pitch;
  for (int idx = tid; idx < nrows * S; idx += kPreThreads) {
    const int row = idx / S, x = idx - row * S;
    const int len = hlen[x];
    const int32_t* k = hk + (int64_t)x * d.h_taps;
    const uint8_t* p = base + (int64_t)row * d.pitch + (int64_t)hlo[x] * 3;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int j = 0; j < len; ++j) {
      const int kj = k[j];
      a0 += (int)p[3 * j] * kj;
      a1 += (int)p[3 * j + 1] * kj;
      a2 += (int)p[3 * j + 2] * kj;
    }
    uint8_t* t = tile + (size_t)idx * 3;
    t[0] = (uint8_t)min(max(a0 >> 22, 0), 255);
    t[1] = (uint8_t)min(max(a1 >> 22, 0), 255);
    t[2] = (uint8_t)min(max(a2 >> 22, 0), 255);
  }
  __syncthreads();

  // ---- pass 2: tile -> output rows r0 .. r1, the float tail by table
  const int64_t plane = (int64_t)S * S;
  T* o = out + (int64_t)blockIdx.y * 3 * plane;
  for (int idx = tid; idx < (r1 - r0) * S; idx += kPreThreads) {
    const int rr = idx / S, x = idx - rr * S, r = r0 + rr;
    const int lo = min(max(vlo[r] - y0, 0), nrows - 1);
    const int len = min(vlen[r], nrows - lo);
    const int32_t* k = vk + (int64_t)r * d.v_taps;
    const uint8_t* t = tile + ((size_t)lo * S + x) * 3;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int j = 0; j < len; ++j) {
      const int kj = k[j];
      a0 += (int)t[0] * kj;
      a1 += (int)t[1] * kj;
      a2 += (int)t[2] * kj;
      t += (size_t)S * 3;
    }
    const int64_t at = (int64_t)r * S + x;
    o[at] = lut_s[min(max(a0 >> 22, 0), 255)];
    o[plane + at] = lut_s[256 + min(max(a1 >> 22, 0), 255)];
    o[2 * plane + at] = lut_s[512 + min(max(a2 >> 22, 0), 255)];
  }
}

// One axis table against its axis: n input samples, m resized samples, window start .. start + S.  0 = fine.
static int pre_check_table(const int32_t* coef, int64_t coef_len, int off, int taps, int n, int S, const char* axis, int img) {
  VQA_REQUIRE(taps >= 1 && off >= 0 && (int64_t)off + (int64_t)S * (2 + (int64_t)taps) <= coef_len,
              "preprocess: image %d: %s table (offset %d, %d taps) outside coef[%lld]", img, axis, off, taps, (long long)coef_len);
  const int32_t* lo = coef + off;
  const int32_t* len = lo + S;
  for (int i = 0; i < S; ++i)
    VQA_REQUIRE(lo[i] >= 0 && len[i] >= 1 && len[i] <= taps && (int64_t)lo[i] + len[i] <= n,
                "preprocess: image %d: %s table entry %d (lo %d, len %d) outside [0, %d) or the %d taps", img, axis, i, lo[i],
                len[i], n, taps);
  return VQA_OK;
}

// Source rows the widest band of BH output rows reads.
static int pre_band_rows(const int32_t* vlo, const int32_t* vlen, int S, int BH) {
  int worst = 0;
  for (int r0 = 0; r0 < S; r0 += BH) {
    int y0 = vlo[r0], y1 = y0;
    for (int r = r0; r < S && r < r0 + BH; ++r) {
      y0 = vlo[r] < y0 ? vlo[r] : y0;
      y1 = vlo[r] + vlen[r] > y1 ? vlo[r] + vlen[r] : y1;
    }
    worst = y1 - y0 > worst ? y1 - y0 : worst;
  }
  return worst;
}

// Every check that needs no device; on success *band and *tile_rows are the launch's band height and LDS tile rows.
static int pre_plan(const vqa_pre_image_t* images, const int32_t* coef, int64_t coef_len, int N, int S, int* band, int* tile_rows) {
  VQA_REQUIRE(N >= 0 && S >= 1, "preprocess: N=%d, S=%d out of range (N >= 0, S >= 1)", N, S);
  VQA_REQUIRE(S <= 4096, "preprocess: S=%d not covered (S <= 4096)", S);
  *band = kPreBandMax;
  *tile_rows = 1;
  if (N == 0) return VQA_OK;
  VQA_REQUIRE(images && coef && coef_len > 0, "preprocess: null pointer (images and coef are required)");
  int rows[5] = {0, 0, 0, 0, 0};              // worst band of 16, 8, 4, 2, 1 output rows
  for (int i = 0; i < N; ++i) {
    const vqa_pre_image_t& d = images[i];
    VQA_REQUIRE(d.H >= 1 && d.W >= 1, "preprocess: image %d: H=%d, W=%d", i, d.H, d.W);
    VQA_REQUIRE(d.oh >= S && d.ow >= S, "preprocess: image %d: resized to %d x %d, a side smaller than S=%d (no padding)", i, d.oh,
                d.ow, S);
    VQA_REQUIRE(d.top >= 0 && d.left >= 0 && d.top <= d.oh - S && d.left <= d.ow - S,
                "preprocess: image %d: crop origin (%d, %d) outside the resized %d x %d image", i, d.top, d.left, d.oh, d.ow);
    if (i > 0 && d.h_off == images[i - 1].h_off && d.v_off == images[i - 1].v_off && d.h_taps == images[i - 1].h_taps &&
        d.v_taps == images[i - 1].v_taps && d.H == images[i - 1].H && d.W == images[i - 1].W)
      continue;                               // the tables of the image before: checked already
    int rc = pre_check_table(coef, coef_len, d.h_off, d.h_taps, d.W, S, "horizontal", i);
    if (rc) return rc;
    rc = pre_check_table(coef, coef_len, d.v_off, d.v_taps, d.H, S, "vertical", i);
    if (rc) return rc;
    for (int b = 0; b < 5; ++b) {
      const int n = pre_band_rows(coef + d.v_off, coef + d.v_off + S, S, kPreBandMax >> b);
      rows[b] = n > rows[b] ? n : rows[b];
    }
  }
  for (int b = 0; b < 5; ++b)
    if ((int64_t)rows[b] * S * 3 <= kPreTileMax) {
      *band = kPreBandMax >> b;
      *tile_rows = rows[b];
      return VQA_OK;
    }
  set_error("preprocess: not covered: one output row of S=%d reads %d source rows, %lld bytes of LDS tile (limit %d)", S, rows[4],
            (long long)rows[4] * S * 3, kPreTileMax);
  return VQA_ERR_INVALID;
}

}  // namespace vqa

using namespace vqa;

extern "C" {

int vqa_preprocess_supported(const vqa_pre_image_t* images, const int32_t* coef, int64_t coef_len, int N, int S) {
  int band = 0, tile_rows = 0;
  return pre_plan(images, coef, coef_len, N, S, &band, &tile_rows) == VQA_OK ? band : 0;
}

int vqa_preprocess_images(const uint8_t* src, int64_t src_bytes, const vqa_pre_image_t* images_host, const int32_t* coef_host,
                          int64_t coef_len, const vqa_pre_image_t* images_dev, const int32_t* coef_dev, int N, int S,
                          const void* lut, int out_is_f32, void* out, vqa_stream_t stream) {
  int band = 0, tile_rows = 0;
  const int rc = pre_plan(images_host, coef_host, coef_len, N, S, &band, &tile_rows);
  if (rc) return rc;
  if (N == 0) return VQA_OK;
  VQA_REQUIRE(src && images_dev && coef_dev && lut && out,
              "vqa_preprocess_images: null pointer (src, images_dev, coef_dev, lut and out are required)");
  VQA_REQUIRE(N <= 65535, "vqa_preprocess_images: N=%d images in one launch (at most 65535)", N);
  for (int i = 0; i < N; ++i) {
    const vqa_pre_image_t& d = images_host[i];
    VQA_REQUIRE(d.pitch >= 3 * (int64_t)d.W && d.src_offset >= 0 && d.src_offset <= src_bytes &&
                    (int64_t)(d.H - 1) * d.pitch + 3 * (int64_t)d.W <= src_bytes - d.src_offset,
                "vqa_preprocess_images: image %d (%d x %d, pitch %lld, offset %lld) outside the %lld source bytes", i, d.H, d.W,
                (long long)d.pitch, (long long)d.src_offset, (long long)src_bytes);
  }
  const int lds = (tile_rows * S * 3 + 15) / 16 * 16;
  const dim3 grid((unsigned)((S + band - 1) / band), (unsigned)N);
  const hipStream_t s = (hipStream_t)stream;
  if (out_is_f32) {
    const int r = set_smem(preprocess_kernel<uint32_t>, kPreTileMax, "preprocess_kernel<f32> LDS");
    if (r) return r;
    hipLaunchKernelGGL(preprocess_kernel<uint32_t>, grid, dim3(kPreThreads), lds, s, src, images_dev, coef_dev,
                       static_cast<const uint32_t*>(lut), static_cast<uint32_t*>(out), S, band, tile_rows);
  } else {
    const int r = set_smem(preprocess_kernel<uint16_t>, kPreTileMax, "preprocess_kernel<f16> LDS");
    if (r) return r;
    hipLaunchKernelGGL(preprocess_kernel<uint16_t>, grid, dim3(kPreThreads), lds, s, src, images_dev, coef_dev,
                       static_cast<const uint16_t*>(lut), static_cast<uint16_t*>(out), S, band, tile_rows);
  }
  return check_hip(hipGetLastError(), "preprocess launch");
}

}  // extern "C"
