// Row gathers (rows of a batch, rows of an image-feature bank with their dropout) and the fp16 <-> fp32 converters of a
// float16 image-feature cache.  HBM-bound streaming kernels, as in elementwise.hip.
#include <hip/hip_fp16.h>
#include "common.hpp"
#include "cache_load.hpp"

namespace vqa {

// dst[b][0:cols] = src[rows[b]][0:cols], zeros for a row index outside [0, M); VEC: one float4 per thread and iteration
template <bool VEC>
__global__ void gather_rows_kernel(const float* src, int64_t src_ld, const int* rows, float* dst, int64_t dst_ld, int B, int M,
                                   int cols) {
  const int cw = VEC ? cols >> 2 : cols;
  const int64_t n = (int64_t)B * cw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / cw;
    const int c = (int)(i - b * cw);
    const int r = rows[b];
    const bool in = (unsigned)r < (unsigned)M;
    if (VEC) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in) v = reinterpret_cast<const float4*>(src + (int64_t)r * src_ld)[c];
      reinterpret_cast<float4*>(dst + b * dst_ld)[c] = v;
    } else {
      dst[b * dst_ld + c] = in ? src[(int64_t)r * src_ld + c] : 0.f;
    }
  }
}

// dst[j][0:row_len] = src[rows[j]][0:row_len] * drop_scale(seed, rows[j]*row_len + i): rows of a large bank compacted and
// dropped in one pass, the mask indexed by the BANK row (64-bit flat index), zeros for a row index outside [0, M).  Rows are
// long (one image's features), so the flat range n * row_len is spread over a capped grid; a thread divides once and then
// walks (row, column) by the grid stride split on the host into (step_j, step_c) = divmod(stride, width).  VEC: one float4
// per thread and iteration (row_len % 4 == 0, so a row start is a multiple of 4 for drop_scale4).  VT: the bank's element
// type (cache_load.hpp); dst is fp32 either way, and the mask multiplies the widened value.
template <bool VEC, class VT>
__device__ __forceinline__ void gather_rows_drop_body(const VT* src, const int* rows, float* dst, int n, int M, int64_t row_len,
                                                      int64_t step_j, int64_t step_c, float p, float inv_keep, uint64_t seed) {
  const int64_t rw = VEC ? row_len >> 2 : row_len;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t j = first / rw, c = first - j * rw;
  while (j < n) {
    const int r = rows[j];
    const bool in = (unsigned)r < (unsigned)M;
    const int64_t s = (int64_t)r * row_len, d = j * row_len;
    if (VEC) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in) {
        v = load_quad(src + s, c);
        if (p > 0.f) {
          const float4 ds_ = drop_scale4(seed, (uint64_t)(s + 4 * c), p, inv_keep);
          v.x *= ds_.x; v.y *= ds_.y; v.z *= ds_.z; v.w *= ds_.w;
        }
      }
      reinterpret_cast<float4*>(dst + d)[c] = v;
    } else {
      float v = 0.f;
      if (in) {
        v = load_one(src, s + c);
        if (p > 0.f) v *= drop_scale(seed, (uint64_t)(s + c), p, inv_keep);
      }
      dst[d + c] = v;
    }
    j += step_j;
    c += step_c;
    if (c >= rw) { c -= rw; ++j; }
  }
}

template <bool VEC, class VT = float>
__global__ void gather_rows_drop_kernel(const VT* src, const int* rows, float* dst, int n, int M, int64_t row_len,
                                        int64_t step_j, int64_t step_c, float p, float inv_keep, uint64_t seed) {
  gather_rows_drop_body<VEC>(src, rows, dst, n, M, row_len, step_j, step_c, p, inv_keep, seed);
}

// Image dropout on rows of a bank of L2-normalised features: for feature row (j, pos) of the n * P asked
// ones, u = src[rows[j]][pos][:] * drop_scale(seed, bank index), vn_out = u / (|u| + 1e-12) -- the operations of
// l2norm_fwd_kernel (elementwise.hip) on a gathered row, the mask indexed by the BANK row (64-bit) -- and, where vdrop_out
// is given, vdrop_out = vn_out * drop_scale(seed2, bank index).  One wave per feature row of C floats; zeros in both
// outputs for a row index outside [0, M).  REG: C <= 256, a lane keeps its quad in registers and a wave has four feature
// rows in flight (one pass over memory); otherwise the general form reads a row twice.  VT: the bank's element type.
template <bool REG, class VT>
__global__ void gather_rows_drop_norm_kernel(const VT* src, const int* rows, float* vn_out, float* vdrop_out, int n, int M, int P,
                                             int C, float p, float inv_keep, uint64_t seed, float p2, float inv_keep2,
                                             uint64_t seed2) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int nch = C >> 2;
  const int64_t frows = (int64_t)n * P;            // feature rows of the output
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (REG) {
    constexpr int R = 4;
    const int c = lane;
    const bool cok = c < nch;
    for (int64_t f0 = R * wave; f0 < frows; f0 += R * nwaves) {
      float4 u[R];
      int64_t s[R];                                // first element of the bank's feature row, -1: nothing to read
      int64_t j = f0 / P;                          // one division a group: (j, pos) then walks the R consecutive rows
      int pos = (int)(f0 - j * P);
#pragma unroll
      for (int k = 0; k < R; ++k) {
        s[k] = -1;
        if (f0 + k < frows) {
          const int r = rows[j];
          if ((unsigned)r < (unsigned)M) s[k] = ((int64_t)r * P + pos) * C;
        }
        u[k] = (cok && s[k] >= 0) ? load_quad(src + s[k], c) : zero4;
        if (++pos == P) { pos = 0; ++j; }
      }
      float ss[R];
#pragma unroll
      for (int k = 0; k < R; ++k) {
        if (p > 0.f && s[k] >= 0) {
          const float4 ds_ = drop_scale4(seed, (uint64_t)(s[k] + 4 * c), p, inv_keep);
          u[k].x *= ds_.x; u[k].y *= ds_.y; u[k].z *= ds_.z; u[k].w *= ds_.w;
        }
        ss[k] = 0.f;
        ss[k] += u[k].x * u[k].x + u[k].y * u[k].y + u[k].z * u[k].z + u[k].w * u[k].w;
      }
#pragma unroll
      for (int k = 0; k < R; ++k) ss[k] = wave_sum(ss[k]);
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int64_t f = f0 + k;
        if (f >= frows) break;
        if (!cok) continue;
        const float inv = 1.0f / (sqrtf(ss[k]) + 1e-12f);
        const float4 o = make_float4(u[k].x * inv, u[k].y * inv, u[k].z * inv, u[k].w * inv);
        reinterpret_cast<float4*>(vn_out + f * C)[c] = o;
        if (vdrop_out) {
          float4 d = o;
          if (p2 > 0.f && s[k] >= 0) {
            const float4 ds_ = drop_scale4(seed2, (uint64_t)(s[k] + 4 * c), p2, inv_keep2);
            d.x *= ds_.x; d.y *= ds_.y; d.z *= ds_.z; d.w *= ds_.w;
          }
          reinterpret_cast<float4*>(vdrop_out + f * C)[c] = d;
        }
      }
    }
    return;
  }
  for (int64_t f = wave; f < frows; f += nwaves) {
    const int64_t j = f / P;
    const int r = rows[j];
    float4* dst = reinterpret_cast<float4*>(vn_out + f * C);
    float4* dst2 = vdrop_out ? reinterpret_cast<float4*>(vdrop_out + f * C) : nullptr;
    if ((unsigned)r >= (unsigned)M) {              // wave-uniform
      for (int c = lane; c < nch; c += 64) {
        dst[c] = zero4;
        if (dst2) dst2[c] = zero4;
      }
      continue;
    }
    const int64_t s = ((int64_t)r * P + (f - j * P)) * C;
    float ss = 0.f;
    for (int c = lane; c < nch; c += 64) {
      float4 u = load_quad(src + s, c);
      if (p > 0.f) {
        const float4 ds_ = drop_scale4(seed, (uint64_t)(s + 4 * c), p, inv_keep);
        u.x *= ds_.x; u.y *= ds_.y; u.z *= ds_.z; u.w *= ds_.w;
      }
      ss += u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w;
    }
    ss = wave_sum(ss);
    const float inv = 1.0f / (sqrtf(ss) + 1e-12f);
    for (int c = lane; c < nch; c += 64) {
      float4 u = load_quad(src + s, c);
      if (p > 0.f) {
        const float4 ds_ = drop_scale4(seed, (uint64_t)(s + 4 * c), p, inv_keep);
        u.x *= ds_.x; u.y *= ds_.y; u.z *= ds_.z; u.w *= ds_.w;
      }
      const float4 o = make_float4(u.x * inv, u.y * inv, u.z * inv, u.w * inv);
      dst[c] = o;
      if (dst2) {
        float4 d = o;
        if (p2 > 0.f) {
          const float4 ds_ = drop_scale4(seed2, (uint64_t)(s + 4 * c), p2, inv_keep2);
          d.x *= ds_.x; d.y *= ds_.y; d.z *= ds_.z; d.w *= ds_.w;
        }
        dst2[c] = d;
      }
    }
  }
}

// fp16 -> fp32, 8 values (16 bytes in, 32 bytes out) per thread and iteration
__global__ void half_to_float_kernel(const __half* x, float* y, int64_t n) {
  const int64_t n8 = n / 8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const uint4 raw = reinterpret_cast<const uint4*>(x)[i];
    const __half2* h = reinterpret_cast<const __half2*>(&raw);
    const float2 a = __half22float2(h[0]), b = __half22float2(h[1]), c = __half22float2(h[2]), d = __half22float2(h[3]);
    reinterpret_cast<float4*>(y)[2 * i] = make_float4(a.x, a.y, b.x, b.y);
    reinterpret_cast<float4*>(y)[2 * i + 1] = make_float4(c.x, c.y, d.x, d.y);
  }
  if (blockIdx.x == 0 && threadIdx.x < n - 8 * n8) y[8 * n8 + threadIdx.x] = __half2float(x[8 * n8 + threadIdx.x]);
}

// fp32 -> fp16, round to nearest even (v_cvt_f16_f32: overflow to +-inf, NaN stays NaN, subnormal results kept): the mirror
// of half_to_float_kernel, 8 values (32 bytes in, 16 bytes out) per thread and iteration
__global__ void float_to_half_kernel(const float* x, __half* y, int64_t n) {
  const int64_t n8 = n / 8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 a = reinterpret_cast<const float4*>(x)[2 * i], b = reinterpret_cast<const float4*>(x)[2 * i + 1];
    uint4 raw;
    __half2* h = reinterpret_cast<__half2*>(&raw);
    h[0] = __halves2half2(__float2half(a.x), __float2half(a.y));
    h[1] = __halves2half2(__float2half(a.z), __float2half(a.w));
    h[2] = __halves2half2(__float2half(b.x), __float2half(b.y));
    h[3] = __halves2half2(__float2half(b.z), __float2half(b.w));
    reinterpret_cast<uint4*>(y)[i] = raw;
  }
  if (blockIdx.x == 0 && threadIdx.x < n - 8 * n8) y[8 * n8 + threadIdx.x] = __float2half(x[8 * n8 + threadIdx.x]);
}

}  // namespace vqa

using namespace vqa;

#define STREAM ((hipStream_t)stream)

// vqa_gather_rows_drop and vqa_gather_rows_drop_f16 (`who` names the entry point in the messages).  The quad kernel loads a
// quad of the bank (16 bytes of fp32, 8 of fp16) and stores 16 bytes; anything else runs the scalar one.  A float16 bank
// is required to be element-aligned, and dst with it; the fp32 form never asked.
template <class VT>
static int gather_rows_drop(const char* who, const VT* src, const int32_t* rows, float* dst, int n, int M, int64_t row_len, float p,
                            uint64_t seed, hipStream_t s) {
  const uintptr_t sb = ptr_bits(src), db = ptr_bits(dst);
  VQA_REQUIRE(src && rows && dst, "%s: null pointer", who);
  VQA_REQUIRE(n >= 0 && M >= 1 && row_len >= 1, "%s: n=%d, M=%d, row_len=%lld out of range", who, n, M, (long long)row_len);
  VQA_REQUIRE(p >= 0.f && p < 1.f, "%s: p=%g outside [0, 1)", who, (double)p);
  if constexpr (std::is_same<VT, __half>::value)
    VQA_REQUIRE((sb & 1) == 0 && (db & 3) == 0, "%s: src must be 2-byte and dst 4-byte aligned", who);
  if (n == 0) return VQA_OK;
  const bool vec = row_len % 4 == 0 && (sb & (kQuadAlign<VT> - 1)) == 0 && (db & 15) == 0;
  const int64_t rw = vec ? row_len / 4 : row_len;
  const int grid = grid_for((int64_t)n * rw, 256);
  const int64_t stride = (int64_t)grid * 256;
  return with_flag(vec, [&](auto v) {
    hipLaunchKernelGGL((gather_rows_drop_kernel<decltype(v)::value, VT>), dim3(grid), dim3(256), 0, s, src, rows, dst, n, M, row_len,
                       stride / rw, stride % rw, p, keep_scale(p), seed);
    return check_hip(hipGetLastError(), "gather_rows_drop launch");
  });
}

// vqa_gather_rows_drop_norm and vqa_gather_rows_drop_norm_f16.  Quads only (there is no scalar kernel): every check is made
// here, before any HIP call.  One wave per feature row, four waves a workgroup; the register form takes four rows a wave.
template <class VT>
static int gather_rows_drop_norm(const char* who, const VT* src, const int32_t* rows, float* vn_out, float* vdrop_out, int n, int M,
                                 int P, int C, float p, uint64_t seed, float p2, uint64_t seed2, hipStream_t s) {
  VQA_REQUIRE(src && rows && vn_out, "%s: null pointer", who);
  VQA_REQUIRE(n >= 0 && M >= 1 && P >= 1, "%s: n=%d, M=%d, P=%d out of range", who, n, M, P);
  VQA_REQUIRE(C >= 4 && C % 4 == 0, "%s: C=%d must be a positive multiple of 4", who, C);
  VQA_REQUIRE(p >= 0.f && p < 1.f, "%s: p=%g outside [0, 1)", who, (double)p);
  VQA_REQUIRE(!vdrop_out || (p2 >= 0.f && p2 < 1.f), "%s: p2=%g outside [0, 1)", who, (double)p2);
  VQA_REQUIRE((ptr_bits(src) & (kQuadAlign<VT> - 1)) == 0, "%s: src must be %d-byte aligned", who, (int)kQuadAlign<VT>);
  VQA_REQUIRE((ptr_bits(vn_out, vdrop_out) & 15) == 0, "%s: vn_out and vdrop_out must be 16-byte aligned", who);
  if (n == 0) return VQA_OK;
  if (!vdrop_out) { p2 = 0.f; seed2 = 0; }
  const bool reg = C <= 256;
  const int grid = grid_for((int64_t)n * P, reg ? 16 : 4);
  return with_flag(reg, [&](auto r) {
    hipLaunchKernelGGL((gather_rows_drop_norm_kernel<decltype(r)::value, VT>), dim3(grid), dim3(256), 0, s, src, rows, vn_out,
                       vdrop_out, n, M, P, C, p, keep_scale(p), seed, p2, keep_scale(p2), seed2);
    return check_hip(hipGetLastError(), "gather_rows_drop_norm launch");
  });
}

extern "C" {

int vqa_gather_rows(const float* src, int64_t src_ld, const int32_t* rows, float* dst, int64_t dst_ld, int B, int M, int cols,
                    vqa_stream_t stream) {
  VQA_REQUIRE(src && rows && dst, "vqa_gather_rows: null pointer");
  VQA_REQUIRE(B >= 0 && M >= 1 && cols >= 1, "vqa_gather_rows: B=%d, M=%d, cols=%d out of range", B, M, cols);
  VQA_REQUIRE(src_ld >= cols && dst_ld >= cols, "vqa_gather_rows: src_ld=%lld and dst_ld=%lld must be >= cols=%d",
              (long long)src_ld, (long long)dst_ld, cols);
  if (B == 0) return VQA_OK;
  const bool vec = cols % 4 == 0 && src_ld % 4 == 0 && dst_ld % 4 == 0 && (ptr_bits(src, dst) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(gather_rows_kernel<true>, dim3(grid_for((int64_t)B * (cols / 4), 256)), dim3(256), 0, STREAM, src, src_ld,
                       rows, dst, dst_ld, B, M, cols);
  else
    hipLaunchKernelGGL(gather_rows_kernel<false>, dim3(grid_for((int64_t)B * cols, 256)), dim3(256), 0, STREAM, src, src_ld, rows,
                       dst, dst_ld, B, M, cols);
  return check_hip(hipGetLastError(), "gather_rows launch");
}

int vqa_gather_rows_drop(const float* src, const int32_t* rows, float* dst, int n, int M, int64_t row_len, float p,
                         uint64_t seed, vqa_stream_t stream) {
  return gather_rows_drop("vqa_gather_rows_drop", src, rows, dst, n, M, row_len, p, seed, STREAM);
}

int vqa_half_to_float(const void* x_f16, float* y, int64_t n, vqa_stream_t stream) {
  VQA_REQUIRE(x_f16 && y && n > 0, "vqa_half_to_float: bad args");
  VQA_REQUIRE((ptr_bits(x_f16, y) & 15) == 0, "vqa_half_to_float: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(half_to_float_kernel, dim3(grid_for(n / 8 + 1, 256)), dim3(256), 0, STREAM,
                     static_cast<const __half*>(x_f16), y, n);
  return check_hip(hipGetLastError(), "half_to_float launch");
}

// ---- float16 image-feature caches: the converter and the cache readers of this file on a half operand
int vqa_float_to_half(const float* x, void* y_f16, int64_t n, vqa_stream_t stream) {
  VQA_REQUIRE(x && y_f16 && n >= 0, "vqa_float_to_half: bad args");
  VQA_REQUIRE((ptr_bits(x, y_f16) & 15) == 0, "vqa_float_to_half: pointers must be 16-byte aligned");
  if (n == 0) return VQA_OK;
  hipLaunchKernelGGL(float_to_half_kernel, dim3(grid_for(n / 8 + 1, 256)), dim3(256), 0, STREAM, x, static_cast<__half*>(y_f16), n);
  return check_hip(hipGetLastError(), "float_to_half launch");
}

int vqa_gather_rows_drop_f16(const void* src_f16, const int32_t* rows, float* dst, int n, int M, int64_t row_len, float p,
                             uint64_t seed, vqa_stream_t stream) {
  return gather_rows_drop("vqa_gather_rows_drop_f16", static_cast<const __half*>(src_f16), rows, dst, n, M, row_len, p, seed, STREAM);
}

// ---- image dropout on a bank of normalised features
int vqa_gather_rows_drop_norm(const float* src, const int32_t* rows, float* vn_out, float* vdrop_out, int n, int M, int P, int C,
                              float p, uint64_t seed, float p2, uint64_t seed2, vqa_stream_t stream) {
  return gather_rows_drop_norm("vqa_gather_rows_drop_norm", src, rows, vn_out, vdrop_out, n, M, P, C, p, seed, p2, seed2, STREAM);
}

int vqa_gather_rows_drop_norm_f16(const void* src_f16, const int32_t* rows, float* vn_out, float* vdrop_out, int n, int M, int P,
                                  int C, float p, uint64_t seed, float p2, uint64_t seed2, vqa_stream_t stream) {
  return gather_rows_drop_norm("vqa_gather_rows_drop_norm_f16", static_cast<const __half*>(src_f16), rows, vn_out, vdrop_out, n, M,
                               P, C, p, seed, p2, seed2, STREAM);
}

}  // extern "C"
