// bf16 path (BASELINE configs[3]): plain GEMMs on v_mfma_f32_32x32x16_bf16 and the fp32 <-> bf16 converters.
//
// Reference ops re-typed here: nn.Linear / 1x1 nn.Conv2d contractions (models/model.py:173-174,178,202,205) with bf16
// operands and fp32 accumulation; parameters stay fp32 (master copy, Adam), a bf16 copy is made per step.
// The convolution kernels of the bf16 path live in conv.hip (conv_bf16.inc).
#include "bf16_core.hpp"
#include "gemm_host.hpp"

namespace vqa {

using CfgB128 = TileCfg<128, 128, 2, 2>;
using CfgB64 = TileCfg<64, 64, 2, 2>;
// 128 x 256: a weight-gradient product whose output is only 256 columns wide (v_conv dW: [mid] x [C = 256], K = B * positions) --
// with two 128-column tiles the reduction-major A operand (dx', 3 GB) was fetched 1.7x (PMC); one tile spans all columns
using CfgB128x256 = TileCfg<128, 256, 2, 2>;

template <class Cfg, class AL, class BL>
__global__ __launch_bounds__(Cfg::THREADS, Cfg::MIN_WAVES) void gemm_bf16_kernel(typename AL::Params pa,
                                                                              typename BL::Params pb, EpiParams pe,
                                                                              int tiles_m, int tiles_n, int nk,
                                                                              int ks_per_split, int order, int splits) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / Cfg::WAVES_N, wn = wave % Cfg::WAVES_N;
  const TileCoord tc = tile_coord(tiles_m, tiles_n, order, splits);
  const int m0 = tc.mt * Cfg::BM, n0 = tc.nt * Cfg::BN;
  const int ks0 = tc.split * ks_per_split;
  const int ks1 = min(nk, ks0 + ks_per_split);
  f32x16 acc[Cfg::TM][Cfg::TN];
  acc_zero<Cfg>(acc);
  if (!gemm_mainloop_b<Cfg, AL, BL>(
          [&](AL& al, BL& bl) {
            al.init(pa, m0, loader_tid<Cfg>(), ks0);
            bl.init(pb, n0, loader_tid<Cfg>(), ks0);
          },
          acc, ks0, ks1, smem))
    return;
  float* slab = pe.slab ? pe.slab + (int64_t)tc.split * pe.M * pe.N : nullptr;
  if (slab) {
    store_acc_tiles<Cfg>(acc, slab, pe.N, pe.M, pe.N, m0, n0, wm, wn, lane);
    return;
  }
  if constexpr (Cfg::WN == 64) {
    // bf16 output of an interior tile, no aux / accumulate, row groups at least a tile tall: 16-byte stores through LDS
    const bool staged = pe.Cb != nullptr && !pe.aux && !pe.accumulate && (!pe.rg || pe.rg_div >= Cfg::BM) &&
                        m0 + Cfg::BM <= pe.M && n0 + Cfg::BN <= pe.N && (pe.ldc & 7) == 0 &&
                        (reinterpret_cast<uintptr_t>(pe.Cb) & 15) == 0;
    if (staged) return gemm_epilogue_bf16_staged<Cfg>(pe, acc, m0, n0, wm, wn, lane, smem);
  }
  gemm_epilogue<Cfg>(pe, acc, m0, n0, wm, wn, lane);
}

template <class Cfg, class AL, class BL>
static int launch_gemm_bf16(const typename AL::Params& pa, const typename BL::Params& pb, const EpiParams& pe,
                            const GemmPlan& p, hipStream_t s) {
  using SL = SmemLayoutB<Cfg, AL::kTypeR, BL::kTypeR>;
  auto kern = gemm_bf16_kernel<Cfg, AL, BL>;
  int rc = ensure_dyn_smem(reinterpret_cast<const void*>(kern), SL::BYTES, "hipFuncSetAttribute(gemm_bf16)");
  if (rc) return rc;
  hipLaunchKernelGGL(kern, dim3(p.tiles_m * p.tiles_n * p.splits), dim3(Cfg::THREADS), SL::BYTES, s, pa, pb, pe,
                     p.tiles_m, p.tiles_n, p.nk, p.ks_per_split, p.order, p.splits);
  return check_hip(hipGetLastError(), "gemm_bf16_kernel launch");
}

// a k-contiguous operand (type R) is addressed as packed pairs of bf16, a reduction-major one (type C) element by element
template <class L>
static typename L::Params operand_bf16(const void* p, int64_t ld, int rows, int K) {
  if constexpr (L::kTypeR) return {static_cast<const float*>(p), ld / 2, rows, K / 2};
  else return {p, ld, rows, K};
}

template <class Cfg>
static int dispatch_gemm_bf16(const void* A, int64_t lda, int transA, const void* B, int64_t ldb, int transB,
                              const EpiParams& pe, const GemmPlan& p, int M, int N, int K, hipStream_t s) {
  return with_layout<PlainR<Cfg::NVA, Cfg::LT>, PlainCb<Cfg::BM, Cfg::LT>, PlainR<Cfg::NVB, Cfg::LT>, PlainCb<Cfg::BN, Cfg::LT>>(
      transA, transB, [&](auto al, auto bl) {
        using AL = typename decltype(al)::type;
        using BL = typename decltype(bl)::type;
        return launch_gemm_bf16<Cfg, AL, BL>(operand_bf16<AL>(A, lda, M, K), operand_bf16<BL>(B, ldb, N, K), pe, p, s);
      });
}

// ------------------------------------------------------------------ converters
// y[i] = bf16(x[i]); 8 values per thread and iteration (32 bytes in, 16 bytes out)
__global__ void f32_to_bf16_kernel(const float* x, uint16_t* y, int64_t n) {
  const int64_t n8 = n / 8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 a = reinterpret_cast<const float4*>(x)[2 * i], b = reinterpret_cast<const float4*>(x)[2 * i + 1];
    uint4 o;
    o.x = pack_bf16x2(a.x, a.y); o.y = pack_bf16x2(a.z, a.w); o.z = pack_bf16x2(b.x, b.y); o.w = pack_bf16x2(b.z, b.w);
    reinterpret_cast<uint4*>(y)[i] = o;
  }
  if (blockIdx.x == 0 && threadIdx.x < n - 8 * n8) y[8 * n8 + threadIdx.x] = bf16_bits(x[8 * n8 + threadIdx.x]);
}
// y = bf16(x * keep(seed, i) / (1 - p)); same counter hash and index convention as vqa_dropout
__global__ void dropout_to_bf16_kernel(const float* x, uint16_t* y, int64_t n, float p, float inv_keep, uint64_t seed) {
  const int64_t n8 = n / 8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 a = reinterpret_cast<const float4*>(x)[2 * i], b = reinterpret_cast<const float4*>(x)[2 * i + 1];
    float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    if (p > 0.f) {
#pragma unroll
      for (int k = 0; k < 8; k += 4) {
        const float4 ds_ = drop_scale4(seed, (uint64_t)(8 * i + k), p, inv_keep);
        v[k] *= ds_.x; v[k + 1] *= ds_.y; v[k + 2] *= ds_.z; v[k + 3] *= ds_.w;
      }
    }
    uint4 o;
    o.x = pack_bf16x2(v[0], v[1]); o.y = pack_bf16x2(v[2], v[3]); o.z = pack_bf16x2(v[4], v[5]); o.w = pack_bf16x2(v[6], v[7]);
    reinterpret_cast<uint4*>(y)[i] = o;
  }
  if (blockIdx.x == 0 && threadIdx.x < n - 8 * n8) {
    const int64_t i = 8 * n8 + threadIdx.x;
    y[i] = bf16_bits(x[i] * (p > 0.f ? drop_scale(seed, (uint64_t)i, p, inv_keep) : 1.f));
  }
}
__global__ void bf16_to_f32_kernel(const uint16_t* x, float* y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = __uint_as_float((uint32_t)x[i] << 16);
}
// y[c][r] = bf16(x[r][c]) for a row-major [rows][cols] matrix: the bf16 copy of a weight in the orientation that makes
// it a k-contiguous (type R) operand of the backward-data GEMM.  32 x 32 tiles through LDS.
__global__ void f32_to_bf16_transpose_kernel(const float* x, uint16_t* y, int rows, int cols) {
  __shared__ float t[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
  for (int k = ty; k < 32; k += 8)
    if (r0 + k < rows && c0 + tx < cols) t[k][tx] = x[(int64_t)(r0 + k) * cols + c0 + tx];
  __syncthreads();
  for (int k = ty; k < 32; k += 8)
    if (c0 + k < cols && r0 + tx < rows) y[(int64_t)(c0 + k) * rows + r0 + tx] = bf16_bits(t[tx][k]);
}

}  // namespace vqa

using namespace vqa;

extern "C" {

int64_t vqa_gemm_bf16_workspace_bytes(int M, int N, int K) { return slab_bytes(plan_gemm(M, N, K, BKB), M, N); }

int vqa_gemm_bf16(const void* A, int64_t lda, int transA, const void* B, int64_t ldb, int transB, void* C,
                  int64_t ldc, int c_is_bf16, int M, int N, int K, const float* bias1, const float* bias2,
                  const float* rowgroup, int64_t rg_ld, int rg_div, int rg_op, int relu, int accumulate, float* aux,
                  float* workspace, int64_t workspace_bytes, int tag, vqa_stream_t stream) {
  if (int rc = check_gemm_args("vqa_gemm_bf16", 8, A, lda, B, ldb, C, ldc, M, N, K, rowgroup, rg_div)) return rc;
  VQA_REQUIRE(K % 8 == 0, "vqa_gemm_bf16: K must be a multiple of 8 (K=%d)", K);
  VQA_REQUIRE((!transA || M % 8 == 0) && (transB || N % 8 == 0),
              "vqa_gemm_bf16: a reduction-major operand needs its row length to be a multiple of 8 (M=%d N=%d)", M, N);
  VQA_REQUIRE(!(c_is_bf16 && accumulate), "vqa_gemm_bf16: accumulate needs an fp32 C");
  hipStream_t s = (hipStream_t)stream;
  GemmPlan p = plan_gemm(M, N, K, BKB);
  EpiParams pe = epi_params(c_is_bf16 ? nullptr : static_cast<float*>(C), c_is_bf16 ? static_cast<uint16_t*>(C) : nullptr, ldc, M, N,
                            bias1, bias2, rowgroup, rg_ld, rg_div, rg_op, relu, accumulate, aux);
  // the ordinary plan's workspace is asked for first, whichever plan then runs (plan_gemm_wide: gemm.hip)
  if (int rc = claim_slab("vqa_gemm_bf16", p, pe, workspace, workspace_bytes)) return rc;
  const bool wide = plan_gemm_wide(p, M, N, K, transA, transB, workspace != nullptr, workspace_bytes);
  if (wide) claim_slab("vqa_gemm_bf16", p, pe, workspace, workspace_bytes);      // admitted: the workspace holds its slabs
  return run_gemm(p, pe, tag, s, [&] {
    using W = CfgB128x256;
    return wide    ? launch_gemm_bf16<W, PlainCb<W::BM, W::LT>, PlainCb<W::BN, W::LT>>({A, lda, M, K}, {B, ldb, N, K}, pe, p, s)
           : p.big ? dispatch_gemm_bf16<CfgB128>(A, lda, transA, B, ldb, transB, pe, p, M, N, K, s)
                   : dispatch_gemm_bf16<CfgB64>(A, lda, transA, B, ldb, transB, pe, p, M, N, K, s);
  });
}

int vqa_gemm_plan(int engine, int M, int N, int K, int transA, int transB, int64_t workspace_bytes, int32_t* out, int n_out) {
  VQA_REQUIRE(engine >= 0 && engine <= 2 && M > 0 && N > 0 && K > 0 && out && n_out >= 10,
              "vqa_gemm_plan: bad args (engine=%d M=%d N=%d K=%d n_out=%d)", engine, M, N, K, n_out);
  GemmPlan p = engine == 1 ? plan_gemm_x3(M, N, K) : plan_gemm(M, N, K, engine == 2 ? BKB : BK);
  // vqa_gemm_bf16 claims the ordinary plan's workspace before it asks for the wide plan
  const bool wide = engine == 2 && workspace_bytes >= slab_bytes(p, M, N) &&
                    plan_gemm_wide(p, M, N, K, transA, transB, workspace_bytes > 0, workspace_bytes);
  const int bm = engine == 1 ? X3_BM : p.big == 2 ? 256 : p.big ? 128 : 64;
  const int bn = engine == 1 ? X3_BN : wide ? 256 : p.big ? 128 : 64;
  const bool persistent = engine == 0 ? gemm_runs_persistent(p) : engine == 1 && gemm_x3_runs_persistent(p);
  const int32_t v[10] = {bm, bn, p.tiles_m, p.tiles_n, p.nk, p.splits, p.ks_per_split, p.order, persistent, wide};
  for (int i = 0; i < 10; ++i) out[i] = v[i];
  return VQA_OK;
}

int vqa_f32_to_bf16(const float* x, void* y_bf16, int64_t n, vqa_stream_t stream) {
  VQA_REQUIRE(x && y_bf16 && n > 0, "vqa_f32_to_bf16: bad args");
  VQA_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)y_bf16 % 16) == 0, "vqa_f32_to_bf16: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(grid_for(n / 8, 256)), dim3(256), 0, (hipStream_t)stream, x,
                     static_cast<uint16_t*>(y_bf16), n);
  return check_hip(hipGetLastError(), "f32_to_bf16 launch");
}

int vqa_dropout_to_bf16(const float* x, void* y_bf16, int64_t n, float p, uint64_t seed, vqa_stream_t stream) {
  VQA_REQUIRE(x && y_bf16 && n > 0 && p >= 0.f && p < 1.f, "vqa_dropout_to_bf16: bad args");
  VQA_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)y_bf16 % 16) == 0, "vqa_dropout_to_bf16: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(dropout_to_bf16_kernel, dim3(grid_for(n / 8, 256)), dim3(256), 0, (hipStream_t)stream, x,
                     static_cast<uint16_t*>(y_bf16), n, p, keep_scale(p), seed);
  return check_hip(hipGetLastError(), "dropout_to_bf16 launch");
}

int vqa_bf16_to_f32(const void* x_bf16, float* y, int64_t n, vqa_stream_t stream) {
  VQA_REQUIRE(x_bf16 && y && n > 0, "vqa_bf16_to_f32: bad args");
  hipLaunchKernelGGL(bf16_to_f32_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     static_cast<const uint16_t*>(x_bf16), y, n);
  return check_hip(hipGetLastError(), "bf16_to_f32 launch");
}

int vqa_f32_to_bf16_transpose(const float* x, void* y_bf16, int rows, int cols, vqa_stream_t stream) {
  VQA_REQUIRE(x && y_bf16 && rows > 0 && cols > 0, "vqa_f32_to_bf16_transpose: bad args");
  hipLaunchKernelGGL(f32_to_bf16_transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0,
                     (hipStream_t)stream, x, static_cast<uint16_t*>(y_bf16), rows, cols);
  return check_hip(hipGetLastError(), "f32_to_bf16_transpose launch");
}

}  // extern "C"
