// First conv block backward-data: the gradient of the loss w.r.t. the input image (saliency, attribution,
// adversarial checks), and the NHWC -> NCHW layout kernel that returns the generic path's input gradient in the
// caller's layout.
//
// Reference: models/model.py:80-82, first iteration (Conv2d(Ci, Co, k=3) + ReLU + MaxPool2d(2,2)); what autograd
// gives back for the image when v.requires_grad.
//
//   dv[b,c,y,x] = sum_{co,ky,kx} w[co,c,ky,kx] * dY[b,co,y-ky,x-kx],
//   dY[b,co,oy,ox] = dP0[b,oy/2,ox/2,co] if the window's arg-max byte is 2*(oy%2)+(ox%2), else 0.
//
// Gather form, no atomics: a thread owns a 2 x 2 block of output pixels (rows 2i, 2i+1, columns 2j, 2j+1).  The
// pre-pool positions that reach it lie in the pool windows (i-1..i, j-1..j); for each of these four windows and each
// output channel, the window's arg-max position decides which one of the nine taps reaches which of the four pixels,
// and that is a compile-time table once the gradient is split by position (gp[p] = a == p ? g : 0).  Per output
// channel a thread does 16 selects and 36 * Ci FMAs for 4 pixels; the weights are wave-uniform (scalar loads).
// A workgroup covers C0D_R block rows x TW block columns; the pooled gradient and the arg-max bytes of its
// (C0D_R + 1) x (TW + 1) windows are staged in LDS, C0D_CC channels at a time, channel-planar (consecutive lanes read
// consecutive windows: no bank conflicts), with 16-byte (fp32) / 8-byte (bf16) global loads.  Windows outside the
// pooled map are staged as dead, so rows and columns that no pooled output reaches come out as exact zeros.
#include "common.hpp"

namespace vqa {

constexpr int C0D_R = 4;     // block rows (8 image rows) per workgroup
constexpr int C0D_CC = 16;   // output channels staged per LDS pass

__device__ __forceinline__ float c0d_bf16_round(float f) {
  const uint32_t u = __float_as_uint(f);
  return __uint_as_float((u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u);   // round to nearest even (finite weights)
}

// grid (ntx * nby, B), block 4 * TW threads.  DPH: dP0 stored as bf16.  OH: dv written as fp16.  WR: weights rounded
// to bf16 (the bf16 path's forward product).
template <int CI, bool DPH, bool OH, bool WR>
__global__ __launch_bounds__(256) void conv0_dgrad_kernel(const void* __restrict__ dp_, const uint8_t* __restrict__ amax,
                                                          const float* __restrict__ w, void* __restrict__ dv_, int H, int W,
                                                          int Hp, int Wp, int Co, int TW, int ntx) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int TW1 = TW + 1, NW = (C0D_R + 1) * TW1;        // staged windows per channel
  float* gl = lds;                                        // [C0D_CC][C0D_R + 1][TW + 1]
  uint8_t* al = reinterpret_cast<uint8_t*>(lds + C0D_CC * NW);
  const int tid = threadIdx.x;
  const int b = blockIdx.y, tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
  const int i0 = ty * C0D_R, j0 = tx * TW;
  const int r = tid / TW, cc = tid - r * TW;              // this thread's block: (i0 + r, j0 + cc)
  const int64_t img = (int64_t)b * Hp * Wp;

  float acc[CI][2][2];
#pragma unroll
  for (int c = 0; c < CI; ++c)
#pragma unroll
    for (int ly = 0; ly < 2; ++ly) { acc[c][ly][0] = 0.f; acc[c][ly][1] = 0.f; }

  for (int c0 = 0; c0 < Co; c0 += C0D_CC) {
    __syncthreads();                                      // the previous pass's readers are done
    // stage: item = (window, quad of 4 channels)
    for (int e = tid; e < NW * (C0D_CC / 4); e += blockDim.x) {
      const int win = e >> 2, q = e & 3;
      const int wr = win / TW1, wc = win - wr * TW1;
      const int py = i0 - 1 + wr, px = j0 - 1 + wc;
      float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
      uint32_t a4 = 0x04040404u;                          // dead
      if (py >= 0 && py < Hp && px >= 0 && px < Wp) {
        const int64_t off = (img + (int64_t)py * Wp + px) * Co + c0 + 4 * q;
        if (DPH) {
          const uint2 h = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(dp_) + off);
          g = make_float4(__uint_as_float(h.x << 16), __uint_as_float(h.x & 0xFFFF0000u), __uint_as_float(h.y << 16),
                          __uint_as_float(h.y & 0xFFFF0000u));
        } else {
          g = *reinterpret_cast<const float4*>(static_cast<const float*>(dp_) + off);
        }
        a4 = *reinterpret_cast<const uint32_t*>(amax + off);
      }
      const int base = (4 * q) * NW + win;
      gl[base] = g.x; gl[base + NW] = g.y; gl[base + 2 * NW] = g.z; gl[base + 3 * NW] = g.w;
      al[base] = (uint8_t)a4; al[base + NW] = (uint8_t)(a4 >> 8);
      al[base + 2 * NW] = (uint8_t)(a4 >> 16); al[base + 3 * NW] = (uint8_t)(a4 >> 24);
    }
    __syncthreads();
    const int nco = min(C0D_CC, Co - c0);
    for (int k = 0; k < nco; ++k) {                       // wave-uniform
      const int co = c0 + k;
      // gp[wy][wx][p]: the window's gradient at arg-max position p, zero elsewhere (and for a dead window)
      float gp[2][2][4];
#pragma unroll
      for (int wy = 0; wy < 2; ++wy)
#pragma unroll
        for (int wx = 0; wx < 2; ++wx) {
          const int s = k * NW + (r + wy) * TW1 + cc + wx;
          const float g = gl[s];
          const int a = al[s];
#pragma unroll
          for (int p = 0; p < 4; ++p) gp[wy][wx][p] = a == p ? g : 0.f;
        }
#pragma unroll
      for (int c = 0; c < CI; ++c) {
        float wt[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const float v = w[((int64_t)co * CI + c) * 9 + t];
          wt[t] = WR ? c0d_bf16_round(v) : v;
        }
        // pixel (ly, lx) of the block, window (wy, wx) (0: i-1 / j-1, 1: i / j), position (dy, dx):
        // ky = 2 - 2 wy + ly - dy, kx = 2 - 2 wx + lx - dx
#pragma unroll
        for (int ly = 0; ly < 2; ++ly)
#pragma unroll
          for (int lx = 0; lx < 2; ++lx)
#pragma unroll
            for (int wy = 0; wy < 2; ++wy)
#pragma unroll
              for (int dy = 0; dy < 2; ++dy) {
                const int ky = 2 - 2 * wy + ly - dy;
                if (ky < 0 || ky > 2) continue;
#pragma unroll
                for (int wx = 0; wx < 2; ++wx)
#pragma unroll
                  for (int dx = 0; dx < 2; ++dx) {
                    const int kx = 2 - 2 * wx + lx - dx;
                    if (kx < 0 || kx > 2) continue;
                    acc[c][ly][lx] = fmaf(gp[wy][wx][2 * dy + dx], wt[3 * ky + kx], acc[c][ly][lx]);
                  }
              }
      }
    }
  }

  // store: rows 2i, 2i+1 (the second only when it exists), columns 2j, 2j+1 (W % 4 == 0: both exist)
  const int i = i0 + r, j = j0 + cc;
  if (r >= C0D_R || j >= W / 2 || 2 * i >= H) return;
#pragma unroll
  for (int c = 0; c < CI; ++c)
#pragma unroll
    for (int ly = 0; ly < 2; ++ly) {
      const int y = 2 * i + ly;
      if (y >= H) continue;
      const int64_t o = (((int64_t)b * CI + c) * H + y) * W + 2 * j;
      if (OH) {
        typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
        h16x2 hv;
        hv[0] = (_Float16)acc[c][ly][0];
        hv[1] = (_Float16)acc[c][ly][1];
        *reinterpret_cast<h16x2*>(static_cast<uint16_t*>(dv_) + o) = hv;
      } else {
        *reinterpret_cast<float2*>(static_cast<float*>(dv_) + o) = make_float2(acc[c][ly][0], acc[c][ly][1]);
      }
    }
}

// NHWC [B][H][W][CP] fp32 -> NCHW [B][C][H][W] fp32 or fp16 (the pad channels C..CP-1 dropped): the inverse of
// vqa_nchw_to_nhwc4.  One thread per pixel; grid-stride.
template <bool OH>
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* __restrict__ x, void* __restrict__ y, int C, int CP,
                                                           int64_t HW, int64_t total) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = p / HW, s = p - b * HW;
    const float* src = x + p * CP;
    for (int c = 0; c < C; ++c) {
      const int64_t o = (b * C + c) * HW + s;
      if (OH) static_cast<_Float16*>(y)[o] = (_Float16)src[c];
      else static_cast<float*>(y)[o] = src[c];
    }
  }
}

static bool c0d_supported(int Ci, int H, int W, int Co) {
  const int Hp = (H - 2) / 2, Wp = (W - 2) / 2;
  return Ci >= 1 && Ci <= 3 && (Co == 32 || Co == 64) && W % 4 == 0 && H >= 6 && Hp > 0 && Wp > 0;
}

}  // namespace vqa

using namespace vqa;

extern "C" {

int vqa_conv0_dgrad_supported(int Ci, int H, int W, int Co, int stride) {
  return (stride == 1 && c0d_supported(Ci, H, W, Co)) ? 1 : 0;
}

int vqa_conv0_dgrad(const void* dpooled, int dpooled_is_bf16, const uint8_t* argmax, const float* w, void* dv, int dv_is_fp16,
                    int round_w_bf16, int B, int Ci, int H, int W, int Co, vqa_stream_t stream) {
  VQA_REQUIRE(dpooled && argmax && w && dv && B > 0, "vqa_conv0_dgrad: bad args");
  VQA_REQUIRE(c0d_supported(Ci, H, W, Co), "vqa_conv0_dgrad: unsupported shape Ci=%d H=%d W=%d Co=%d", Ci, H, W, Co);
  VQA_REQUIRE(B <= 65535, "vqa_conv0_dgrad: B=%d above the grid limit", B);
  VQA_REQUIRE(((uintptr_t)dpooled % 16) == 0 && ((uintptr_t)argmax % 16) == 0 && ((uintptr_t)dv % 8) == 0,
              "vqa_conv0_dgrad: dpooled / argmax must be 16-byte aligned, dv 8-byte aligned");
  const int Hp = (H - 2) / 2, Wp = (W - 2) / 2;
  const int BW = W / 2, BH = (H + 1) / 2;                // 2 x 2 output blocks
  const int ntx = (BW + 63) / 64;
  const int TW = (BW + ntx - 1) / ntx;                   // <= 64: 4 * TW <= 256 threads
  const int nby = (BH + C0D_R - 1) / C0D_R;
  const size_t NW = (size_t)(C0D_R + 1) * (TW + 1);
  const size_t lds = (size_t)C0D_CC * NW * 5;
  const dim3 grid(ntx * nby, B), block(C0D_R * TW);
  const int dph = dpooled_is_bf16 ? 1 : 0, oh = dv_is_fp16 ? 1 : 0, wr = round_w_bf16 ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
#define C0D_LAUNCH(CI, DPH, OH, WR)                                                                                  \
  hipLaunchKernelGGL((conv0_dgrad_kernel<CI, DPH, OH, WR>), grid, block, lds, s, dpooled, argmax, w, dv, H, W, Hp, Wp, \
                     Co, TW, ntx)
#define C0D_CI(DPH, OH, WR)                       \
  switch (Ci) {                                   \
    case 1: C0D_LAUNCH(1, DPH, OH, WR); break;    \
    case 2: C0D_LAUNCH(2, DPH, OH, WR); break;    \
    default: C0D_LAUNCH(3, DPH, OH, WR); break;   \
  }
  switch (dph * 4 + oh * 2 + wr) {
    case 0: C0D_CI(false, false, false); break;
    case 1: C0D_CI(false, false, true); break;
    case 2: C0D_CI(false, true, false); break;
    case 3: C0D_CI(false, true, true); break;
    case 4: C0D_CI(true, false, false); break;
    case 5: C0D_CI(true, false, true); break;
    case 6: C0D_CI(true, true, false); break;
    default: C0D_CI(true, true, true); break;
  }
#undef C0D_CI
#undef C0D_LAUNCH
  return check_hip(hipGetLastError(), "conv0_dgrad launch");
}

int vqa_nhwc_to_nchw(const float* x_nhwc, void* y_nchw, int y_is_fp16, int B, int C, int CP, int H, int W, vqa_stream_t stream) {
  VQA_REQUIRE(x_nhwc && y_nchw && B > 0 && H > 0 && W > 0 && C >= 1 && C <= CP, "vqa_nhwc_to_nchw: bad args C=%d CP=%d", C, CP);
  const int64_t HW = (int64_t)H * W, total = (int64_t)B * HW;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  if (y_is_fp16)
    hipLaunchKernelGGL(nhwc_to_nchw_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x_nhwc, y_nchw, C, CP, HW, total);
  else
    hipLaunchKernelGGL(nhwc_to_nchw_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x_nhwc, y_nchw, C, CP, HW, total);
  return check_hip(hipGetLastError(), "nhwc_to_nchw launch");
}

}  // extern "C"
