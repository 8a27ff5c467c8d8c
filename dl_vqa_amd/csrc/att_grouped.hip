// Attention scores for many questions per image (inference): one v' = v_conv(vn) per IMAGE, the questions of an image walked
// over an LDS-resident tile of it.  x = relu(v' (+|*) q') is never written:
//   score[b][g][p] = bx[g] + sum_m wx[g][m] * relu(v'[n*P + p][m] (+|*) q'[b][m])                          n = image of b
//   '|':  score[b][g][p] = (bx[g] + sum_m wx[g][m] * relu(v'[n*P + p][m])) + sum_m wx[g][mid + m] * relu(q'[b][m])
// A workgroup (4 waves) owns TP = 4 * PW consecutive positions of ONE image: the tile [TP][mid] fp32 is copied to LDS once
// (64 KiB at TP = 16, mid = 1024: two workgroups per CU), then every question order[offsets[n] .. offsets[n+1]) of that image
// reads only its q' row (4 KiB, through L2).  HBM traffic: v' once per image instead of x once per question.
// No atomics: a score element is the sum over a lane's channel quads lane*4 + 256*i in ascending i (x, y, z, w inside a quad),
// then the wave butterfly -- the same order whatever the grouping, the tile or the kernel variant.
#include "common.hpp"

namespace vqa {

template <bool MUL>
__device__ __forceinline__ float4 att_combine(const float4 v, const float4 q) {
  float4 x;
  if (MUL) { x.x = v.x * q.x; x.y = v.y * q.y; x.z = v.z * q.z; x.w = v.w * q.w; }
  else { x.x = v.x + q.x; x.y = v.y + q.y; x.z = v.z + q.z; x.w = v.w + q.w; }
  x.x = fmaxf(x.x, 0.f); x.y = fmaxf(x.y, 0.f); x.z = fmaxf(x.z, 0.f); x.w = fmaxf(x.w, 0.f);
  return x;
}
__device__ __forceinline__ float4 relu4(float4 x) {
  x.x = fmaxf(x.x, 0.f); x.y = fmaxf(x.y, 0.f); x.z = fmaxf(x.z, 0.f); x.w = fmaxf(x.w, 0.f);
  return x;
}
__device__ __forceinline__ float dot4(const float4 x, const float4 w) { return x.x * w.x + x.y * w.y + x.z * w.z + x.w * w.w; }

// tile rows row0 .. row0+rows-1 of v' -> LDS (a flat copy: the rows of one image are contiguous in v')
__device__ __forceinline__ void att_tile_to_lds(const float* vprime, float* tile, int64_t row0, int rows, int mid) {
  const float4* src = reinterpret_cast<const float4*>(vprime + row0 * mid);
  float4* dst = reinterpret_cast<float4*>(tile);
  const int n4 = rows * (mid >> 2);
  int i = threadIdx.x;
  for (; i + 768 < n4; i += 1024) {          // four loads in flight per thread
    float4 t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) t[u] = src[i + 256 * u];
#pragma unroll
    for (int u = 0; u < 4; ++u) dst[i + 256 * u] = t[u];
  }
  for (; i < n4; i += 256) dst[i] = src[i];
}

// the question range of image n, clamped to [0, B] (a malformed offsets array then reads nothing out of bounds)
__device__ __forceinline__ void att_group_range(const int* offsets, int n, int B, int& k0, int& k1) {
  k0 = offsets[n];
  k1 = offsets[n + 1];
  k0 = k0 < 0 ? 0 : k0;
  k1 = k1 > B ? B : k1;
}

// '+' / '*', mid = 256 * IT <= 1024: x_conv weights and the question's q' row in registers, 4 positions per wave.
// grid (ceil(P/16), N), 256 threads, 16 * mid floats of dynamic LDS.
template <int G, int IT, bool MUL>
__global__ __launch_bounds__(256) void att_score_grouped_kernel(const float* vprime, const float* qp, const float* wx, int wx_ld,
                                                                const float* bx, const int* order, const int* offsets,
                                                                float* score, int B, int P) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  constexpr int mid = 256 * IT, PW = 4, TP = 16;
  const int n = blockIdx.y, p0 = blockIdx.x * TP;
  int k0, k1;
  att_group_range(offsets, n, B, k0, k1);
  if (k0 >= k1) return;                                   // nobody asks about this image
  const int rows = min(TP, P - p0);
  att_tile_to_lds(vprime, tile, (int64_t)n * P + p0, rows, mid);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 w[IT][G];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int g = 0; g < G; ++g) w[i][g] = reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld)[lane + 64 * i];
  float bias[G];
#pragma unroll
  for (int g = 0; g < G; ++g) bias[g] = bx[g];
  __syncthreads();
  const int pl = wave * PW;                               // first local position of this wave
  if (pl >= rows) return;
  float4 q[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  int b = order[k0];
  bool ok = (unsigned)b < (unsigned)B;
  if (ok) {
#pragma unroll
    for (int i = 0; i < IT; ++i) q[i] = reinterpret_cast<const float4*>(qp + (int64_t)b * mid)[lane + 64 * i];
  }
  for (int k = k0; k < k1; ++k) {
    // the next question's q' row is in flight while this one is reduced
    float4 qn[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) qn[i] = q[i];
    int bn = -1;
    bool okn = false;
    if (k + 1 < k1) {
      bn = order[k + 1];
      okn = (unsigned)bn < (unsigned)B;
      if (okn) {
#pragma unroll
        for (int i = 0; i < IT; ++i) qn[i] = reinterpret_cast<const float4*>(qp + (int64_t)bn * mid)[lane + 64 * i];
      }
    }
    if (ok) {
      float acc[PW][G];
#pragma unroll
      for (int j = 0; j < PW; ++j)
#pragma unroll
        for (int g = 0; g < G; ++g) acc[j][g] = 0.f;
#pragma unroll
      for (int i = 0; i < IT; ++i) {
#pragma unroll
        for (int j = 0; j < PW; ++j) {
          if (pl + j < rows) {                            // wave-uniform
            const float4 v = reinterpret_cast<const float4*>(tile + (pl + j) * mid)[lane + 64 * i];
            const float4 x = att_combine<MUL>(v, q[i]);
#pragma unroll
            for (int g = 0; g < G; ++g) acc[j][g] += dot4(x, w[i][g]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < PW; ++j) {
        if (pl + j < rows) {
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const float s = wave_sum(acc[j][g]);
            if (lane == 0) score[((int64_t)b * G + g) * P + p0 + pl + j] = s + bias[g];
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) q[i] = qn[i];
    b = bn;
    ok = okn;
  }
}

// Any mid % 4 == 0 and every mode: the channel walk is a run-time loop (weights and q' re-read through L1 per position),
// `pw` positions per wave (the tile is 4 * pw rows).  Same per-lane operation order as the kernel above.
template <int G>
__global__ __launch_bounds__(256) void att_score_grouped_general_kernel(const float* vprime, const float* qp, const float* wx,
                                                                        int wx_ld, const float* bx, const int* order,
                                                                        const int* offsets, float* score, int B, int P, int mid,
                                                                        int pw, int mode) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  const int TP = 4 * pw;
  const int n = blockIdx.y, p0 = blockIdx.x * TP;
  int k0, k1;
  att_group_range(offsets, n, B, k0, k1);
  if (k0 >= k1) return;
  const int rows = min(TP, P - p0);
  att_tile_to_lds(vprime, tile, (int64_t)n * P + p0, rows, mid);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nq = mid >> 2;
  for (int j = 0; j < pw; ++j) {
    const int pl = wave * pw + j;
    if (pl >= rows) break;
    const float4* vrow = reinterpret_cast<const float4*>(tile + pl * mid);
    float vpart[G];
#pragma unroll
    for (int g = 0; g < G; ++g) vpart[g] = 0.f;
    if (mode == 2) {                                      // the v' half does not depend on the question
      float acc[G];
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = 0.f;
      for (int c = lane; c < nq; c += 64) {
        const float4 x = relu4(vrow[c]);
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] += dot4(x, reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld)[c]);
      }
#pragma unroll
      for (int g = 0; g < G; ++g) vpart[g] = wave_sum(acc[g]) + bx[g];
    }
    for (int k = k0; k < k1; ++k) {
      const int b = order[k];
      if ((unsigned)b >= (unsigned)B) continue;
      const float4* qrow = reinterpret_cast<const float4*>(qp + (int64_t)b * mid);
      float acc[G];
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = 0.f;
      if (mode == 2) {
        for (int c = lane; c < nq; c += 64) {
          const float4 x = relu4(qrow[c]);
#pragma unroll
          for (int g = 0; g < G; ++g) acc[g] += dot4(x, reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld + mid)[c]);
        }
      } else {
        for (int c = lane; c < nq; c += 64) {
          const float4 x = mode == 1 ? att_combine<true>(vrow[c], qrow[c]) : att_combine<false>(vrow[c], qrow[c]);
#pragma unroll
          for (int g = 0; g < G; ++g) acc[g] += dot4(x, reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld)[c]);
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float s = wave_sum(acc[g]);
        if (lane == 0) score[((int64_t)b * G + g) * P + p0 + pl] = mode == 2 ? vpart[g] + s : s + bx[g];
      }
    }
  }
}

}  // namespace vqa

using namespace vqa;

extern "C" {

int vqa_att_score_grouped_fwd(const float* vprime, const float* qp, const float* wx, int wx_ld, const float* bx,
                              const int32_t* order, const int32_t* offsets, float* score, int N, int B, int P, int mid, int G,
                              int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_FWD, (hipStream_t)stream);
  VQA_REQUIRE(G >= 1 && G <= 4, "glimpses=%d unsupported (1..4)", G);
  VQA_REQUIRE(mode >= 0 && mode <= 2, "vqa_att_score_grouped_fwd: mode %d (0 '+', 1 '*', 2 '|')", mode);
  VQA_REQUIRE(vprime && qp && wx && bx && score, "vqa_att_score_grouped_fwd: null pointer");
  VQA_REQUIRE(order && offsets, "vqa_att_score_grouped_fwd: null order / offsets");
  VQA_REQUIRE(N >= 1 && N <= 65535 && B >= 0 && P >= 1, "vqa_att_score_grouped_fwd: N=%d (1..65535), B=%d, P=%d out of range",
              N, B, P);
  VQA_REQUIRE(mid >= 4 && mid % 4 == 0 && wx_ld % 4 == 0 && wx_ld >= (mode == 2 ? 2 * mid : mid),
              "vqa_att_score_grouped_fwd: bad args (mid=%d and wx_ld=%d must be multiples of 4, wx_ld >= channels of x)", mid,
              wx_ld);
  VQA_REQUIRE(mid <= 4096, "vqa_att_score_grouped_fwd: mid=%d too large for the LDS tile (4 rows x mid fp32 <= 64 KiB)", mid);
  VQA_REQUIRE(((reinterpret_cast<uintptr_t>(vprime) | reinterpret_cast<uintptr_t>(qp) | reinterpret_cast<uintptr_t>(wx)) & 15) == 0,
              "vqa_att_score_grouped_fwd: vprime, qp and wx must be 16-byte aligned");
  if (B == 0) return VQA_OK;
  hipStream_t s = (hipStream_t)stream;
  if (mode != 2 && mid % 256 == 0 && mid <= 1024) {
    const dim3 grid((P + 15) / 16, N);
    const size_t lds = (size_t)16 * mid * 4;
#define GROUPED_LAUNCH(kG, kIT)                                                                                                   \
  do {                                                                                                                            \
    if (mode == 1)                                                                                                                \
      hipLaunchKernelGGL((att_score_grouped_kernel<kG, kIT, true>), grid, dim3(256), lds, s, vprime, qp, wx, wx_ld, bx, order,    \
                         offsets, score, B, P);                                                                                   \
    else                                                                                                                          \
      hipLaunchKernelGGL((att_score_grouped_kernel<kG, kIT, false>), grid, dim3(256), lds, s, vprime, qp, wx, wx_ld, bx, order,   \
                         offsets, score, B, P);                                                                                   \
  } while (0)
#define GROUPED_IT(kG)                                                                                                            \
  switch (mid / 256) {                                                                                                            \
    case 1: GROUPED_LAUNCH(kG, 1); break;                                                                                         \
    case 2: GROUPED_LAUNCH(kG, 2); break;                                                                                         \
    case 3: GROUPED_LAUNCH(kG, 3); break;                                                                                         \
    default: GROUPED_LAUNCH(kG, 4); break;                                                                                        \
  }
    switch (G) {
      case 1: GROUPED_IT(1); break;
      case 2: GROUPED_IT(2); break;
      case 3: GROUPED_IT(3); break;
      default: GROUPED_IT(4); break;
    }
#undef GROUPED_IT
#undef GROUPED_LAUNCH
    return check_hip(hipGetLastError(), "att_score_grouped_fwd launch");
  }
  const int pw = mid <= 1024 ? 4 : (mid <= 2048 ? 2 : 1);      // 4 * pw rows of mid floats <= 64 KiB
  const int TP = 4 * pw;
  const dim3 grid((P + TP - 1) / TP, N);
  const size_t lds = (size_t)TP * mid * 4;
  switch (G) {
    case 1: hipLaunchKernelGGL(att_score_grouped_general_kernel<1>, grid, dim3(256), lds, s, vprime, qp, wx, wx_ld, bx, order,
                               offsets, score, B, P, mid, pw, mode); break;
    case 2: hipLaunchKernelGGL(att_score_grouped_general_kernel<2>, grid, dim3(256), lds, s, vprime, qp, wx, wx_ld, bx, order,
                               offsets, score, B, P, mid, pw, mode); break;
    case 3: hipLaunchKernelGGL(att_score_grouped_general_kernel<3>, grid, dim3(256), lds, s, vprime, qp, wx, wx_ld, bx, order,
                               offsets, score, B, P, mid, pw, mode); break;
    default: hipLaunchKernelGGL(att_score_grouped_general_kernel<4>, grid, dim3(256), lds, s, vprime, qp, wx, wx_ld, bx, order,
                                offsets, score, B, P, mid, pw, mode); break;
  }
  return check_hip(hipGetLastError(), "att_score_grouped_fwd launch");
}

}  // extern "C"
