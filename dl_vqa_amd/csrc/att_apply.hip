// The second half of the attention stage: softmax over positions + weighted sum of the image features, forward and
// backward -- the vqa_att_apply_* entry points, plain, gathered (several questions per image) and on a float16
// image-feature cache; and the dscore backward that also writes r1, the weighted-sum path of the gradient x input map
// (vqa_att_attr_apply_gather).  The scores it starts from: att_score.hip.  HBM-bound streaming kernels, as in elementwise.hip.
#include <hip/hip_fp16.h>
#include "common.hpp"
#include "cache_load.hpp"

namespace vqa {

// Softmax over the P positions of every glimpse into LDS (and to `probs` from the first channel block).
template <int G>
__device__ __forceinline__ void att_softmax_to_lds(const float* score, float* probs, float* pr, float* red, int b, int P,
                                                   bool write) {
  const int tid = threadIdx.x;
  for (int g = 0; g < G; ++g) {
    const float* s = score + ((int64_t)b * G + g) * P;
    float mx = -INFINITY;
    for (int i = tid; i < P; i += blockDim.x) mx = fmaxf(mx, s[i]);
    mx = block_reduce(mx, red, true);
    float sum = 0.f;
    for (int i = tid; i < P; i += blockDim.x) { const float e = expf(s[i] - mx); pr[g * P + i] = e; sum += e; }
    sum = block_reduce(sum, red, false);
    const float inv = 1.f / sum;
    for (int i = tid; i < P; i += blockDim.x) {
      const float v = pr[g * P + i] * inv;
      pr[g * P + i] = v;
      if (write) probs[((int64_t)b * G + g) * P + i] = v;
    }
  }
}

// C % 4 == 0: 256 threads = 16 position groups x 16 channel quads, 16-byte loads, four positions in flight per thread
// (the scalar form below runs at 26 % of the HBM rate: one 4-byte load per FMA pair, 169 dependent iterations).
// grid (B, ceil(C/64)); dynamic LDS: G*P + 16 + 16*G*64 floats.  Sum order per channel: positions pg, pg+16, ... within
// a group, then the 16 groups in order.
// b = the sample (score / probs / out row), n = the image whose vn rows it weights: n == b in vqa_att_apply_fwd,
// n = img[b] in vqa_att_apply_gather_fwd (several questions per image).  VT: vn's element type (cache_load.hpp); a lane's
// four channels are one 16-byte load of fp32 or one 8-byte load of fp16, everything else is the same code.
template <int G, class VT>
__device__ __forceinline__ void att_apply_fwd_v4_body(float* sm, const float* score, const VT* vn, float* probs, float* out,
                                                      int64_t out_ld, int P, int C, int b, int n) {
  float* pr = sm;            // [G][P]
  float* red = sm + G * P;   // [16]
  float* part = red + 16;    // [16][G][64]
  const int tid = threadIdx.x;
  att_softmax_to_lds<G>(score, probs, pr, red, b, P, blockIdx.y == 0);
  __syncthreads();
  const int cq = tid & 15, pg = tid >> 4;
  const int c = blockIdx.y * 64 + cq * 4;
  float4 acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < C) {
    const VT* vb = vn + (int64_t)n * P * C + c;
    int i = pg;
    for (; i + 48 < P; i += 64) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = load_quad(vb + (int64_t)(i + 16 * u) * C, 0);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float w = pr[g * P + i + 16 * u];
          acc[g].x += w * v[u].x; acc[g].y += w * v[u].y; acc[g].z += w * v[u].z; acc[g].w += w * v[u].w;
        }
    }
    for (; i < P; i += 16) {
      const float4 v = load_quad(vb + (int64_t)i * C, 0);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float w = pr[g * P + i];
        acc[g].x += w * v.x; acc[g].y += w * v.y; acc[g].z += w * v.z; acc[g].w += w * v.w;
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) *reinterpret_cast<float4*>(part + (pg * G + g) * 64 + cq * 4) = acc[g];
  __syncthreads();
  // 64 * G outputs, one per thread (G <= 4)
  for (int o = tid; o < 64 * G; o += 256) {
    const int g = o >> 6, cl = o & 63;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) v += part[(k * G + g) * 64 + cl];
    if (blockIdx.y * 64 + cl < C) out[(int64_t)b * out_ld + g * C + blockIdx.y * 64 + cl] = v;
  }
}

// GATHER (vqa_att_apply_gather_fwd): n = img[b], and a sample whose index is outside [0, N) is left unwritten (block-uniform
// exit).  Otherwise n = b, and img / N are not read.  A float16 vn is a cache: only GATHER is instantiated for it.
template <int G, bool GATHER, class VT = float>
__global__ void att_apply_fwd_v4_kernel(const float* score, const VT* vn, const int* img, float* probs, float* out,
                                        int64_t out_ld, int P, int C, int N) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  int n = blockIdx.x;
  if (GATHER) {
    n = img[blockIdx.x];
    if ((unsigned)n >= (unsigned)N) return;
  }
  att_apply_fwd_v4_body<G>(sm, score, vn, probs, out, out_ld, P, C, blockIdx.x, n);
}

// grid (B, ceil(C/64)), 256 threads = 4 position groups x 64 channels; dynamic LDS: G*P + 16 + 4*G*64 floats
template <int G, class VT>
__device__ __forceinline__ void att_apply_fwd_body(float* sm, const float* score, const VT* vn, float* probs, float* out,
                                                   int64_t out_ld, int P, int C, int b, int n) {
  float* pr = sm;            // [G][P]
  float* red = sm + G * P;   // [16]
  float* part = red + 16;    // [4][G][64]
  const int tid = threadIdx.x;
  att_softmax_to_lds<G>(score, probs, pr, red, b, P, blockIdx.y == 0);
  __syncthreads();
  const int cl = tid & 63, pg = tid >> 6;
  const int c = blockIdx.y * 64 + cl;
  float acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = 0.f;
  if (c < C) {
    const VT* vb = vn + (int64_t)n * P * C + c;
    for (int i = pg; i < P; i += 4) {
      const float v = load_one(vb, (int64_t)i * C);
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] += pr[g * P + i] * v;
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) part[(pg * G + g) * 64 + cl] = acc[g];
  __syncthreads();
  if (pg == 0 && c < C) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float v = part[g * 64 + cl] + part[(G + g) * 64 + cl] + part[(2 * G + g) * 64 + cl] + part[(3 * G + g) * 64 + cl];
      out[(int64_t)b * out_ld + g * C + c] = v;
    }
  }
}

template <int G, bool GATHER, class VT = float>
__global__ void att_apply_fwd_kernel(const float* score, const VT* vn, const int* img, float* probs, float* out,
                                     int64_t out_ld, int P, int C, int N) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  int n = blockIdx.x;
  if (GATHER) {
    n = img[blockIdx.x];
    if ((unsigned)n >= (unsigned)N) return;
  }
  att_apply_fwd_body<G>(sm, score, vn, probs, out, out_ld, P, C, blockIdx.x, n);
}

// pass 1: one wave per (b,p): dprob -> dscore buffer, dvn row written
// One (sample b, position pp) row against the image row `v` that b weights there: dprob[b][g][pp] = <v, dout[b][g]> and
// (d != null) d[c] = sum_g probs[b][g][pp] * dout[b][g*C + c].  v: row b*P + pp in vqa_att_apply_bwd, row img[b]*P + pp in
// vqa_att_apply_gather_bwd -- the (sample, image) form, as in att_apply_fwd_body.  v: the row's first element, fp32 or fp16
// (cache_load.hpp), read a channel quad at a time.
// ATTR (vqa_att_attr_apply_gather): also r1[b][pp] = sum_g probs[b][g][pp] * dprob[b][g][pp], g ascending, from the same
// wave sums before the softmax backward overwrites them -- the weighted-sum path of the gradient x input map.
template <int G, class VT, bool ATTR = false>
__device__ __forceinline__ void att_apply_bwd_row(const float* dout, int64_t dout_ld, const float* probs, const VT* v,
                                                  float4* d, float* dprob, int64_t b, int pp, int P, int C, int lane,
                                                  float* r1) {
  const int nch = C >> 2;
  float pr[G], acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) { pr[g] = probs[(b * G + g) * P + pp]; acc[g] = 0.f; }
  for (int c = lane; c < nch; c += 64) {
    const float4 x = load_quad(v, c);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float4 go = reinterpret_cast<const float4*>(dout + b * dout_ld + (int64_t)g * C)[c];
      acc[g] += x.x * go.x + x.y * go.y + x.z * go.z + x.w * go.w;
      o.x += pr[g] * go.x; o.y += pr[g] * go.y; o.z += pr[g] * go.z; o.w += pr[g] * go.w;
    }
    if (d) d[c] = o;       // d == null: vqa_l2norm_bwd_joined recomputes this branch where it is consumed
  }
  float r = 0.f;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float s = wave_sum(acc[g]);
    if (lane == 0) dprob[(b * G + g) * P + pp] = s;
    if (ATTR) r += pr[g] * s;
  }
  if (ATTR && lane == 0) r1[b * P + pp] = r;
}

// GATHER (vqa_att_apply_gather_bwd, several questions per image): sample b weighted the rows of image img[b] of vn [N][P][C];
// dvn is null there -- the per-image sum is the kernel below.  On a float16 vn (vqa_att_apply_gather_dscore_f16; GATHER
// only) dvn is always null: nobody wants a gradient of a cache.  It stays a run-time argument all the same: the row body
// then compiles to the arithmetic (the same fused multiply-adds) of the fp32 instantiation, which a body specialised for
// d == null does not.
// ATTR (GATHER only): the row body also writes r1 [B][P] (null and not read otherwise); dvn is null at run time there as well.
template <int G, bool GATHER, class VT = float, bool ATTR = false>
__global__ void att_apply_bwd_rows_kernel(const float* dout, int64_t dout_ld, const float* probs, const VT* vn,
                                          const int* img, int N, float* dprob, float* dvn, int64_t M, int P, int C,
                                          float* r1) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t m = wave; m < M; m += nwaves) {
    const int64_t b = m / P;
    const int pp = (int)(m - b * P);
    int64_t vm = m;
    if (GATHER) {
      int n = img[b];
      n = n < 0 ? 0 : (n >= N ? N - 1 : n);               // a malformed index reads nothing out of bounds
      vm = (int64_t)n * P + pp;
    }
    att_apply_bwd_row<G, VT, ATTR>(dout, dout_ld, probs, vn + vm * C, dvn ? reinterpret_cast<float4*>(dvn + m * C) : nullptr, dprob,
                                   b, pp, P, C, lane, r1);
  }
}

// Several questions per image: the weighted-sum branch of d loss / d vn summed per IMAGE, one wave per image row (n, pp):
// dvn[n][pp][c] = sum over the questions b = order[offsets[n] .. offsets[n+1]) in that order, g ascending inside a question,
// of probs[b][g][pp] * dout[b][g*C + c] -- the row body's sum for one question.  Every row of dvn is written, zeros for an
// image nobody asks about.
template <int G>
__global__ void att_apply_gather_dvn_kernel(const float* dout, int64_t dout_ld, const float* probs, const int* order,
                                            const int* offsets, float* dvn, int64_t M, int B, int P, int C) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int nch = C >> 2;
  for (int64_t m = wave; m < M; m += nwaves) {
    const int64_t n = m / P;
    const int pp = (int)(m - n * P);
    int k0 = offsets[n], k1 = offsets[n + 1];
    k0 = k0 < 0 ? 0 : k0;
    k1 = k1 > B ? B : k1;
    float4* d = reinterpret_cast<float4*>(dvn + m * C);
    for (int c = lane; c < nch; c += 64) {
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = k0; k < k1; ++k) {
        const int64_t b = order[k];
        if ((uint64_t)b >= (uint64_t)B) continue;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float pr = probs[(b * G + g) * P + pp];
          const float4 go = reinterpret_cast<const float4*>(dout + b * dout_ld + (int64_t)g * C)[c];
          o.x += pr * go.x; o.y += pr * go.y; o.z += pr * go.z; o.w += pr * go.w;
        }
      }
      d[c] = o;
    }
  }
}
// pass 2: block per (b,g): dscore = probs * (dprob - sum_p probs*dprob), in place on dprob
// rowsum (optional) [B*G]: sum_p dscore of the block's row -- the per-sample part of the x_conv bias gradient
__global__ void softmax_bwd_kernel(const float* probs, float* dscore, int P, float* rowsum) {
  __shared__ float red[16];
  const int64_t base = (int64_t)blockIdx.x * P;
  float s = 0.f;
  for (int i = threadIdx.x; i < P; i += blockDim.x) s += probs[base + i] * dscore[base + i];
  s = block_reduce(s, red, false);
  float t = 0.f;
  for (int i = threadIdx.x; i < P; i += blockDim.x) {
    const float d = probs[base + i] * (dscore[base + i] - s);
    dscore[base + i] = d;
    t += d;
  }
  if (rowsum) {
    t = block_reduce(t, red, false);
    if (threadIdx.x == 0) rowsum[blockIdx.x] = t;
  }
}

}  // namespace vqa

using namespace vqa;

#define STREAM ((hipStream_t)stream)

// ---------------------------------------------------------------- softmax + weighted sum: the host side of vqa_att_apply_*
// dynamic LDS of both forward kernels (the scalar one uses less of it): probs [G][P], 16 reduction slots, part [16][G][64]
static size_t att_apply_fwd_lds(int G, int P) { return ((size_t)G * P + 16 + 16 * G * 64) * 4; }

// What the entry points check, before any HIP call (`who` names the caller in the messages).  backward: the kernels
// read dout / vn and write dvn as float4, so C and the leading dimension are multiples of 4 and `quads` (ptr_bits of those
// pointers, a null one counts as aligned) is 16-byte aligned.  pointers / indices: the form's data pointers and its
// img / order / offsets are all there (true for a form without indices).  N: 1 for a form without an image count.
static int att_apply_check(const char* who, bool backward, bool pointers, bool indices, int N, int B, int P, int C, int G,
                           int64_t ld, uintptr_t quads) {
  VQA_REQUIRE(G >= 1 && G <= 4, "%s: glimpses=%d unsupported (1..4)", who, G);
  VQA_REQUIRE(pointers, "%s: null pointer", who);
  VQA_REQUIRE(indices, "%s: null pointer among img / order / offsets", who);
  const bool widths = backward ? C >= 4 && C % 4 == 0 && ld % 4 == 0 : C >= 1;
  VQA_REQUIRE(N >= 1 && B >= 0 && P >= 1 && widths && ld >= (int64_t)G * C, "%s: N=%d, B=%d, P=%d, C=%d%s, %s=%lld out of range",
              who, N, B, P, C, backward ? " (a multiple of 4)" : "", backward ? "dout_ld" : "out_ld", (long long)ld);
  VQA_REQUIRE(backward || att_apply_fwd_lds(G, P) <= 64 * 1024, "%s: G*P=%d too large for LDS", who, G * P);
  VQA_REQUIRE((quads & 15) == 0, "%s: dout, vn and dvn must be 16-byte aligned", who);
  return VQA_OK;
}

// a float16 vn is a cache, which only the gather forms read: their kernels are the only ones instantiated for it
template <class VT, class F>
static int with_gather(bool gather, F&& f) {
  if constexpr (std::is_same<VT, float>::value) return with_flag(gather, f);
  else return f(Flag<true>{});
}

// img == null: sample b weights its own image (vqa_att_apply_fwd), N is not read.  The quad kernels need whole quads
// of channels and a vn aligned for load_quad (16 bytes of fp32, 8 of fp16); anything else runs the scalar ones.
template <class VT>
static int att_apply_fwd_launch(const float* score, const VT* vn, const int32_t* img, float* probs, float* out,
                                int64_t out_ld, int N, int B, int P, int C, int G, hipStream_t s) {
  if (B == 0) return VQA_OK;
  const dim3 grid(B, (C + 63) / 64);
  const size_t lds = att_apply_fwd_lds(G, P);
  const bool quads = C % 4 == 0 && (ptr_bits(vn) & (kQuadAlign<VT> - 1)) == 0;
  return with_int14(G, [&](auto g) {
    return with_gather<VT>(img != nullptr, [&](auto gather) {
      return with_flag(quads, [&](auto v4) {
        if (decltype(v4)::value)
          hipLaunchKernelGGL((att_apply_fwd_v4_kernel<decltype(g)::value, decltype(gather)::value, VT>), grid, dim3(256), lds, s,
                             score, vn, img, probs, out, out_ld, P, C, N);
        else
          hipLaunchKernelGGL((att_apply_fwd_kernel<decltype(g)::value, decltype(gather)::value, VT>), grid, dim3(256), lds, s,
                             score, vn, img, probs, out, out_ld, P, C, N);
        return check_hip(hipGetLastError(), "att_apply_fwd launch");
      });
    });
  });
}

// img == null: the plain form, whose rows kernel writes dvn [B][P][C] itself (dvn == null: nobody wants it).  With img the
// rows kernel leaves dvn alone, and order / offsets (with dvn [N][P][C]) add the per-image sum; then the softmax backward.
// The dscore forms (fp32 and float16 vn) are the gather form without order / offsets / dvn.
template <class VT>
static int att_apply_bwd_launch(const float* dout, int64_t dout_ld, const float* probs, const VT* vn, const int32_t* img,
                                const int32_t* order, const int32_t* offsets, float* dscore, float* dvn, float* dscore_rowsum,
                                int N, int B, int P, int C, int G, hipStream_t s, float* r1 = nullptr) {
  if (B == 0) return VQA_OK;
  const int64_t M = (int64_t)B * P, Mn = (int64_t)N * P;
  int rc = with_int14(G, [&](auto g) {
    if (r1) {                                             // the attribution form: a dscore form that also writes r1
      hipLaunchKernelGGL((att_apply_bwd_rows_kernel<decltype(g)::value, true, VT, true>), dim3(grid_for(M, 4)), dim3(256), 0, s,
                         dout, dout_ld, probs, vn, img, N, dscore, static_cast<float*>(nullptr), M, P, C, r1);
      return check_hip(hipGetLastError(), "att_apply_bwd_rows (attribution) launch");
    }
    return with_gather<VT>(img != nullptr, [&](auto gather) {
      hipLaunchKernelGGL((att_apply_bwd_rows_kernel<decltype(g)::value, decltype(gather)::value, VT>), dim3(grid_for(M, 4)),
                         dim3(256), 0, s, dout, dout_ld, probs, vn, img, N, dscore, decltype(gather)::value ? nullptr : dvn, M, P, C,
                         static_cast<float*>(nullptr));
      return check_hip(hipGetLastError(), "att_apply_bwd_rows launch");
    });
  });
  if (rc == VQA_OK && order)
    rc = with_int14(G, [&](auto g) {
      hipLaunchKernelGGL(att_apply_gather_dvn_kernel<decltype(g)::value>, dim3(grid_for(Mn, 4)), dim3(256), 0, s, dout, dout_ld,
                         probs, order, offsets, dvn, Mn, B, P, C);
      return check_hip(hipGetLastError(), "att_apply_gather_dvn launch");
    });
  if (rc) return rc;
  hipLaunchKernelGGL(softmax_bwd_kernel, dim3(B * G), dim3(256), 0, s, probs, dscore, P, dscore_rowsum);
  return check_hip(hipGetLastError(), "softmax_bwd launch");
}

extern "C" {

// vqa_att_apply_fwd and vqa_att_apply_bwd take the checks of their gather forms: what used to reach a launch with undefined
// results (out_ld / dout_ld < G*C, P < 1, a dout, vn or dvn that the backward cannot read as float4, G outside 1..4) is
// VQA_ERR_INVALID, and B == 0 is VQA_OK without a launch.  Every argument set that was valid runs the kernels it ran, on the
// same grid, block and LDS size; a vn that is not 16-byte aligned now takes the forward's scalar kernels.
int vqa_att_apply_fwd(const float* score, const float* vn, float* probs, float* out, int64_t out_ld, int B, int P,
                      int C, int G, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_APPLY_FWD, (hipStream_t)stream);
  const int rc = att_apply_check("vqa_att_apply_fwd", false, score && vn && probs && out, true, 1, B, P, C, G, out_ld, 0);
  return rc ? rc : att_apply_fwd_launch(score, vn, nullptr, probs, out, out_ld, 0, B, P, C, G, STREAM);
}

int vqa_att_apply_gather_fwd(const float* score, const float* vn, const int32_t* img, float* probs, float* out,
                             int64_t out_ld, int N, int B, int P, int C, int G, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_APPLY_FWD, (hipStream_t)stream);
  const int rc = att_apply_check("vqa_att_apply_gather_fwd", false, score && vn && probs && out, img, N, B, P, C, G, out_ld, 0);
  return rc ? rc : att_apply_fwd_launch(score, vn, img, probs, out, out_ld, N, B, P, C, G, STREAM);
}

int vqa_att_apply_bwd(const float* dout, int64_t dout_ld, const float* probs, const float* vn, float* dscore,
                      float* dvn, float* dscore_rowsum, int B, int P, int C, int G, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_APPLY_BWD, (hipStream_t)stream);
  const int rc = att_apply_check("vqa_att_apply_bwd", true, dout && probs && vn && dscore, true, 1, B, P, C, G, dout_ld,
                                 ptr_bits(dout, vn, dvn));
  return rc ? rc : att_apply_bwd_launch(dout, dout_ld, probs, vn, nullptr, nullptr, nullptr, dscore, dvn, dscore_rowsum, 0, B, P,
                                        C, G, STREAM);
}

int vqa_att_apply_gather_bwd(const float* dout, int64_t dout_ld, const float* probs, const float* vn, const int32_t* img,
                             const int32_t* order, const int32_t* offsets, float* dscore, float* dvn, float* dscore_rowsum,
                             int N, int B, int P, int C, int G, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_APPLY_BWD, (hipStream_t)stream);
  const int rc = att_apply_check("vqa_att_apply_gather_bwd", true, dout && probs && vn && dscore && dvn, img && order && offsets,
                                 N, B, P, C, G, dout_ld, ptr_bits(dout, vn, dvn));
  return rc ? rc : att_apply_bwd_launch(dout, dout_ld, probs, vn, img, order, offsets, dscore, dvn, dscore_rowsum, N, B, P, C, G,
                                        STREAM);
}

int vqa_att_apply_gather_dscore(const float* dout, int64_t dout_ld, const float* probs, const float* vn, const int32_t* img,
                                float* dscore, float* dscore_rowsum, int N, int B, int P, int C, int G, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_APPLY_BWD, (hipStream_t)stream);
  const int rc = att_apply_check("vqa_att_apply_gather_dscore", true, dout && probs && vn && dscore, img, N, B, P, C, G, dout_ld,
                                 ptr_bits(dout, vn));
  return rc ? rc : att_apply_bwd_launch(dout, dout_ld, probs, vn, img, nullptr, nullptr, dscore, nullptr, dscore_rowsum, N, B, P,
                                        C, G, STREAM);
}

// ---- gradient x input attribution: vqa_att_apply_gather_dscore's launches, the rows kernel writing r1 too
int vqa_att_attr_apply_gather(const float* dout, int64_t dout_ld, const float* probs, const float* vn, const int32_t* img,
                              float* dscore, float* dscore_rowsum, float* r1, int N, int B, int P, int C, int G,
                              vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_APPLY_BWD, (hipStream_t)stream);
  const int rc = att_apply_check("vqa_att_attr_apply_gather", true, dout && probs && vn && dscore && r1, img, N, B, P, C, G,
                                 dout_ld, ptr_bits(dout, vn));
  return rc ? rc : att_apply_bwd_launch(dout, dout_ld, probs, vn, img, nullptr, nullptr, dscore, nullptr, dscore_rowsum, N, B, P,
                                        C, G, STREAM, r1);
}

int vqa_att_attr_apply_gather_f16(const float* dout, int64_t dout_ld, const float* probs, const void* vn_f16,
                                  const int32_t* img, float* dscore, float* dscore_rowsum, float* r1, int N, int B, int P, int C,
                                  int G, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_APPLY_BWD, (hipStream_t)stream);
  const int rc = att_apply_check("vqa_att_attr_apply_gather_f16", true, dout && probs && vn_f16 && dscore && r1, img, N, B, P, C,
                                 G, dout_ld, ptr_bits(dout));
  if (rc) return rc;
  VQA_REQUIRE((ptr_bits(vn_f16) & (kQuadAlign<__half> - 1)) == 0,
              "vqa_att_attr_apply_gather_f16: vn must be 8-byte aligned");
  return att_apply_bwd_launch(dout, dout_ld, probs, static_cast<const __half*>(vn_f16), img, nullptr, nullptr, dscore, nullptr,
                              dscore_rowsum, N, B, P, C, G, STREAM, r1);
}

// ---- float16 image-feature caches: the gather forward and the dscore backward on a half vn, the same
// launchers, grids, blocks and LDS sizes
int vqa_att_apply_gather_fwd_f16(const float* score, const void* vn_f16, const int32_t* img, float* probs, float* out,
                                 int64_t out_ld, int N, int B, int P, int C, int G, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_APPLY_FWD, (hipStream_t)stream);
  const int rc = att_apply_check("vqa_att_apply_gather_fwd_f16", false, score && vn_f16 && probs && out, img, N, B, P, C, G, out_ld,
                                 0);
  if (rc) return rc;
  VQA_REQUIRE((ptr_bits(vn_f16) & 1) == 0, "vqa_att_apply_gather_fwd_f16: vn must be 2-byte aligned");
  return att_apply_fwd_launch(score, static_cast<const __half*>(vn_f16), img, probs, out, out_ld, N, B, P, C, G, STREAM);
}

int vqa_att_apply_gather_dscore_f16(const float* dout, int64_t dout_ld, const float* probs, const void* vn_f16,
                                    const int32_t* img, float* dscore, float* dscore_rowsum, int N, int B, int P, int C, int G,
                                    vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_APPLY_BWD, (hipStream_t)stream);
  const int rc = att_apply_check("vqa_att_apply_gather_dscore_f16", true, dout && probs && vn_f16 && dscore, img, N, B, P, C, G,
                                 dout_ld, ptr_bits(dout));
  if (rc) return rc;
  // the rows kernel reads a quad of halves as 8 bytes where the fp32 form reads 16
  VQA_REQUIRE((ptr_bits(vn_f16) & (kQuadAlign<__half> - 1)) == 0,
              "vqa_att_apply_gather_dscore_f16: vn must be 8-byte aligned");
  return att_apply_bwd_launch(dout, dout_ld, probs, static_cast<const __half*>(vn_f16), img, nullptr, nullptr, dscore, nullptr,
                              dscore_rowsum, N, B, P, C, G, STREAM);
}

}  // extern "C"
