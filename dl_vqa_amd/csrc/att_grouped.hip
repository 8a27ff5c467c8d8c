// Attention scores for many questions per image (inference, and training through shared image features: the backward
// kernels are at the end of this file): one v' = v_conv(vn) per IMAGE, the questions of an image walked
// over an LDS-resident tile of it.  x = relu(v' (+|*) q') is never written:
//   score[b][g][p] = bx[g] + sum_m wx[g][m] * relu(v'[n*P + p][m] (+|*) q'[b][m])                          n = image of b
//   '|':  score[b][g][p] = (bx[g] + sum_m wx[g][m] * relu(v'[n*P + p][m])) + sum_m wx[g][mid + m] * relu(q'[b][m])
// A workgroup (4 waves) owns TP = 4 * PW consecutive positions of ONE image: the tile [TP][mid] fp32 is copied to LDS once
// (64 KiB at TP = 16, mid = 1024: two workgroups per CU), then every question order[offsets[n] .. offsets[n+1]) of that image
// reads only its q' row (4 KiB, through L2).  HBM traffic: v' once per image instead of x once per question.
// No atomics: a score element is the sum over a lane's channel quads lane*4 + 256*i in ascending i (x, y, z, w inside a quad),
// then the wave butterfly -- the same order whatever the grouping, the tile or the kernel variant.
// DROP (vqa_att_score_grouped_drop_fwd, train mode): x is multiplied by the x_conv dropout mask (models/model.py:194) before
// the product, drop_scale(seed, (b*P + p)*xld + m) over the logical [B][P][xld] tensor x -- indexed by the QUESTION b, as
// vqa_att_score_fwd does; for '|' the q' half takes channel mid + m.  DROP = false is the code the inference entry point runs.
// PAIRS (vqa_att_score_grouped_pairs_fwd, answers from cached question features): pair b reads the q' row qp[qrow[b]] of a
// table [M][mid] of distinct questions; everything else is still indexed by b.  Only the row address changes: the operation
// order above is the same, so the scores equal the PAIRS = false kernels' on the expanded qp[qrow], bit for bit.
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

// the q' row that question / pair b reads, -1: skip b (b outside [0, B); PAIRS: qrow[b] outside [0, M))
template <bool PAIRS>
__device__ __forceinline__ int att_q_row(const int* qrow, int b, int B, int M) {
  if ((unsigned)b >= (unsigned)B) return -1;
  if (!PAIRS) return b;
  const int r = qrow[b];
  return (unsigned)r < (unsigned)M ? r : -1;
}

// '+' / '*', mid = 256 * IT <= 1024: x_conv weights and the question's q' row in registers, 4 positions per wave.
// grid (ceil(P/16), N), 256 threads, 16 * mid floats of dynamic LDS.
__device__ __forceinline__ float4 mul4(const float4 a, const float4 b) {
  return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}

template <int G, int IT, bool MUL, bool DROP, bool PAIRS>
__global__ __launch_bounds__(256) void att_score_grouped_kernel(const float* vprime, const float* qp, const int* qrow, int M,
                                                                const float* wx, int wx_ld, const float* bx, const int* order,
                                                                const int* offsets, float* score, int B, int P, float p,
                                                                float inv_keep, uint64_t seed) {
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
  const int r0 = att_q_row<PAIRS>(qrow, b, B, M);
  bool ok = r0 >= 0;
  if (ok) {
#pragma unroll
    for (int i = 0; i < IT; ++i) q[i] = reinterpret_cast<const float4*>(qp + (int64_t)r0 * mid)[lane + 64 * i];
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
      const int rn = att_q_row<PAIRS>(qrow, bn, B, M);
      okn = rn >= 0;
      if (okn) {
#pragma unroll
        for (int i = 0; i < IT; ++i) qn[i] = reinterpret_cast<const float4*>(qp + (int64_t)rn * mid)[lane + 64 * i];
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
            float4 x = att_combine<MUL>(v, q[i]);
            if (DROP)
              x = mul4(x, drop_scale4(seed, ((uint64_t)b * P + p0 + pl + j) * mid + 4 * (lane + 64 * i), p, inv_keep));
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
template <int G, bool DROP, bool PAIRS>
__global__ __launch_bounds__(256) void att_score_grouped_general_kernel(const float* vprime, const float* qp, const int* qrow,
                                                                        int M, const float* wx, int wx_ld, const float* bx,
                                                                        const int* order, const int* offsets, float* score, int B,
                                                                        int P, int mid, int pw, int mode, float p, float inv_keep,
                                                                        uint64_t seed) {
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
    if (mode == 2 && !DROP) {                             // the v' half does not depend on the question
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
      const int r = att_q_row<PAIRS>(qrow, b, B, M);
      if (r < 0) continue;
      const float4* qv = reinterpret_cast<const float4*>(qp + (int64_t)r * mid);
      float acc[G];
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = 0.f;
      // DROP: element (b, position, channel) of the logical [B][P][xld] tensor x, xld = 2 * mid for '|'
      const uint64_t e0 = ((uint64_t)b * P + p0 + pl) * (mode == 2 ? 2 * mid : mid);
      if (mode == 2) {
        if (DROP) {                                       // train mode: the mask makes the v' half the question's own
          for (int c = lane; c < nq; c += 64) {
            const float4 x = mul4(relu4(vrow[c]), drop_scale4(seed, e0 + 4 * c, p, inv_keep));
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] += dot4(x, reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld)[c]);
          }
#pragma unroll
          for (int g = 0; g < G; ++g) { vpart[g] = wave_sum(acc[g]) + bx[g]; acc[g] = 0.f; }
        }
        for (int c = lane; c < nq; c += 64) {
          float4 x = relu4(qv[c]);
          if (DROP) x = mul4(x, drop_scale4(seed, e0 + mid + 4 * c, p, inv_keep));
#pragma unroll
          for (int g = 0; g < G; ++g) acc[g] += dot4(x, reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld + mid)[c]);
        }
      } else {
        for (int c = lane; c < nq; c += 64) {
          float4 x = mode == 1 ? att_combine<true>(vrow[c], qv[c]) : att_combine<false>(vrow[c], qv[c]);
          if (DROP) x = mul4(x, drop_scale4(seed, e0 + 4 * c, p, inv_keep));
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

// ------------------------------------------------------------------ backward (training through shared image features)
// d loss / d v' (one row per IMAGE position, summed over the image's questions), d loss / d q' and the x_conv weight
// gradient from dscore; x = relu(v' (+|*) q') is recomputed, never read.  With
//   dxpre[b][p][m] = (x > 0) * mask[b][p][m] * sum_g dscore[b][g][p] * wx[g][m]        mask = drop_scale(seed, (b*P + p)*xld + m)
//   '+':  dv'[n*P + p][m] = sum_{b in n} dxpre                dq'[b][m] = sum_p dxpre
//   '*':  dv'[n*P + p][m] = sum_{b in n} dxpre * q'[b][m]     dq'[b][m] = sum_p dxpre * v'[n*P + p][m]
//   '|':  dv' as '+' with x = relu(v') (the v' half);          dq'[b][m] = (q' > 0) * sum_p mask[b][p][mid + m] * sum_g dscore * wx[g][mid + m]
//   dwx[g][m] = sum_{b,p} dscore[b][g][p] * x[b][p][m] * mask[b][p][m]                 (both halves for '|')
// The forward kernel's ownership, turned by 90 degrees: a workgroup owns BTP = 16 consecutive positions of ONE image and walks
// that image's questions, but a THREAD owns one channel quad over all 16 positions (the forward reduces over channels, so its
// lanes share a position; the backward reduces over positions and questions, so its lanes share nothing).  The thread's
// column of the v' tile and of the dv' tile stay in registers across the question walk (2 x 16 float4), no LDS, no barrier:
//   dv'       written once per (image, position), complete;
//   dq_part   [b][tile][mid]: the thread's sum over the tile's positions -- vqa_sum_parts(batch B, parts NT) finishes it;
//   dwx_part  [n*NT + tile][G][xld]: the thread's sum over the tile's positions and the image's questions -- vqa_colsum
//             over the N*NT rows finishes it (the dq_part / dwx_part pattern of vqa_att_score_bwd).
// An image without questions writes zero dv' rows and a zero dwx_part row.  No atomics: every sum has one order (questions in
// `order`'s order, positions ascending, g ascending), whatever the grid.
constexpr int BTP = 16;

template <int G, int MODE, bool DROP>
__device__ __forceinline__ void att_score_bwd_quad(const float* __restrict__ dscore, const float* __restrict__ vprime,
                                                   const float* __restrict__ qp, const float* __restrict__ wx, int wx_ld,
                                                   const int* __restrict__ order, float* __restrict__ dvprime,
                                                   float* __restrict__ dq_part, float* __restrict__ dwx_part, int n, int tile,
                                                   int NT, int rows, int k0, int k1, int B, int P, int mid, int c, float p,
                                                   float inv_keep, uint64_t seed) {
  const int xld = MODE == 2 ? 2 * mid : mid;
  const int p0 = tile * BTP;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 w[G], dw[G], w2[G], dw2[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    w[g] = reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld)[c];
    w2[g] = MODE == 2 ? reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld + mid)[c] : zero;
    dw[g] = zero;
    dw2[g] = zero;
  }
  float4 v[BTP], dv[BTP];
#pragma unroll
  for (int j = 0; j < BTP; ++j) {
    v[j] = zero;
    dv[j] = zero;
    if (j < rows && k0 < k1) v[j] = reinterpret_cast<const float4*>(vprime + ((int64_t)n * P + p0 + j) * mid)[c];
    if (MODE == 2) v[j] = relu4(v[j]);                    // '|': the v' half of x does not depend on the question
  }
  for (int k = k0; k < k1; ++k) {
    const int b = order[k];
    if ((unsigned)b >= (unsigned)B) continue;
    const float4 q = reinterpret_cast<const float4*>(qp + (int64_t)b * mid)[c];
    const float4 rq = relu4(q);
    float4 dq = zero;
#pragma unroll
    for (int j = 0; j < BTP; ++j) {
      if (j < rows) {                                     // workgroup-uniform
        const int64_t m = (int64_t)b * P + p0 + j;
        float ds[G];
#pragma unroll
        for (int g = 0; g < G; ++g) ds[g] = dscore[((int64_t)b * G + g) * P + p0 + j];
        const float4 x = MODE == 2 ? v[j] : att_combine<MODE == 1>(v[j], q);
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
        if (DROP) sc = drop_scale4(seed, (uint64_t)m * xld + 4 * c, p, inv_keep);
        float4 t = zero;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          t.x += ds[g] * w[g].x; t.y += ds[g] * w[g].y; t.z += ds[g] * w[g].z; t.w += ds[g] * w[g].w;
          dw[g].x += ds[g] * x.x * sc.x; dw[g].y += ds[g] * x.y * sc.y; dw[g].z += ds[g] * x.z * sc.z; dw[g].w += ds[g] * x.w * sc.w;
        }
        float4 d;
        d.x = x.x > 0.f ? t.x * sc.x : 0.f; d.y = x.y > 0.f ? t.y * sc.y : 0.f;
        d.z = x.z > 0.f ? t.z * sc.z : 0.f; d.w = x.w > 0.f ? t.w * sc.w : 0.f;
        if (MODE == 0) {
          dq.x += d.x; dq.y += d.y; dq.z += d.z; dq.w += d.w;
          dv[j].x += d.x; dv[j].y += d.y; dv[j].z += d.z; dv[j].w += d.w;
        } else if (MODE == 1) {
          dq.x += d.x * v[j].x; dq.y += d.y * v[j].y; dq.z += d.z * v[j].z; dq.w += d.w * v[j].w;
          dv[j].x += d.x * q.x; dv[j].y += d.y * q.y; dv[j].z += d.z * q.z; dv[j].w += d.w * q.w;
        } else {
          dv[j].x += d.x; dv[j].y += d.y; dv[j].z += d.z; dv[j].w += d.w;
          float4 s2 = make_float4(1.f, 1.f, 1.f, 1.f);
          if (DROP) s2 = drop_scale4(seed, (uint64_t)m * xld + mid + 4 * c, p, inv_keep);
          float4 t2 = zero;
#pragma unroll
          for (int g = 0; g < G; ++g) {
            t2.x += ds[g] * w2[g].x; t2.y += ds[g] * w2[g].y; t2.z += ds[g] * w2[g].z; t2.w += ds[g] * w2[g].w;
            dw2[g].x += ds[g] * rq.x * s2.x; dw2[g].y += ds[g] * rq.y * s2.y; dw2[g].z += ds[g] * rq.z * s2.z; dw2[g].w += ds[g] * rq.w * s2.w;
          }
          dq.x += q.x > 0.f ? t2.x * s2.x : 0.f; dq.y += q.y > 0.f ? t2.y * s2.y : 0.f;
          dq.z += q.z > 0.f ? t2.z * s2.z : 0.f; dq.w += q.w > 0.f ? t2.w * s2.w : 0.f;
        }
      }
    }
    reinterpret_cast<float4*>(dq_part + ((int64_t)b * NT + tile) * mid)[c] = dq;
  }
#pragma unroll
  for (int j = 0; j < BTP; ++j)
    if (j < rows) reinterpret_cast<float4*>(dvprime + ((int64_t)n * P + p0 + j) * mid)[c] = dv[j];
  const int64_t part = (int64_t)n * NT + tile;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    reinterpret_cast<float4*>(dwx_part + (part * G + g) * xld)[c] = dw[g];
    if (MODE == 2) reinterpret_cast<float4*>(dwx_part + (part * G + g) * xld + mid)[c] = dw2[g];
  }
}

// '+' / '*', mid = 256 * IT <= 1024: one channel quad per thread, 64 * IT threads, every stride a compile-time constant.
// grid (ceil(P/16), N).
template <int G, int IT, bool MUL, bool DROP>
__global__ __launch_bounds__(64 * IT) void att_score_grouped_bwd_kernel(const float* dscore, const float* vprime, const float* qp,
                                                                         const float* wx, int wx_ld, const int* order,
                                                                         const int* offsets, float* dvprime, float* dq_part,
                                                                         float* dwx_part, int B, int P, float p, float inv_keep,
                                                                         uint64_t seed) {
  constexpr int mid = 256 * IT;
  const int n = blockIdx.y, tile = blockIdx.x;
  int k0, k1;
  att_group_range(offsets, n, B, k0, k1);
  att_score_bwd_quad<G, MUL ? 1 : 0, DROP>(dscore, vprime, qp, wx, wx_ld, order, dvprime, dq_part, dwx_part, n, tile, gridDim.x,
                                          min(BTP, P - tile * BTP), k0, k1, B, P, mid, threadIdx.x, p, inv_keep, seed);
}

// Any mid % 4 == 0 and every mode: the same body under a run-time walk over the thread's channel quads (tid, tid + 256, ...).
template <int G, int MODE, bool DROP>
__global__ __launch_bounds__(256) void att_score_grouped_bwd_general_kernel(const float* dscore, const float* vprime,
                                                                            const float* qp, const float* wx, int wx_ld,
                                                                            const int* order, const int* offsets, float* dvprime,
                                                                            float* dq_part, float* dwx_part, int B, int P, int mid,
                                                                            float p, float inv_keep, uint64_t seed) {
  const int n = blockIdx.y, tile = blockIdx.x;
  int k0, k1;
  att_group_range(offsets, n, B, k0, k1);
  const int rows = min(BTP, P - tile * BTP);
  for (int c = threadIdx.x; c < (mid >> 2); c += 256)
    att_score_bwd_quad<G, MODE, DROP>(dscore, vprime, qp, wx, wx_ld, order, dvprime, dq_part, dwx_part, n, tile, gridDim.x, rows,
                                      k0, k1, B, P, mid, c, p, inv_keep, seed);
}

}  // namespace vqa

using namespace vqa;

// what the four entry points check (`who` names the caller in the messages); `rest` is the entry point's own data pointers
// beside vprime, qp and wx: all non-null, and 16-byte aligned where `quads` holds their bits
#define GROUPED_REQUIRE(who, rest, quads)                                                                                         \
  VQA_REQUIRE(G >= 1 && G <= 4, "glimpses=%d unsupported (1..4)", G);                                                             \
  VQA_REQUIRE(mode >= 0 && mode <= 2, who ": mode %d (0 '+', 1 '*', 2 '|')", mode);                                               \
  VQA_REQUIRE(vprime && qp && wx && (rest), who ": null pointer");                                                                \
  VQA_REQUIRE(order && offsets, who ": null order / offsets");                                                                    \
  VQA_REQUIRE(N >= 1 && N <= 65535 && B >= 0 && P >= 1, who ": N=%d (1..65535), B=%d, P=%d out of range", N, B, P);               \
  VQA_REQUIRE(mid >= 4 && mid % 4 == 0 && wx_ld % 4 == 0 && wx_ld >= (mode == 2 ? 2 * mid : mid),                                 \
              who ": bad args (mid=%d and wx_ld=%d must be multiples of 4, wx_ld >= channels of x)", mid, wx_ld);                 \
  VQA_REQUIRE(mid <= 4096, who ": mid=%d too large (the forward's LDS tile: 4 rows x mid fp32 <= 64 KiB)", mid);                  \
  VQA_REQUIRE(((reinterpret_cast<uintptr_t>(vprime) | reinterpret_cast<uintptr_t>(qp) | reinterpret_cast<uintptr_t>(wx) |         \
                (uintptr_t)(quads)) & 15) == 0, who ": vprime, qp, wx and the outputs read as quads must be 16-byte aligned")
#define GROUPED_FWD_REQUIRE(who) GROUPED_REQUIRE(who, bx && score, 0)

// the launch of the forward entry points: p == 0 runs the DROP = false kernels, the inference entry point's code; qrow != NULL
// (inference only, p == 0) runs their PAIRS instantiations over the q' table qp [M][mid]
static int grouped_fwd_launch(const float* vprime, const float* qp, const int32_t* qrow, int M, const float* wx, int wx_ld,
                              const float* bx, const int32_t* order, const int32_t* offsets, float* score, int N, int B, int P,
                              int mid, int G, int mode, float p, uint64_t seed, hipStream_t s) {
  const float ik = keep_scale(p);
  const bool pairs = qrow != nullptr;              // the pairs entry point passes p = 0: DROP x PAIRS is never instantiated
  if (mode != 2 && mid % 256 == 0 && mid <= 1024) {
    const dim3 grid((P + 15) / 16, N);
    const size_t lds = (size_t)16 * mid * 4;
    with_int14(G, [&](auto g) {
      return with_int14(mid / 256, [&](auto it) {
        return with_flags(mode == 1, pairs ? false : p > 0.f, [&](auto mul, auto drop) {
          if (pairs)
            hipLaunchKernelGGL((att_score_grouped_kernel<decltype(g)::value, decltype(it)::value, decltype(mul)::value, false,
                                                         true>),
                               grid, dim3(256), lds, s, vprime, qp, qrow, M, wx, wx_ld, bx, order, offsets, score, B, P, 0.f, 1.f,
                               (uint64_t)0);
          else
            hipLaunchKernelGGL((att_score_grouped_kernel<decltype(g)::value, decltype(it)::value, decltype(mul)::value,
                                                         decltype(drop)::value, false>),
                               grid, dim3(256), lds, s, vprime, qp, qrow, M, wx, wx_ld, bx, order, offsets, score, B, P, p, ik,
                               seed);
          return 0;
        });
      });
    });
    return check_hip(hipGetLastError(), "att_score_grouped_fwd launch");
  }
  const int pw = mid <= 1024 ? 4 : (mid <= 2048 ? 2 : 1);      // 4 * pw rows of mid floats <= 64 KiB
  const int TP = 4 * pw;
  const dim3 grid((P + TP - 1) / TP, N);
  const size_t lds = (size_t)TP * mid * 4;
  with_int14(G, [&](auto g) {
    return with_flag(pairs ? false : p > 0.f, [&](auto drop) {
      if (pairs)
        hipLaunchKernelGGL((att_score_grouped_general_kernel<decltype(g)::value, false, true>), grid, dim3(256), lds, s, vprime,
                           qp, qrow, M, wx, wx_ld, bx, order, offsets, score, B, P, mid, pw, mode, 0.f, 1.f, (uint64_t)0);
      else
        hipLaunchKernelGGL((att_score_grouped_general_kernel<decltype(g)::value, decltype(drop)::value, false>), grid, dim3(256),
                           lds, s, vprime, qp, qrow, M, wx, wx_ld, bx, order, offsets, score, B, P, mid, pw, mode, p, ik, seed);
      return 0;
    });
  });
  return check_hip(hipGetLastError(), "att_score_grouped_fwd launch");
}

extern "C" {

int vqa_att_score_grouped_fwd(const float* vprime, const float* qp, const float* wx, int wx_ld, const float* bx,
                              const int32_t* order, const int32_t* offsets, float* score, int N, int B, int P, int mid, int G,
                              int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_FWD, (hipStream_t)stream);
  GROUPED_FWD_REQUIRE("vqa_att_score_grouped_fwd");
  if (B == 0) return VQA_OK;
  return grouped_fwd_launch(vprime, qp, nullptr, 0, wx, wx_ld, bx, order, offsets, score, N, B, P, mid, G, mode, 0.f, 0,
                            (hipStream_t)stream);
}

int vqa_att_score_grouped_pairs_fwd(const float* vprime, const float* qp, const int32_t* qrow, const float* wx, int wx_ld,
                                    const float* bx, const int32_t* order, const int32_t* offsets, float* score, int N, int B,
                                    int M, int P, int mid, int G, int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_FWD, (hipStream_t)stream);
  GROUPED_FWD_REQUIRE("vqa_att_score_grouped_pairs_fwd");
  VQA_REQUIRE(qrow, "vqa_att_score_grouped_pairs_fwd: null qrow");
  VQA_REQUIRE(M >= 1, "vqa_att_score_grouped_pairs_fwd: M=%d question rows (>= 1)", M);
  if (B == 0) return VQA_OK;
  return grouped_fwd_launch(vprime, qp, qrow, M, wx, wx_ld, bx, order, offsets, score, N, B, P, mid, G, mode, 0.f, 0,
                            (hipStream_t)stream);
}

int vqa_att_score_grouped_drop_fwd(const float* vprime, const float* qp, const float* wx, int wx_ld, const float* bx,
                                   const int32_t* order, const int32_t* offsets, float* score, int N, int B, int P, int mid,
                                   int G, int mode, float p, uint64_t seed, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_FWD, (hipStream_t)stream);
  GROUPED_FWD_REQUIRE("vqa_att_score_grouped_drop_fwd");
  VQA_REQUIRE(p >= 0.f && p < 1.f, "vqa_att_score_grouped_drop_fwd: dropout p=%g outside [0, 1)", (double)p);
  if (B == 0) return VQA_OK;
  return grouped_fwd_launch(vprime, qp, nullptr, 0, wx, wx_ld, bx, order, offsets, score, N, B, P, mid, G, mode, p, seed,
                            (hipStream_t)stream);
}

int vqa_att_score_grouped_tiles(int P) { return P < 1 ? 1 : (P + BTP - 1) / BTP; }

int vqa_att_score_grouped_bwd(const float* dscore, const float* vprime, const float* qp, const float* wx, int wx_ld,
                              const int32_t* order, const int32_t* offsets, float* dvprime, float* dq_part, float* dwx_part,
                              int N, int B, int P, int mid, int G, int mode, float p, uint64_t seed, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_BWD, (hipStream_t)stream);
  GROUPED_REQUIRE("vqa_att_score_grouped_bwd", dscore && dvprime && dq_part && dwx_part,
                  reinterpret_cast<uintptr_t>(dvprime) | reinterpret_cast<uintptr_t>(dq_part) | reinterpret_cast<uintptr_t>(dwx_part));
  VQA_REQUIRE(p >= 0.f && p < 1.f, "vqa_att_score_grouped_bwd: dropout p=%g outside [0, 1)", (double)p);
  if (B == 0) return VQA_OK;
  hipStream_t s = (hipStream_t)stream;
  const float ik = keep_scale(p);
  const dim3 grid(vqa_att_score_grouped_tiles(P), N);
  if (mode != 2 && mid % 256 == 0 && mid <= 1024) {
    with_int14(G, [&](auto g) {
      return with_int14(mid / 256, [&](auto it) {
        return with_flags(mode == 1, p > 0.f, [&](auto mul, auto drop) {
          hipLaunchKernelGGL((att_score_grouped_bwd_kernel<decltype(g)::value, decltype(it)::value, decltype(mul)::value,
                                                           decltype(drop)::value>),
                             grid, dim3(64 * decltype(it)::value), 0, s, dscore, vprime, qp, wx, wx_ld, order, offsets, dvprime,
                             dq_part, dwx_part, B, P, p, ik, seed);
          return 0;
        });
      });
    });
    return check_hip(hipGetLastError(), "att_score_grouped_bwd launch");
  }
#define GROUPED_BWD_GENERAL(kMODE)                                                                                                \
  with_int14(G, [&](auto g) {                                                                                                     \
    return with_flag(p > 0.f, [&](auto drop) {                                                                                    \
      hipLaunchKernelGGL((att_score_grouped_bwd_general_kernel<decltype(g)::value, kMODE, decltype(drop)::value>), grid,          \
                         dim3(256), 0, s, dscore, vprime, qp, wx, wx_ld, order, offsets, dvprime, dq_part, dwx_part, B, P, mid,   \
                         p, ik, seed);                                                                                            \
      return 0;                                                                                                                   \
    });                                                                                                                           \
  })
  if (mode == 0) GROUPED_BWD_GENERAL(0);
  else if (mode == 1) GROUPED_BWD_GENERAL(1);
  else GROUPED_BWD_GENERAL(2);
#undef GROUPED_BWD_GENERAL
  return check_hip(hipGetLastError(), "att_score_grouped_bwd launch");
}

}  // extern "C"
