// Attention scores (x_conv), plain and grouped, forward and backward: every kernel and entry point of the score half of the
// attention stage.  The plain forms read x = relu(v' (+|*) q') as the GEMM epilogue wrote it, one row per (question,
// position); the grouped forms (many questions per image: inference, and training through shared image features) never
// write x.  Shared by both: the per-quad element math (att_combine, relu4, mul4, dot4), the backward element body
// (att_score_bwd_dx), and on the host one argument check (att_score_check) and one path choice per family
// (att_score_fwd_path, att_score_grouped_pw).  The forward kernels each keep their own accumulate and write-out
// (wave_sum per glimpse, lane 0 stores + bias): helpers for them move the instruction schedule of kernels whose arithmetic
// they do not touch, the pool_pick rule of common.hpp.
//
// Grouped forms: one v' = v_conv(vn) per IMAGE, the questions of an image walked over an LDS-resident tile of it:
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
// Attribution (vqa_att_attr_score_grouped*, inference): the same ownership and walk turned to the gradient x input map of a
// question -- see the section "grouped attribution" below.  vqa_att_attr_dq_grouped* (the gradient of one logit at q' through
// the scores, for the per-token map): the grouped backward's body under DQ_ONLY -- see "grouped backward" below.
#include "common.hpp"
#include "cache_load.hpp"

namespace vqa {

// ------------------------------------------------------------------ element math on channel quads
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
__device__ __forceinline__ float4 mul4(const float4 a, const float4 b) {
  return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}
__device__ __forceinline__ float dot4(const float4 x, const float4 w) { return x.x * w.x + x.y * w.y + x.z * w.z + x.w * w.w; }

// 4 consecutive elements of an fp32 or bf16 row, as floats
template <bool XB>
__device__ __forceinline__ float4 ld4(const void* row, int c) {
  if (XB) {
    const uint2 w = reinterpret_cast<const uint2*>(row)[c];
    return make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
                       __uint_as_float(w.y & 0xffff0000u));
  }
  return reinterpret_cast<const float4*>(row)[c];
}
template <bool XB>
__device__ __forceinline__ void st4(void* row, int c, float4 v) {
  if (XB) reinterpret_cast<uint2*>(row)[c] = make_uint2(f2bf16_pair(v.x, v.y), f2bf16_pair(v.z, v.w));
  else reinterpret_cast<float4*>(row)[c] = v;
}

// The backward of one quad of one row, for the plain and the grouped kernels alike.  With ds = dscore[b][:][p], x the quad
// of relu(...) and sc its dropout scales:  dw[g] += ds[g] * x * sc  (the x_conv weight gradient);  returns
// d = (x > 0) * sc * sum_g ds[g] * w[g], the gradient at the pre-activation.  What d becomes (dq', dv', the in-place
// store, the '*' factors) differs per kernel and mode and stays at the call sites.  DW = false (the attribution form
// vqa_att_attr_dq_grouped, which wants d alone): the dw lines are not compiled; d is the same expression either way.
template <int G, bool DW = true>
__device__ __forceinline__ float4 att_score_bwd_dx(const float (&ds)[G], const float4 (&w)[G], const float4 x, const float4 sc,
                                                   float4 (&dw)[G]) {
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (DW) {
      t.x += ds[g] * w[g].x; t.y += ds[g] * w[g].y; t.z += ds[g] * w[g].z; t.w += ds[g] * w[g].w;
    } else {                                              // the fused multiply-adds hipcc contracts the line above to
      t.x = fmaf(ds[g], w[g].x, t.x); t.y = fmaf(ds[g], w[g].y, t.y); t.z = fmaf(ds[g], w[g].z, t.z); t.w = fmaf(ds[g], w[g].w, t.w);
    }
    if (DW) {
      dw[g].x += ds[g] * x.x * sc.x; dw[g].y += ds[g] * x.y * sc.y; dw[g].z += ds[g] * x.z * sc.z; dw[g].w += ds[g] * x.w * sc.w;
    }
  }
  float4 d;
  d.x = x.x > 0.f ? t.x * sc.x : 0.f; d.y = x.y > 0.f ? t.y * sc.y : 0.f;
  d.z = x.z > 0.f ? t.z * sc.z : 0.f; d.w = x.w > 0.f ? t.w * sc.w : 0.f;
  return d;
}
// '|': the q' half of the same row (q the quad of q', rq = relu(q), s2 its dropout scales, w2 = wx[g][mid + ...]).  The
// grouped body takes it; att_score_bwd_kernel spells the same lines out (see there).
template <int G>
__device__ __forceinline__ void att_score_bwd_qhalf(const float (&ds)[G], const float4 (&w2)[G], const float4 q, const float4 rq,
                                                    const float4 s2, float4 (&dw2)[G], float4& dq) {
  float4 t2 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    t2.x += ds[g] * w2[g].x; t2.y += ds[g] * w2[g].y; t2.z += ds[g] * w2[g].z; t2.w += ds[g] * w2[g].w;
    dw2[g].x += ds[g] * rq.x * s2.x; dw2[g].y += ds[g] * rq.y * s2.y; dw2[g].z += ds[g] * rq.z * s2.z; dw2[g].w += ds[g] * rq.w * s2.w;
  }
  dq.x += q.x > 0.f ? t2.x * s2.x : 0.f; dq.y += q.y > 0.f ? t2.y * s2.y : 0.f;
  dq.z += q.z > 0.f ? t2.z * s2.z : 0.f; dq.w += q.w > 0.f ? t2.w * s2.w : 0.f;
}

// ------------------------------------------------------------------ plain forward
// x = relu(v' (+|*) q') is xs [M][mid]; for do_option '|' x = relu(cat[v', tile(q')]) has 2*mid channels:
// the v' half is xs, the q' half is relu(qcat[b][:]) replicated over positions (but with its own
// per-position dropout mask, as nn.Dropout acts on the concatenated tensor).  xld = channels of x.
// XB: xs holds bf16 (the bf16 path stores x = relu(v' (+|*) q') as bf16)
template <int G, bool XB>
__global__ void att_score_fwd_kernel(const void* xs, const float* wx, int wx_ld, const float* bx, float* score,
                                     int64_t M, int P, int mid, float p, float inv_keep, uint64_t seed,
                                     const float* qcat) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int nch = mid >> 2;
  const int xld = qcat ? 2 * mid : mid;
  for (int64_t m = wave; m < M; m += nwaves) {
    const int64_t b = m / P;
    const int pp = (int)(m - b * P);
    const char* row = static_cast<const char*>(xs) + m * mid * (XB ? 2 : 4);
    float acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = 0.f;
    for (int c = lane; c < nch; c += 64) {
      float4 x = ld4<XB>(row, c);
      if (p > 0.f) x = mul4(x, drop_scale4(seed, (uint64_t)m * xld + 4 * c, p, inv_keep));
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float4 w = reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld)[c];
        acc[g] += x.x * w.x + x.y * w.y + x.z * w.z + x.w * w.w;
      }
      if (qcat) {
        float4 q = relu4(reinterpret_cast<const float4*>(qcat + b * mid)[c]);
        if (p > 0.f) q = mul4(q, drop_scale4(seed, (uint64_t)m * xld + mid + 4 * c, p, inv_keep));
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float4 w = reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld + mid)[c];
          acc[g] += q.x * w.x + q.y * w.y + q.z * w.z + q.w * w.w;
        }
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float v = wave_sum(acc[g]);
      if (lane == 0) score[(b * G + g) * P + pp] = v + bx[g];
    }
  }
}

// fp32 x without the concatenated half, mid a multiple of 256 up to 1024 (the reference's 1024): the general kernel above walks
// a row in mid/256 DEPENDENT rounds of 16-byte loads with one row per wave in flight and re-reads the x_conv weights for every
// row (3.9 TB/s).  Here a lane issues all IT loads of a row before it touches the first value, the next row's loads are issued
// before the current row is reduced, and the weights live in registers.  Same per-lane operation order as the general kernel.
template <int G, int IT>
__global__ __launch_bounds__(256) void att_score_fwd_rows_kernel(const float* xs, const float* wx, int wx_ld, const float* bx,
                                                                 float* score, int64_t M, int P, float p, float inv_keep,
                                                                 uint64_t seed) {
  constexpr int mid = 256 * IT;
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  float4 w[IT][G];
  float bias[G];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int g = 0; g < G; ++g) w[i][g] = reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld)[lane + 64 * i];
#pragma unroll
  for (int g = 0; g < G; ++g) bias[g] = bx[g];
  float4 cur[IT], nxt[IT];
  int64_t m = wave;
  if (m < M) {
#pragma unroll
    for (int i = 0; i < IT; ++i) cur[i] = reinterpret_cast<const float4*>(xs + m * mid)[lane + 64 * i];
  }
  for (; m < M; m += nwaves) {
    const int64_t mn = m + nwaves;
    if (mn < M) {
#pragma unroll
      for (int i = 0; i < IT; ++i) nxt[i] = reinterpret_cast<const float4*>(xs + mn * mid)[lane + 64 * i];
    }
    float acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = 0.f;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      float4 x = cur[i];
      if (p > 0.f) {
        const uint64_t e = (uint64_t)m * mid + 4 * (lane + 64 * i);
        const float4 ds_ = drop_scale4(seed, e, p, inv_keep);
        x.x *= ds_.x; x.y *= ds_.y; x.z *= ds_.z; x.w *= ds_.w;
      }
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] += x.x * w[i][g].x + x.y * w[i][g].y + x.z * w[i][g].z + x.w * w[i][g].w;
    }
    const int64_t b = m / P;
    const int pp = (int)(m - b * P);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float v = wave_sum(acc[g]);
      if (lane == 0) score[(b * G + g) * P + pp] = v + bias[g];
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) cur[i] = nxt[i];
  }
}

// The bf16 path's form of the above (x = relu(v' (+|*) q') stored as bf16, no concatenated half, mid <= 1024): the generic
// kernel walked a row in four dependent rounds of 8-byte loads and re-read the x_conv weights for every row -- 2.3 TB/s.  Here
// a lane owns 8 channels per round (16-byte loads), keeps its weights in registers for the whole kernel, and a wave has the
// loads of TWO rows in flight before it touches the first value.  (Eight channels per lane and round, so the quad helpers
// above do not fit its element math; the write-out is the shared one.)
template <int G>
__global__ __launch_bounds__(256) void att_score_fwd_bf16_kernel(const uint16_t* xs, const float* wx, int wx_ld, const float* bx,
                                                                 float* score, int64_t M, int P, int mid, float p, float inv_keep,
                                                                 uint64_t seed) {
  constexpr int IT = 2;                                   // rounds of 64 lanes x 8 channels: mid <= 1024
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int n8 = mid >> 3;
  float w[IT][G][8];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int c8 = lane + 64 * i;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int k = 0; k < 8; ++k) w[i][g][k] = c8 < n8 ? wx[(int64_t)g * wx_ld + 8 * c8 + k] : 0.f;
  }
  float bias[G];
#pragma unroll
  for (int g = 0; g < G; ++g) bias[g] = bx[g];
  for (int64_t m0 = 2 * wave; m0 < M; m0 += 2 * nwaves) {
    uint4 xr[2][IT];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        const int c8 = lane + 64 * i;
        xr[rr][i] = (m0 + rr < M && c8 < n8) ? *reinterpret_cast<const uint4*>(xs + (m0 + rr) * mid + 8 * c8) : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int64_t m = m0 + rr;
      float acc[G];
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = 0.f;
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        const int c8 = lane + 64 * i;
        const uint32_t u[4] = {xr[rr][i].x, xr[rr][i].y, xr[rr][i].z, xr[rr][i].w};
        float x[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) { x[2 * k] = __uint_as_float(u[k] << 16); x[2 * k + 1] = __uint_as_float(u[k] & 0xffff0000u); }
        if (p > 0.f) {
          const uint64_t e = (uint64_t)m * mid + 8 * c8;
          const float4 s0 = drop_scale4(seed, e, p, inv_keep), s1 = drop_scale4(seed, e + 4, p, inv_keep);
          x[0] *= s0.x; x[1] *= s0.y; x[2] *= s0.z; x[3] *= s0.w; x[4] *= s1.x; x[5] *= s1.y; x[6] *= s1.z; x[7] *= s1.w;
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[g] += x[k] * w[i][g][k];
      }
      if (m < M) {
        const int64_t b = m / P;
        const int pp = (int)(m - b * P);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float v = wave_sum(acc[g]);
          if (lane == 0) score[(b * G + g) * P + pp] = v + bias[g];
        }
      }
    }
  }
}

// ------------------------------------------------------------------ plain backward
// grid (B, RS); thread -> float4 column chunks; loops the rows of its split.
// mode 0 '+': xs <- dz = (x>0) * mask * sum_g ds*wx            dq' part = sum_p dz
// mode 1 '*': xs <- dv' = dz * q'[b]                             dq' part = sum_p dz * v'
// mode 2 '|': xs <- dv' = dz (v' half);  q' half: dq' part = (q'>0) * sum_p mask_q * sum_g ds*wx[g][mid+n]
// dwx_part[part][G][xld]: sum_p ds[g] * dropout(x) over the rows of the part (both halves for '|').
template <int G, bool XB>
__global__ void att_score_bwd_kernel(const float* dscore, const float* wx, int wx_ld, void* xs, float* dwx_part,
                                     float* dq_part, int P, int mid, int RS, float p, float inv_keep, uint64_t seed,
                                     int mode, const float* vprime, const float* qp) {
  const int b = blockIdx.x, rs = blockIdx.y;
  const int rows_per = (P + RS - 1) / RS;
  const int p0 = rs * rows_per, p1 = min(P, p0 + rows_per);
  const int nch = mid >> 2;
  const int xld = mode == 2 ? 2 * mid : mid;
  const int64_t part = (int64_t)b * RS + rs;
  for (int c = threadIdx.x; c < nch; c += blockDim.x) {
    float4 w[G], dw[G], w2[G], dw2[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      w[g] = reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld)[c];
      dw[g] = make_float4(0.f, 0.f, 0.f, 0.f);
      dw2[g] = make_float4(0.f, 0.f, 0.f, 0.f);
      w2[g] = mode == 2 ? reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld + mid)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 qv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mode != 0) qv = reinterpret_cast<const float4*>(qp + (int64_t)b * mid)[c];
    const float4 rq = relu4(qv);
    float4 dq = make_float4(0.f, 0.f, 0.f, 0.f);
    // rows in batches of four: the four loads of x (and the batch's dscore values) are issued before the first of them is
    // used -- xs is rewritten in place, so hipcc may not move a row's load above the previous row's store by itself, and one
    // dependent load -> compute -> store chain per row left the kernel at 4 TB/s
    for (int pb = p0; pb < p1; pb += 4) {
      float4 xb[4];
      float dsb[4][G];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int pp = pb + u < p1 ? pb + u : p1 - 1;
        const int64_t m = (int64_t)b * P + pp;
        xb[u] = ld4<XB>(static_cast<const char*>(xs) + m * mid * (XB ? 2 : 4), c);
#pragma unroll
        for (int g = 0; g < G; ++g) dsb[u][g] = dscore[((int64_t)b * G + g) * P + pp];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
      const int pp = pb + u;
      if (pp >= p1) break;
      const int64_t m = (int64_t)b * P + pp;
      char* xrow = static_cast<char*>(xs) + m * mid * (XB ? 2 : 4);
      const float4 x = xb[u];
      float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
      if (p > 0.f) {
        const uint64_t e = (uint64_t)m * xld + 4 * c;
        sc = drop_scale4(seed, e, p, inv_keep);
      }
      float ds[G];
#pragma unroll
      for (int g = 0; g < G; ++g) ds[g] = dsb[u][g];
      float4 d = att_score_bwd_dx<G>(ds, w, x, sc, dw);
      if (mode == 0) {
        dq.x += d.x; dq.y += d.y; dq.z += d.z; dq.w += d.w;
      } else if (mode == 1) {
        const float4 vp = reinterpret_cast<const float4*>(vprime + m * mid)[c];
        dq.x += d.x * vp.x; dq.y += d.y * vp.y; dq.z += d.z * vp.z; dq.w += d.w * vp.w;
        d = mul4(d, qv);
      } else {
        float4 s2 = make_float4(1.f, 1.f, 1.f, 1.f);
        if (p > 0.f) {
          const uint64_t e = (uint64_t)m * xld + mid + 4 * c;
          s2 = drop_scale4(seed, e, p, inv_keep);
        }
        // its own spelling: att_score_bwd_qhalf here re-schedules all eight instantiations of this kernel
        float4 t2 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          t2.x += ds[g] * w2[g].x; t2.y += ds[g] * w2[g].y; t2.z += ds[g] * w2[g].z; t2.w += ds[g] * w2[g].w;
          dw2[g].x += ds[g] * rq.x * s2.x; dw2[g].y += ds[g] * rq.y * s2.y; dw2[g].z += ds[g] * rq.z * s2.z; dw2[g].w += ds[g] * rq.w * s2.w;
        }
        dq.x += qv.x > 0.f ? t2.x * s2.x : 0.f; dq.y += qv.y > 0.f ? t2.y * s2.y : 0.f;
        dq.z += qv.z > 0.f ? t2.z * s2.z : 0.f; dq.w += qv.w > 0.f ? t2.w * s2.w : 0.f;
      }
      st4<XB>(xrow, c, d);
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      reinterpret_cast<float4*>(dwx_part + (part * G + g) * xld)[c] = dw[g];
      if (mode == 2) reinterpret_cast<float4*>(dwx_part + (part * G + g) * xld + mid)[c] = dw2[g];
    }
    reinterpret_cast<float4*>(dq_part + part * mid)[c] = dq;
  }
}

// ------------------------------------------------------------------ grouped forward
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

// The same walk over a float16 v' (a float16 image-feature cache, cache_load.hpp): a quad of halves is one 8-byte load,
// widened here -- the one place v' enters the grouped forward kernels -- so the LDS tile is fp32 either way and everything
// behind it is the same code.  (An overload, not a template over both: the fp32 loader above keeps its code.)
__device__ __forceinline__ void att_tile_to_lds(const __half* vprime, float* tile, int64_t row0, int rows, int mid) {
  const __half* src = vprime + row0 * mid;
  float4* dst = reinterpret_cast<float4*>(tile);
  const int n4 = rows * (mid >> 2);
  int i = threadIdx.x;
  for (; i + 768 < n4; i += 1024) {          // four loads in flight per thread
    float4 t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) t[u] = load_quad(src, i + 256 * u);
#pragma unroll
    for (int u = 0; u < 4; ++u) dst[i + 256 * u] = t[u];
  }
  for (; i < n4; i += 256) dst[i] = load_quad(src, i);
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
// VT: v' is fp32, or fp16 for a float16 image-feature cache (vqa_att_score_grouped_fwd_f16 / _pairs_fwd_f16: inference, DROP = false)
template <int G, int IT, bool MUL, bool DROP, bool PAIRS, class VT = float>
__global__ __launch_bounds__(256) void att_score_grouped_kernel(const VT* vprime, const float* qp, const int* qrow, int M,
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
  float bias[G];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int g = 0; g < G; ++g) w[i][g] = reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld)[lane + 64 * i];
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
template <int G, bool DROP, bool PAIRS, class VT = float>
__global__ __launch_bounds__(256) void att_score_grouped_general_kernel(const VT* vprime, const float* qp, const int* qrow,
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
      // its own write-out: for '|' the bias is already inside vpart, a register array that att_score_store's `bias` cannot
      // alias with bx without going through memory
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float s = wave_sum(acc[g]);
        if (lane == 0) score[((int64_t)b * G + g) * P + p0 + pl] = mode == 2 ? vpart[g] + s : s + bx[g];
      }
    }
  }
}

// ------------------------------------------------------------------ grouped attribution (gradient x input at vn, inference)
// R[b][p] = r1[b][p] + sum_m c[b][p][m] * s[b][p][m] * v'[n*P + p][m] with c = sum_g dscore[b][g][p] * wx[g][m] and s the
// derivative of x = relu(v' (+|*) q') by v' (include/vqa_hip.h): the score path of the map, v_conv folded away because
// vn . Wv^T is the cached v' itself.  The grouped forward's ownership and walk (a workgroup: a tile of positions of ONE
// image in LDS, the image's questions streamed past it, lanes reduce over mid), with dscore where the forward has nothing
// and r1 where it has the bias.  One quad's term, for every kernel and mode: c in g-ascending order, then
// c.x*s.x*v.x + ... in x, y, z, w order; a lane sums its quads lane + 64*i in ascending i, then the wave butterfly.
template <int G, int MODE>
__device__ __forceinline__ float att_attr_quad(const float (&ds)[G], const float4 (&w)[G], const float4 v, const float4 q) {
  float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int g = 0; g < G; ++g) { c.x += ds[g] * w[g].x; c.y += ds[g] * w[g].y; c.z += ds[g] * w[g].z; c.w += ds[g] * w[g].w; }
  float4 s;
  if (MODE == 0) {
    s.x = v.x + q.x > 0.f ? 1.f : 0.f; s.y = v.y + q.y > 0.f ? 1.f : 0.f;
    s.z = v.z + q.z > 0.f ? 1.f : 0.f; s.w = v.w + q.w > 0.f ? 1.f : 0.f;
  } else if (MODE == 1) {
    s.x = v.x * q.x > 0.f ? q.x : 0.f; s.y = v.y * q.y > 0.f ? q.y : 0.f;
    s.z = v.z * q.z > 0.f ? q.z : 0.f; s.w = v.w * q.w > 0.f ? q.w : 0.f;
  } else {
    s.x = v.x > 0.f ? 1.f : 0.f; s.y = v.y > 0.f ? 1.f : 0.f; s.z = v.z > 0.f ? 1.f : 0.f; s.w = v.w > 0.f ? 1.f : 0.f;
  }
  return c.x * s.x * v.x + c.y * s.y * v.y + c.z * s.z * v.z + c.w * s.w * v.w;
}

// '+' / '*', mid = 256 * IT <= 1024: the grouped forward's register kernel with its operands -- x_conv weights and the
// question's q' row in registers, 4 positions per wave, the next question's row in flight.  grid (ceil(P/16), N), 256
// threads, 16 * mid floats of dynamic LDS.  Every asked (b, p) is written exactly once.
template <int G, int IT, bool MUL, bool PAIRS, class VT = float>
__global__ __launch_bounds__(256) void att_attr_score_grouped_kernel(const float* r1, const float* dscore, const VT* vprime,
                                                                     const float* qp, const int* qrow, int M, const float* wx,
                                                                     int wx_ld, const int* order, const int* offsets, float* out,
                                                                     int B, int P) {
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
#pragma unroll
      for (int j = 0; j < PW; ++j) {
        if (pl + j < rows) {                              // wave-uniform
          const int64_t pos = p0 + pl + j;
          float ds[G];
#pragma unroll
          for (int g = 0; g < G; ++g) ds[g] = dscore[((int64_t)b * G + g) * P + pos];
          float acc = 0.f;
#pragma unroll
          for (int i = 0; i < IT; ++i)
            acc += att_attr_quad<G, MUL ? 1 : 0>(ds, w[i], reinterpret_cast<const float4*>(tile + (pl + j) * mid)[lane + 64 * i],
                                                 q[i]);
          acc = wave_sum(acc);
          if (lane == 0) out[(int64_t)b * P + pos] = r1[(int64_t)b * P + pos] + acc;
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
// `pw` positions per wave (the tile is 4 * pw rows).  '|' reads the first mid columns of wx and no q'.
template <int G, int MODE, bool PAIRS, class VT = float>
__global__ __launch_bounds__(256) void att_attr_score_grouped_general_kernel(const float* r1, const float* dscore,
                                                                             const VT* vprime, const float* qp, const int* qrow,
                                                                             int M, const float* wx, int wx_ld, const int* order,
                                                                             const int* offsets, float* out, int B, int P,
                                                                             int mid, int pw) {
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
    const int64_t pos = p0 + pl;
    const float4* vrow = reinterpret_cast<const float4*>(tile + pl * mid);
    for (int k = k0; k < k1; ++k) {
      const int b = order[k];
      const int r = att_q_row<PAIRS>(qrow, b, B, M);
      if (r < 0) continue;
      const float4* qv = MODE == 2 ? nullptr : reinterpret_cast<const float4*>(qp + (int64_t)r * mid);     // '|' reads no q'
      float ds[G];
#pragma unroll
      for (int g = 0; g < G; ++g) ds[g] = dscore[((int64_t)b * G + g) * P + pos];
      float acc = 0.f;
      for (int c = lane; c < nq; c += 64) {
        float4 w[G];
#pragma unroll
        for (int g = 0; g < G; ++g) w[g] = reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld)[c];
        const float4 q = MODE == 2 ? make_float4(0.f, 0.f, 0.f, 0.f) : qv[c];
        acc += att_attr_quad<G, MODE>(ds, w, vrow[c], q);
      }
      acc = wave_sum(acc);
      if (lane == 0) out[(int64_t)b * P + pos] = r1[(int64_t)b * P + pos] + acc;
    }
  }
}

// ------------------------------------------------------------------ integrated gradients: the path alpha * v' (inference)
// VqaNet.explain_integrated (include/vqa_hip.h): the grouped forward and the grouped attribution evaluated at
// S points x = alpha_s * v' of the straight path from the zero cache to the real one.  v_conv has no bias, so scaling vn by
// alpha scales v' by alpha: the path costs a multiply on the staged quad, and ONE staged tile serves every question of the
// image and every step of every question -- v' leaves HBM once per walk, as in the kernels above, whatever S is.
//   path scores   score[b][s][g][p] = bx[g] + sum_m wx[g][m] * relu((alpha_s v'[n*P+p][m]) (+|*) q'[b][m])   ('|': as the forward)
//   path attr     out[b][p] = scale * sum_s (r1[b][s][p] + sum_m c_s[m] * s_s[m] * (alpha_s v'[n*P+p][m]))
// with c_s = sum_g dscore[b][s][g][p] * wx[g][m] and s_s the indicator of att_attr_quad AT alpha_s v'.  The step-rows (b, s)
// are laid out as a batch of B*S questions, [B][S][G][P] and [B][S][P], so the apply-gather kernels between the two walks take
// them as they are.  Evaluation order: x = alpha_s * v' is rounded FIRST (att_path_quad: never contracted into the add that
// follows), then the element math of the kernels above runs on x -- both walks see the same pre-activation bits, and with
// dyadic inputs the fp32 indicator is the exact one.  Per (b, s, p) the summation order is the forward's / the attribution's;
// the path sum runs over s ascending, each step's r1 + r2 formed first, then scale: one order for every (b, p), no atomics,
// every asked (b, p) written exactly once.  The s loop sits inside the question walk: a register loop, nothing per step is
// kept but alpha_s.
__device__ __forceinline__ float4 att_path_quad(const float4 v, const float a) {
#pragma clang fp contract(off)
  return make_float4(a * v.x, a * v.y, a * v.z, a * v.w);
}

// Between the two walks the classifier sees the image half of its input at the step's path position: x[r][c] *= alphas[r % S]
// for the step-row r = b*S + s, over the first `cols` columns of a [rows][ld] buffer (the weighted sum of vn is linear in vn).
__global__ void att_path_scale_rows_kernel(float* x, int64_t ld, const float* alphas, int S, int64_t rows, int cols) {
  const int64_t n = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols;
    x[r * ld + (i - r * cols)] *= alphas[r % S];
  }
}

// '+' / '*', mid = 256 * IT <= 1024: att_score_grouped_kernel (DROP = false) with the step loop around its reduction.
// grid (ceil(P/16), N), 256 threads, 16 * mid floats of dynamic LDS.
template <int G, int IT, bool MUL, bool PAIRS, class VT = float>
__global__ __launch_bounds__(256) void att_path_score_grouped_kernel(const VT* vprime, const float* qp, const int* qrow, int M,
                                                                     const float* wx, int wx_ld, const float* bx,
                                                                     const float* alphas, const int* order, const int* offsets,
                                                                     float* score, int B, int S, int P) {
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
  float bias[G];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int g = 0; g < G; ++g) w[i][g] = reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld)[lane + 64 * i];
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
    // the next question's q' row is in flight while this one's steps are reduced
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
      for (int s = 0; s < S; ++s) {
        const float a = alphas[s];
        float acc[PW][G];
#pragma unroll
        for (int j = 0; j < PW; ++j)
#pragma unroll
          for (int g = 0; g < G; ++g) acc[j][g] = 0.f;
#pragma unroll
        for (int i = 0; i < IT; ++i) {
#pragma unroll
          for (int j = 0; j < PW; ++j) {
            if (pl + j < rows) {                          // wave-uniform
              const float4 v = reinterpret_cast<const float4*>(tile + (pl + j) * mid)[lane + 64 * i];
              const float4 x = att_combine<MUL>(att_path_quad(v, a), q[i]);
#pragma unroll
              for (int g = 0; g < G; ++g) acc[j][g] += dot4(x, w[i][g]);
            }
          }
        }
        const int64_t row = ((int64_t)b * S + s) * G;
#pragma unroll
        for (int j = 0; j < PW; ++j) {
          if (pl + j < rows) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
              const float t = wave_sum(acc[j][g]);
              if (lane == 0) score[(row + g) * P + p0 + pl + j] = t + bias[g];
            }
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

// Any mid % 4 == 0 and every mode: att_score_grouped_general_kernel (DROP = false) with the step loop inside the question
// walk.  '|': the q' half does not depend on the step and is reduced once per (position, question); the v' half, relu(alpha_s
// v'), is the step's own.
template <int G, bool PAIRS, class VT = float>
__global__ __launch_bounds__(256) void att_path_score_grouped_general_kernel(const VT* vprime, const float* qp, const int* qrow,
                                                                             int M, const float* wx, int wx_ld, const float* bx,
                                                                             const float* alphas, const int* order,
                                                                             const int* offsets, float* score, int B, int S, int P,
                                                                             int mid, int pw, int mode) {
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
    for (int k = k0; k < k1; ++k) {
      const int b = order[k];
      const int r = att_q_row<PAIRS>(qrow, b, B, M);
      if (r < 0) continue;
      const float4* qv = reinterpret_cast<const float4*>(qp + (int64_t)r * mid);
      float qpart[G];
#pragma unroll
      for (int g = 0; g < G; ++g) qpart[g] = 0.f;
      if (mode == 2) {
        float acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = 0.f;
        for (int c = lane; c < nq; c += 64) {
          const float4 x = relu4(qv[c]);
#pragma unroll
          for (int g = 0; g < G; ++g) acc[g] += dot4(x, reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld + mid)[c]);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) qpart[g] = wave_sum(acc[g]);
      }
      for (int s = 0; s < S; ++s) {
        const float a = alphas[s];
        float acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = 0.f;
        for (int c = lane; c < nq; c += 64) {
          const float4 xv = att_path_quad(vrow[c], a);
          const float4 x = mode == 2 ? relu4(xv) : (mode == 1 ? att_combine<true>(xv, qv[c]) : att_combine<false>(xv, qv[c]));
#pragma unroll
          for (int g = 0; g < G; ++g) acc[g] += dot4(x, reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld)[c]);
        }
        const int64_t row = ((int64_t)b * S + s) * G;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float t = wave_sum(acc[g]) + bx[g];       // '|': the bias goes with the v' half, as in the forward
          if (lane == 0) score[(row + g) * P + p0 + pl] = mode == 2 ? t + qpart[g] : t;
        }
      }
    }
  }
}

// '+' / '*', mid = 256 * IT <= 1024: att_attr_score_grouped_kernel with the step loop around its reduction and the path sum
// in a register per position.  The four positions of a wave advance through a step together, so that the step's dscore and
// r1 values (4 * (G + 1) broadcast loads) are in flight at once.
template <int G, int IT, bool MUL, bool PAIRS, class VT = float>
__global__ __launch_bounds__(256) void att_path_attr_grouped_kernel(const float* r1, const float* dscore, const VT* vprime,
                                                                    const float* qp, const int* qrow, int M, const float* wx,
                                                                    int wx_ld, const float* alphas, float scale, const int* order,
                                                                    const int* offsets, float* out, int B, int S, int P) {
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
      float total[PW];
#pragma unroll
      for (int j = 0; j < PW; ++j) total[j] = 0.f;
      for (int s = 0; s < S; ++s) {
        const float a = alphas[s];
        const int64_t row = (int64_t)b * S + s;
        float ds[PW][G], r[PW];
#pragma unroll
        for (int j = 0; j < PW; ++j) {
          const bool in = pl + j < rows;                  // wave-uniform
          const int64_t pos = p0 + pl + j;
          r[j] = in ? r1[row * P + pos] : 0.f;
#pragma unroll
          for (int g = 0; g < G; ++g) ds[j][g] = in ? dscore[(row * G + g) * P + pos] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < PW; ++j) {
          if (pl + j < rows) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < IT; ++i)
              acc += att_attr_quad<G, MUL ? 1 : 0>(
                  ds[j], w[i], att_path_quad(reinterpret_cast<const float4*>(tile + (pl + j) * mid)[lane + 64 * i], a), q[i]);
            total[j] += r[j] + wave_sum(acc);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < PW; ++j)
        if (pl + j < rows && lane == 0) out[(int64_t)b * P + p0 + pl + j] = scale * total[j];
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) q[i] = qn[i];
    b = bn;
    ok = okn;
  }
}

// Any mid % 4 == 0 and every mode: att_attr_score_grouped_general_kernel with the step loop inside the question walk.
template <int G, int MODE, bool PAIRS, class VT = float>
__global__ __launch_bounds__(256) void att_path_attr_grouped_general_kernel(const float* r1, const float* dscore, const VT* vprime,
                                                                            const float* qp, const int* qrow, int M,
                                                                            const float* wx, int wx_ld, const float* alphas,
                                                                            float scale, const int* order, const int* offsets,
                                                                            float* out, int B, int S, int P, int mid, int pw) {
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
    const int64_t pos = p0 + pl;
    const float4* vrow = reinterpret_cast<const float4*>(tile + pl * mid);
    for (int k = k0; k < k1; ++k) {
      const int b = order[k];
      const int r = att_q_row<PAIRS>(qrow, b, B, M);
      if (r < 0) continue;
      const float4* qv = MODE == 2 ? nullptr : reinterpret_cast<const float4*>(qp + (int64_t)r * mid);     // '|' reads no q'
      float total = 0.f;
      for (int s = 0; s < S; ++s) {
        const float a = alphas[s];
        const int64_t row = (int64_t)b * S + s;
        float ds[G];
#pragma unroll
        for (int g = 0; g < G; ++g) ds[g] = dscore[(row * G + g) * P + pos];
        float acc = 0.f;
        for (int c = lane; c < nq; c += 64) {
          float4 w[G];
#pragma unroll
          for (int g = 0; g < G; ++g) w[g] = reinterpret_cast<const float4*>(wx + (int64_t)g * wx_ld)[c];
          const float4 q = MODE == 2 ? make_float4(0.f, 0.f, 0.f, 0.f) : qv[c];
          acc += att_attr_quad<G, MODE>(ds, w, att_path_quad(vrow[c], a), q);
        }
        total += r1[row * P + pos] + wave_sum(acc);
      }
      if (lane == 0) out[(int64_t)b * P + pos] = scale * total;
    }
  }
}

// ------------------------------------------------------------------ grouped backward (training through shared image features)
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

//
// DQ_ONLY (vqa_att_attr_dq_grouped / _f16, inference: the gradient of ONE logit at q' through the scores, for the per-token
// map of VqaNet.explain_words): the same body with the dv' tile, the dw accumulators and their stores compiled out -- the
// thread keeps its 16 float4 of v' and nothing else across the question walk, dvprime and dwx_part are never touched (NULL).
// dq is the same sequence of operations on the same values, so dq_part equals the training form's at p = 0 bit for bit.
// '+' / '*' only: for '|' the q' half adds the same constant to every position's score and softmax is shift-invariant, so
// the gradient at q' of anything behind the softmax is identically zero -- there is no DQ_ONLY instantiation of MODE 2.
// VT: v' is fp32, or fp16 for a float16 image-feature cache (cache_load.hpp; DQ_ONLY only): widened on load, same bits.
template <int G, int MODE, bool DROP, bool DQ_ONLY = false, class VT = float>
__device__ __forceinline__ void att_score_bwd_quad(const float* __restrict__ dscore, const VT* __restrict__ vprime,
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
  static_assert(!DQ_ONLY || (MODE != 2 && !DROP), "DQ_ONLY: '+' / '*', no dropout");
  float4 v[BTP], dv[DQ_ONLY ? 1 : BTP];
#pragma unroll
  for (int j = 0; j < BTP; ++j) {
    v[j] = zero;
    if constexpr (!DQ_ONLY) dv[j] = zero;
    if (j < rows && k0 < k1) v[j] = load_quad(vprime + ((int64_t)n * P + p0 + j) * mid, c);
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
        const float4 d = att_score_bwd_dx<G, !DQ_ONLY>(ds, w, x, sc, dw);
        if constexpr (DQ_ONLY) {
          if (MODE == 0) { dq.x += d.x; dq.y += d.y; dq.z += d.z; dq.w += d.w; }
          else {                                          // as the training form's `dq += d * v` compiles: fused
            dq.x = fmaf(d.x, v[j].x, dq.x); dq.y = fmaf(d.y, v[j].y, dq.y); dq.z = fmaf(d.z, v[j].z, dq.z); dq.w = fmaf(d.w, v[j].w, dq.w);
          }
        } else if (MODE == 0) {
          dq.x += d.x; dq.y += d.y; dq.z += d.z; dq.w += d.w;
          dv[j].x += d.x; dv[j].y += d.y; dv[j].z += d.z; dv[j].w += d.w;
        } else if (MODE == 1) {
          dq.x += d.x * v[j].x; dq.y += d.y * v[j].y; dq.z += d.z * v[j].z; dq.w += d.w * v[j].w;
          dv[j].x += d.x * q.x; dv[j].y += d.y * q.y; dv[j].z += d.z * q.z; dv[j].w += d.w * q.w;
        } else {
          dv[j].x += d.x; dv[j].y += d.y; dv[j].z += d.z; dv[j].w += d.w;
          float4 s2 = make_float4(1.f, 1.f, 1.f, 1.f);
          if (DROP) s2 = drop_scale4(seed, (uint64_t)m * xld + mid + 4 * c, p, inv_keep);
          att_score_bwd_qhalf<G>(ds, w2, q, rq, s2, dw2, dq);
        }
      }
    }
    reinterpret_cast<float4*>(dq_part + ((int64_t)b * NT + tile) * mid)[c] = dq;
  }
  if constexpr (!DQ_ONLY) {
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

// vqa_att_attr_dq_grouped / _f16: the two kernels above under DQ_ONLY -- same grid, same block, same ownership (16 positions
// of one image per workgroup, one channel quad per thread), same dispatch (att_score_grouped_pw).  No LDS, no atomics.
template <int G, int IT, bool MUL, class VT>
__global__ __launch_bounds__(64 * IT) void att_attr_dq_grouped_kernel(const float* dscore, const VT* vprime, const float* qp,
                                                                       const float* wx, int wx_ld, const int* order,
                                                                       const int* offsets, float* dq_part, int B, int P) {
  constexpr int mid = 256 * IT;
  const int n = blockIdx.y, tile = blockIdx.x;
  int k0, k1;
  att_group_range(offsets, n, B, k0, k1);
  att_score_bwd_quad<G, MUL ? 1 : 0, false, true, VT>(dscore, vprime, qp, wx, wx_ld, order, nullptr, dq_part, nullptr, n, tile,
                                                      gridDim.x, min(BTP, P - tile * BTP), k0, k1, B, P, mid, threadIdx.x, 0.f,
                                                      1.f, 0);
}

template <int G, int MODE, class VT>
__global__ __launch_bounds__(256) void att_attr_dq_grouped_general_kernel(const float* dscore, const VT* vprime, const float* qp,
                                                                          const float* wx, int wx_ld, const int* order,
                                                                          const int* offsets, float* dq_part, int B, int P,
                                                                          int mid) {
  const int n = blockIdx.y, tile = blockIdx.x;
  int k0, k1;
  att_group_range(offsets, n, B, k0, k1);
  const int rows = min(BTP, P - tile * BTP);
  for (int c = threadIdx.x; c < (mid >> 2); c += 256)
    att_score_bwd_quad<G, MODE, false, true, VT>(dscore, vprime, qp, wx, wx_ld, order, nullptr, dq_part, nullptr, n, tile,
                                                 gridDim.x, rows, k0, k1, B, P, mid, c, 0.f, 1.f, 0);
}

}  // namespace vqa

using namespace vqa;

// ---------------------------------------------------------------- host side
// What the six score entry points check, before any HIP call (`who` names the caller in the messages).
// grouped: the form has an LDS tile of v' that bounds mid.  pointers: the form's data pointers are all there, those its mode
// needs included.  indices: its order / offsets (true for a plain form).  N: 1 for a form without an image count.
// mode: 0 '+', 1 '*', 2 '|' -- x has 2 * mid channels for '|' (the plain forward passes 2 where it has a qcat, else 0).
// p: the x_conv dropout (0 for a form without).  quads: ptr_bits() of what the kernels read or write as float4 whatever the
// path -- wx, the q' / v' operands, the backward's outputs; a null pointer counts as aligned.  The plain forms' xs is not
// among them: its alignment selects the forward's register kernels and is no error.
static int att_score_check(const char* who, bool grouped, bool pointers, bool indices, int N, int B, int P, int mid, int wx_ld,
                           int G, int mode, float p, uintptr_t quads) {
  VQA_REQUIRE(G >= 1 && G <= 4, "%s: glimpses=%d unsupported (1..4)", who, G);
  VQA_REQUIRE(mode >= 0 && mode <= 2, "%s: mode %d (0 '+', 1 '*', 2 '|')", who, mode);
  VQA_REQUIRE(pointers, "%s: null pointer", who);
  VQA_REQUIRE(indices, "%s: null order / offsets", who);
  VQA_REQUIRE(N >= 1 && N <= 65535 && B >= 0 && P >= 1, "%s: N=%d (1..65535), B=%d, P=%d out of range", who, N, B, P);
  VQA_REQUIRE(mid >= 4 && mid % 4 == 0 && wx_ld % 4 == 0 && wx_ld >= (mode == 2 ? 2 * mid : mid),
              "%s: bad args (mid=%d and wx_ld=%d must be multiples of 4, wx_ld >= channels of x)", who, mid, wx_ld);
  VQA_REQUIRE(!grouped || mid <= 4096, "%s: mid=%d too large (the forward's LDS tile: 4 rows x mid fp32 <= 64 KiB)", who, mid);
  VQA_REQUIRE((quads & 15) == 0, "%s: wx, the q' / v' operands and the outputs read as quads must be 16-byte aligned", who);
  VQA_REQUIRE(p >= 0.f && p < 1.f, "%s: dropout p=%g outside [0, 1)", who, (double)p);
  return VQA_OK;
}

// the kernel of vqa_att_score_fwd: the register kernels need an xs they can read 16 bytes at a time and no concatenated half
enum ScoreFwdPath { SCORE_FWD_BF16_ROWS, SCORE_FWD_ROWS, SCORE_FWD_GENERAL };
static ScoreFwdPath att_score_fwd_path(const void* xs, bool bf16, bool qcat, int mid, int G) {
  if (qcat || mid > 1024 || (ptr_bits(xs) & 15) != 0) return SCORE_FWD_GENERAL;
  if (bf16) return mid % 8 == 0 ? SCORE_FWD_BF16_ROWS : SCORE_FWD_GENERAL;
  return G <= 2 && mid % 256 == 0 ? SCORE_FWD_ROWS : SCORE_FWD_GENERAL;      // the rows kernel exists for one and two glimpses only
}

// the kernels of the grouped forms: 0 = the register kernels ('+' / '*', mid = 256 * IT <= 1024), else the general kernels
// with that many positions per wave in the forward (4 * pw rows of mid floats <= 64 KiB)
static int att_score_grouped_pw(int mode, int mid) {
  if (mode != 2 && mid % 256 == 0 && mid <= 1024) return 0;
  return mid <= 1024 ? 4 : (mid <= 2048 ? 2 : 1);
}

// DROP x PAIRS is never instantiated: the pairs entry point (inference) has no dropout
template <class F>
static int with_drop_or_pairs(bool drop, bool pairs, F&& f) {
  return pairs ? f(Flag<false>{}, Flag<true>{}) : with_flag(drop, [&](auto d) { return f(d, Flag<false>{}); });
}

// the grouped forward entry points: p == 0 runs the DROP = false kernels, the inference entry point's code; qrow != NULL
// (inference only, p == 0, seed == 0) runs their PAIRS instantiations over the q' table qp [M][mid].  VT = __half: the two
// inference entry points on a float16 v' (a float16 image-feature cache, p == 0): no DROP kernel is instantiated for it, and
// the tile loader reads a quad of halves as 8 bytes, so v' is 8-byte aligned where the fp32 form asks for 16
template <class VT>
static int grouped_fwd(const char* who, const VT* vprime, const float* qp, const int32_t* qrow, int M, const float* wx,
                       int wx_ld, const float* bx, const int32_t* order, const int32_t* offsets, float* score, int N, int B, int P,
                       int mid, int G, int mode, float p, uint64_t seed, hipStream_t s) {
  constexpr bool f32 = std::is_same<VT, float>::value;
  const int rc = att_score_check(who, true, vprime && qp && wx && bx && score, order && offsets, N, B, P, mid, wx_ld, G, mode, p,
                                 f32 ? ptr_bits(vprime, qp, wx) : ptr_bits(qp, wx));
  if (rc) return rc;
  VQA_REQUIRE((ptr_bits(vprime) & (kQuadAlign<VT> - 1)) == 0, "%s: vprime must be %d-byte aligned", who, (int)kQuadAlign<VT>);
  if (B == 0) return VQA_OK;
  const float ik = keep_scale(p);
  const int pw = att_score_grouped_pw(mode, mid), TP = pw ? 4 * pw : 16;
  const dim3 grid((P + TP - 1) / TP, N);
  const size_t lds = (size_t)TP * mid * 4;
  with_int14(G, [&](auto g) {
    auto launch = [&](auto drop, auto pairs) {
      constexpr int kG = decltype(g)::value;
      constexpr bool kDrop = decltype(drop)::value, kPairs = decltype(pairs)::value;
      if (pw)
        hipLaunchKernelGGL((att_score_grouped_general_kernel<kG, kDrop, kPairs, VT>), grid, dim3(256), lds, s, vprime, qp, qrow, M,
                           wx, wx_ld, bx, order, offsets, score, B, P, mid, pw, mode, p, ik, seed);
      else
        with_int14(mid / 256, [&](auto it) {
          return with_flag(mode == 1, [&](auto mul) {
            hipLaunchKernelGGL((att_score_grouped_kernel<kG, decltype(it)::value, decltype(mul)::value, kDrop, kPairs, VT>), grid,
                               dim3(256), lds, s, vprime, qp, qrow, M, wx, wx_ld, bx, order, offsets, score, B, P, p, ik, seed);
            return 0;
          });
        });
      return 0;
    };
    if constexpr (f32) return with_drop_or_pairs(p > 0.f, qrow != nullptr, launch);
    else return with_flag(qrow != nullptr, [&](auto pairs) { return launch(Flag<false>{}, pairs); });
  });
  return check_hip(hipGetLastError(), "att_score_grouped_fwd launch");
}

// the four attribution entry points: the grouped forward's checks, grid, LDS size and path choice (att_score_grouped_pw);
// qrow != NULL runs the PAIRS instantiations over the q' table qp [M][mid]; '|' reads no q' (qp may be NULL there)
template <class VT>
static int grouped_attr(const char* who, const float* r1, const float* dscore, const VT* vprime, const float* qp,
                        const int32_t* qrow, int M, const float* wx, int wx_ld, const int32_t* order, const int32_t* offsets,
                        float* out, int N, int B, int P, int mid, int G, int mode, hipStream_t s) {
  constexpr bool f32 = std::is_same<VT, float>::value;
  const int rc = att_score_check(who, true, r1 && dscore && vprime && wx && out && (mode == 2 || qp), order && offsets, N, B, P,
                                 mid, wx_ld, G, mode, 0.f, f32 ? ptr_bits(vprime, qp, wx) : ptr_bits(qp, wx));
  if (rc) return rc;
  VQA_REQUIRE((ptr_bits(vprime) & (kQuadAlign<VT> - 1)) == 0, "%s: vprime must be %d-byte aligned", who, (int)kQuadAlign<VT>);
  if (B == 0) return VQA_OK;
  const int pw = att_score_grouped_pw(mode, mid), TP = pw ? 4 * pw : 16;
  const dim3 grid((P + TP - 1) / TP, N);
  const size_t lds = (size_t)TP * mid * 4;
  // MODE is a template argument of the general kernel: a macro passes the constant
#define GROUPED_ATTR_GENERAL(kMODE)                                                                                              \
  hipLaunchKernelGGL((att_attr_score_grouped_general_kernel<kG, kMODE, kPairs, VT>), grid, dim3(256), lds, s, r1, dscore, vprime, \
                     qp, qrow, M, wx, wx_ld, order, offsets, out, B, P, mid, pw)
  with_int14(G, [&](auto g) {
    return with_flag(qrow != nullptr, [&](auto pairs) {
      constexpr int kG = decltype(g)::value;
      constexpr bool kPairs = decltype(pairs)::value;
      if (pw == 0)
        with_int14(mid / 256, [&](auto it) {
          return with_flag(mode == 1, [&](auto mul) {
            hipLaunchKernelGGL((att_attr_score_grouped_kernel<kG, decltype(it)::value, decltype(mul)::value, kPairs, VT>), grid,
                               dim3(256), lds, s, r1, dscore, vprime, qp, qrow, M, wx, wx_ld, order, offsets, out, B, P);
            return 0;
          });
        });
      else if (mode == 0) GROUPED_ATTR_GENERAL(0);
      else if (mode == 1) GROUPED_ATTR_GENERAL(1);
      else GROUPED_ATTR_GENERAL(2);
      return 0;
    });
  });
#undef GROUPED_ATTR_GENERAL
  return check_hip(hipGetLastError(), "att_attr_score_grouped launch");
}

// what the eight path entry points add to the grouped checks: the step positions
static int att_path_check(const char* who, const float* alphas, int S) {
  VQA_REQUIRE(alphas, "%s: null alphas", who);
  VQA_REQUIRE(S >= 1 && S <= VQA_ATT_PATH_MAX_STEPS, "%s: S=%d steps out of range (1..%d)", who, S, VQA_ATT_PATH_MAX_STEPS);
  return VQA_OK;
}

// the four path-score entry points: grouped_fwd's checks, grid, LDS size and path choice at p = 0, over S step positions
template <class VT>
static int grouped_path_fwd(const char* who, const VT* vprime, const float* qp, const int32_t* qrow, int M, const float* wx,
                            int wx_ld, const float* bx, const float* alphas, const int32_t* order, const int32_t* offsets,
                            float* score, int N, int B, int S, int P, int mid, int G, int mode, hipStream_t s) {
  constexpr bool f32 = std::is_same<VT, float>::value;
  int rc = att_score_check(who, true, vprime && qp && wx && bx && score, order && offsets, N, B, P, mid, wx_ld, G, mode, 0.f,
                           f32 ? ptr_bits(vprime, qp, wx) : ptr_bits(qp, wx));
  if (rc) return rc;
  if ((rc = att_path_check(who, alphas, S))) return rc;
  VQA_REQUIRE((ptr_bits(vprime) & (kQuadAlign<VT> - 1)) == 0, "%s: vprime must be %d-byte aligned", who, (int)kQuadAlign<VT>);
  if (B == 0) return VQA_OK;
  const int pw = att_score_grouped_pw(mode, mid), TP = pw ? 4 * pw : 16;
  const dim3 grid((P + TP - 1) / TP, N);
  const size_t lds = (size_t)TP * mid * 4;
  with_int14(G, [&](auto g) {
    return with_flag(qrow != nullptr, [&](auto pairs) {
      constexpr int kG = decltype(g)::value;
      constexpr bool kPairs = decltype(pairs)::value;
      if (pw)
        hipLaunchKernelGGL((att_path_score_grouped_general_kernel<kG, kPairs, VT>), grid, dim3(256), lds, s, vprime, qp, qrow, M, wx,
                           wx_ld, bx, alphas, order, offsets, score, B, S, P, mid, pw, mode);
      else
        with_int14(mid / 256, [&](auto it) {
          return with_flag(mode == 1, [&](auto mul) {
            hipLaunchKernelGGL((att_path_score_grouped_kernel<kG, decltype(it)::value, decltype(mul)::value, kPairs, VT>), grid,
                               dim3(256), lds, s, vprime, qp, qrow, M, wx, wx_ld, bx, alphas, order, offsets, score, B, S, P);
            return 0;
          });
        });
      return 0;
    });
  });
  return check_hip(hipGetLastError(), "att_path_score_grouped launch");
}

// the four path-attribution entry points: grouped_attr's checks, grid, LDS size and path choice, over S step positions
template <class VT>
static int grouped_path_attr(const char* who, const float* r1, const float* dscore, const VT* vprime, const float* qp,
                             const int32_t* qrow, int M, const float* wx, int wx_ld, const float* alphas, float scale,
                             const int32_t* order, const int32_t* offsets, float* out, int N, int B, int S, int P, int mid, int G,
                             int mode, hipStream_t s) {
  constexpr bool f32 = std::is_same<VT, float>::value;
  int rc = att_score_check(who, true, r1 && dscore && vprime && wx && out && (mode == 2 || qp), order && offsets, N, B, P, mid,
                           wx_ld, G, mode, 0.f, f32 ? ptr_bits(vprime, qp, wx) : ptr_bits(qp, wx));
  if (rc) return rc;
  if ((rc = att_path_check(who, alphas, S))) return rc;
  VQA_REQUIRE((ptr_bits(vprime) & (kQuadAlign<VT> - 1)) == 0, "%s: vprime must be %d-byte aligned", who, (int)kQuadAlign<VT>);
  if (B == 0) return VQA_OK;
  const int pw = att_score_grouped_pw(mode, mid), TP = pw ? 4 * pw : 16;
  const dim3 grid((P + TP - 1) / TP, N);
  const size_t lds = (size_t)TP * mid * 4;
  // MODE is a template argument of the general kernel: a macro passes the constant
#define GROUPED_PATH_ATTR_GENERAL(kMODE)                                                                                          \
  hipLaunchKernelGGL((att_path_attr_grouped_general_kernel<kG, kMODE, kPairs, VT>), grid, dim3(256), lds, s, r1, dscore, vprime,  \
                     qp, qrow, M, wx, wx_ld, alphas, scale, order, offsets, out, B, S, P, mid, pw)
  with_int14(G, [&](auto g) {
    return with_flag(qrow != nullptr, [&](auto pairs) {
      constexpr int kG = decltype(g)::value;
      constexpr bool kPairs = decltype(pairs)::value;
      if (pw == 0)
        with_int14(mid / 256, [&](auto it) {
          return with_flag(mode == 1, [&](auto mul) {
            hipLaunchKernelGGL((att_path_attr_grouped_kernel<kG, decltype(it)::value, decltype(mul)::value, kPairs, VT>), grid,
                               dim3(256), lds, s, r1, dscore, vprime, qp, qrow, M, wx, wx_ld, alphas, scale, order, offsets, out, B,
                               S, P);
            return 0;
          });
        });
      else if (mode == 0) GROUPED_PATH_ATTR_GENERAL(0);
      else if (mode == 1) GROUPED_PATH_ATTR_GENERAL(1);
      else GROUPED_PATH_ATTR_GENERAL(2);
      return 0;
    });
  });
#undef GROUPED_PATH_ATTR_GENERAL
  return check_hip(hipGetLastError(), "att_path_attr_grouped launch");
}

// the two entry points of d logit / d q' through the scores: the checks and limits of att_score_check, the grid and the
// path choice of vqa_att_score_grouped_bwd.  '|' is refused: that gradient is identically zero (see att_score_bwd_quad)
template <class VT>
static int grouped_attr_dq(const char* who, const float* dscore, const VT* vprime, const float* qp, const float* wx, int wx_ld,
                           const int32_t* order, const int32_t* offsets, float* dq_part, int N, int B, int P, int mid, int G,
                           int mode, hipStream_t s) {
  constexpr bool f32 = std::is_same<VT, float>::value;
  VQA_REQUIRE(mode != 2,
              "%s: mode 2 ('|') has no gradient to compute: the q' half adds the same constant to every position's score and "
              "softmax is shift-invariant, so d logit / d q' through the scores is identically zero (modes 0 '+' and 1 '*' only)",
              who);
  const int rc = att_score_check(who, true, dscore && vprime && qp && wx && dq_part, order && offsets, N, B, P, mid, wx_ld, G,
                                 mode, 0.f, (f32 ? ptr_bits(vprime, qp, wx) : ptr_bits(qp, wx)) | ptr_bits(dq_part));
  if (rc) return rc;
  VQA_REQUIRE((ptr_bits(vprime) & (kQuadAlign<VT> - 1)) == 0, "%s: vprime must be %d-byte aligned", who, (int)kQuadAlign<VT>);
  if (B == 0) return VQA_OK;
  const dim3 grid((P + BTP - 1) / BTP, N);                 // vqa_att_score_grouped_tiles(P)
  with_int14(G, [&](auto g) {
    constexpr int kG = decltype(g)::value;
    if (att_score_grouped_pw(mode, mid) == 0)
      with_int14(mid / 256, [&](auto it) {
        return with_flag(mode == 1, [&](auto mul) {
          hipLaunchKernelGGL((att_attr_dq_grouped_kernel<kG, decltype(it)::value, decltype(mul)::value, VT>), grid,
                             dim3(64 * decltype(it)::value), 0, s, dscore, vprime, qp, wx, wx_ld, order, offsets, dq_part, B, P);
          return 0;
        });
      });
    else if (mode == 0)
      hipLaunchKernelGGL((att_attr_dq_grouped_general_kernel<kG, 0, VT>), grid, dim3(256), 0, s, dscore, vprime, qp, wx, wx_ld,
                         order, offsets, dq_part, B, P, mid);
    else
      hipLaunchKernelGGL((att_attr_dq_grouped_general_kernel<kG, 1, VT>), grid, dim3(256), 0, s, dscore, vprime, qp, wx, wx_ld,
                         order, offsets, dq_part, B, P, mid);
    return 0;
  });
  return check_hip(hipGetLastError(), "att_attr_dq_grouped launch");
}

extern "C" {

// The plain forms take the checks of their grouped forms (att_score_check): what used to reach a launch with undefined
// results -- B < 0 or P < 1, a mid below 4, a p outside [0, 1), a wx / qcat / qp / vprime / dwx_part / dq_part that cannot
// be read or written as float4 -- is VQA_ERR_INVALID, and B == 0 is VQA_OK without a launch (the backward's grid (B, RS)
// was an invalid configuration there).  Every argument set that was valid runs the kernel it ran, on the same grid and block.
int vqa_att_score_fwd(const void* xs, int xs_is_bf16, const float* wx, int wx_ld, const float* bx, float* score, int B,
                      int P, int mid, int G, float p, uint64_t seed, const float* qcat, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_FWD, (hipStream_t)stream);
  const int rc = att_score_check("vqa_att_score_fwd", false, xs && wx && bx && score, true, 1, B, P, mid, wx_ld, G, qcat ? 2 : 0, p,
                                 ptr_bits(wx, qcat));
  if (rc) return rc;
  if (B == 0) return VQA_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t M = (int64_t)B * P;
  const float ik = keep_scale(p);
  const ScoreFwdPath path = att_score_fwd_path(xs, xs_is_bf16 != 0, qcat != nullptr, mid, G);
  const dim3 grid(grid_for(M, path == SCORE_FWD_BF16_ROWS ? 8 : 4));
  with_int14(G, [&](auto g) {
    constexpr int kG = decltype(g)::value;
    if (path == SCORE_FWD_BF16_ROWS)
      hipLaunchKernelGGL((att_score_fwd_bf16_kernel<kG>), grid, dim3(256), 0, s, static_cast<const uint16_t*>(xs), wx, wx_ld, bx,
                         score, M, P, mid, p, ik, seed);
    else if (path == SCORE_FWD_ROWS)
      with_int14(mid / 256, [&](auto it) {
        hipLaunchKernelGGL((att_score_fwd_rows_kernel<(kG <= 2 ? kG : 2), decltype(it)::value>), grid, dim3(256), 0, s,
                           static_cast<const float*>(xs), wx, wx_ld, bx, score, M, P, p, ik, seed);
        return 0;
      });
    else
      with_flag(xs_is_bf16 != 0, [&](auto bf16) {
        hipLaunchKernelGGL((att_score_fwd_kernel<kG, decltype(bf16)::value>), grid, dim3(256), 0, s, xs, wx, wx_ld, bx, score, M,
                           P, mid, p, ik, seed, qcat);
        return 0;
      });
    return 0;
  });
  return check_hip(hipGetLastError(), "att_score_fwd launch");
}

int vqa_att_row_splits(int P) {
  int rs = (P + 127) / 128;
  return rs < 1 ? 1 : (rs > 8 ? 8 : rs);
}

int vqa_att_score_bwd(const float* dscore, const float* wx, int wx_ld, void* xs_inout, int xs_is_bf16, float* dwx_part,
                      float* dq_part, int B, int P, int mid, int G, float p, uint64_t seed, int mode,
                      const float* vprime, const float* qp, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_BWD, (hipStream_t)stream);
  const bool operands = (mode != 1 || (vprime && qp)) && (mode != 2 || qp);      // '+' reads neither
  const int rc = att_score_check("vqa_att_score_bwd", false, dscore && wx && xs_inout && dwx_part && dq_part && operands, true, 1,
                                 B, P, mid, wx_ld, G, mode, p, ptr_bits(wx, dwx_part, dq_part, mode ? qp : nullptr, mode == 1 ? vprime : nullptr));
  if (rc) return rc;
  if (B == 0) return VQA_OK;
  const int RS = vqa_att_row_splits(P);
  return with_int14(G, [&](auto g) {
    return with_flag(xs_is_bf16 != 0, [&](auto bf16) {
      hipLaunchKernelGGL((att_score_bwd_kernel<decltype(g)::value, decltype(bf16)::value>), dim3(B, RS), dim3(256), 0,
                         (hipStream_t)stream, dscore, wx, wx_ld, xs_inout, dwx_part, dq_part, P, mid, RS, p, keep_scale(p), seed,
                         mode, vprime, qp);
      return check_hip(hipGetLastError(), "att_score_bwd launch");
    });
  });
}

int vqa_att_score_grouped_fwd(const float* vprime, const float* qp, const float* wx, int wx_ld, const float* bx,
                              const int32_t* order, const int32_t* offsets, float* score, int N, int B, int P, int mid, int G,
                              int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_FWD, (hipStream_t)stream);
  return grouped_fwd("vqa_att_score_grouped_fwd", vprime, qp, nullptr, 0, wx, wx_ld, bx, order, offsets, score, N, B, P, mid, G,
                     mode, 0.f, 0, (hipStream_t)stream);
}

int vqa_att_score_grouped_pairs_fwd(const float* vprime, const float* qp, const int32_t* qrow, const float* wx, int wx_ld,
                                    const float* bx, const int32_t* order, const int32_t* offsets, float* score, int N, int B,
                                    int M, int P, int mid, int G, int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_FWD, (hipStream_t)stream);
  VQA_REQUIRE(qrow, "vqa_att_score_grouped_pairs_fwd: null qrow");
  VQA_REQUIRE(M >= 1, "vqa_att_score_grouped_pairs_fwd: M=%d question rows (>= 1)", M);
  return grouped_fwd("vqa_att_score_grouped_pairs_fwd", vprime, qp, qrow, M, wx, wx_ld, bx, order, offsets, score, N, B, P, mid, G,
                     mode, 0.f, 0, (hipStream_t)stream);
}

int vqa_att_score_grouped_drop_fwd(const float* vprime, const float* qp, const float* wx, int wx_ld, const float* bx,
                                   const int32_t* order, const int32_t* offsets, float* score, int N, int B, int P, int mid,
                                   int G, int mode, float p, uint64_t seed, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_FWD, (hipStream_t)stream);
  return grouped_fwd("vqa_att_score_grouped_drop_fwd", vprime, qp, nullptr, 0, wx, wx_ld, bx, order, offsets, score, N, B, P, mid, G,
                     mode, p, seed, (hipStream_t)stream);
}

int vqa_att_score_grouped_tiles(int P) { return P < 1 ? 1 : (P + BTP - 1) / BTP; }

int vqa_att_score_grouped_bwd(const float* dscore, const float* vprime, const float* qp, const float* wx, int wx_ld,
                              const int32_t* order, const int32_t* offsets, float* dvprime, float* dq_part, float* dwx_part,
                              int N, int B, int P, int mid, int G, int mode, float p, uint64_t seed, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_BWD, (hipStream_t)stream);
  const int rc = att_score_check("vqa_att_score_grouped_bwd", true, dscore && vprime && qp && wx && dvprime && dq_part && dwx_part,
                                 order && offsets, N, B, P, mid, wx_ld, G, mode, p,
                                 ptr_bits(vprime, qp, wx, dvprime, dq_part, dwx_part));
  if (rc) return rc;
  if (B == 0) return VQA_OK;
  hipStream_t s = (hipStream_t)stream;
  const float ik = keep_scale(p);
  const dim3 grid(vqa_att_score_grouped_tiles(P), N);
  // MODE is a template argument of the general kernel and `mul` one of the register kernel: a macro passes the constant
#define GROUPED_BWD_GENERAL(kMODE)                                                                                                \
  hipLaunchKernelGGL((att_score_grouped_bwd_general_kernel<kG, kMODE, kDrop>), grid, dim3(256), 0, s, dscore, vprime, qp, wx,    \
                     wx_ld, order, offsets, dvprime, dq_part, dwx_part, B, P, mid, p, ik, seed)
  with_int14(G, [&](auto g) {
    return with_flag(p > 0.f, [&](auto drop) {
      constexpr int kG = decltype(g)::value;
      constexpr bool kDrop = decltype(drop)::value;
      if (att_score_grouped_pw(mode, mid) == 0)
        with_int14(mid / 256, [&](auto it) {
          return with_flag(mode == 1, [&](auto mul) {
            hipLaunchKernelGGL((att_score_grouped_bwd_kernel<kG, decltype(it)::value, decltype(mul)::value, kDrop>), grid,
                               dim3(64 * decltype(it)::value), 0, s, dscore, vprime, qp, wx, wx_ld, order, offsets, dvprime,
                               dq_part, dwx_part, B, P, p, ik, seed);
            return 0;
          });
        });
      else if (mode == 0) GROUPED_BWD_GENERAL(0);
      else if (mode == 1) GROUPED_BWD_GENERAL(1);
      else GROUPED_BWD_GENERAL(2);
      return 0;
    });
  });
#undef GROUPED_BWD_GENERAL
  return check_hip(hipGetLastError(), "att_score_grouped_bwd launch");
}

int vqa_att_score_grouped_fwd_f16(const void* vprime_f16, const float* qp, const float* wx, int wx_ld, const float* bx,
                                  const int32_t* order, const int32_t* offsets, float* score, int N, int B, int P, int mid, int G,
                                  int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_FWD, (hipStream_t)stream);
  return grouped_fwd("vqa_att_score_grouped_fwd_f16", static_cast<const __half*>(vprime_f16), qp, nullptr, 0, wx, wx_ld, bx, order,
                     offsets, score, N, B, P, mid, G, mode, 0.f, 0, (hipStream_t)stream);
}

int vqa_att_score_grouped_pairs_fwd_f16(const void* vprime_f16, const float* qp, const int32_t* qrow, const float* wx, int wx_ld,
                                        const float* bx, const int32_t* order, const int32_t* offsets, float* score, int N, int B,
                                        int M, int P, int mid, int G, int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_FWD, (hipStream_t)stream);
  VQA_REQUIRE(qrow, "vqa_att_score_grouped_pairs_fwd_f16: null qrow");
  VQA_REQUIRE(M >= 1, "vqa_att_score_grouped_pairs_fwd_f16: M=%d question rows (>= 1)", M);
  return grouped_fwd("vqa_att_score_grouped_pairs_fwd_f16", static_cast<const __half*>(vprime_f16), qp, qrow, M, wx, wx_ld, bx,
                     order, offsets, score, N, B, P, mid, G, mode, 0.f, 0, (hipStream_t)stream);
}

// ---- gradient x input attribution
int vqa_att_attr_score_grouped_path(int mode, int mid) { return att_score_grouped_pw(mode, mid); }

int vqa_att_attr_score_grouped(const float* r1, const float* dscore, const float* vprime, const float* qp, const float* wx,
                               int wx_ld, const int32_t* order, const int32_t* offsets, float* out, int N, int B, int P, int mid,
                               int G, int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_BWD, (hipStream_t)stream);
  return grouped_attr("vqa_att_attr_score_grouped", r1, dscore, vprime, qp, nullptr, 0, wx, wx_ld, order, offsets, out, N, B, P,
                      mid, G, mode, (hipStream_t)stream);
}

int vqa_att_attr_score_grouped_pairs(const float* r1, const float* dscore, const float* vprime, const float* qp,
                                     const int32_t* qrow, const float* wx, int wx_ld, const int32_t* order, const int32_t* offsets,
                                     float* out, int N, int B, int M, int P, int mid, int G, int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_BWD, (hipStream_t)stream);
  VQA_REQUIRE(qrow, "vqa_att_attr_score_grouped_pairs: null qrow");
  VQA_REQUIRE(M >= 1, "vqa_att_attr_score_grouped_pairs: M=%d question rows (>= 1)", M);
  return grouped_attr("vqa_att_attr_score_grouped_pairs", r1, dscore, vprime, qp, qrow, M, wx, wx_ld, order, offsets, out, N, B, P,
                      mid, G, mode, (hipStream_t)stream);
}

int vqa_att_attr_score_grouped_f16(const float* r1, const float* dscore, const void* vprime_f16, const float* qp, const float* wx,
                                   int wx_ld, const int32_t* order, const int32_t* offsets, float* out, int N, int B, int P,
                                   int mid, int G, int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_BWD, (hipStream_t)stream);
  return grouped_attr("vqa_att_attr_score_grouped_f16", r1, dscore, static_cast<const __half*>(vprime_f16), qp, nullptr, 0, wx,
                      wx_ld, order, offsets, out, N, B, P, mid, G, mode, (hipStream_t)stream);
}

int vqa_att_attr_score_grouped_pairs_f16(const float* r1, const float* dscore, const void* vprime_f16, const float* qp,
                                         const int32_t* qrow, const float* wx, int wx_ld, const int32_t* order,
                                         const int32_t* offsets, float* out, int N, int B, int M, int P, int mid, int G, int mode,
                                         vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_BWD, (hipStream_t)stream);
  VQA_REQUIRE(qrow, "vqa_att_attr_score_grouped_pairs_f16: null qrow");
  VQA_REQUIRE(M >= 1, "vqa_att_attr_score_grouped_pairs_f16: M=%d question rows (>= 1)", M);
  return grouped_attr("vqa_att_attr_score_grouped_pairs_f16", r1, dscore, static_cast<const __half*>(vprime_f16), qp, qrow, M, wx,
                      wx_ld, order, offsets, out, N, B, P, mid, G, mode, (hipStream_t)stream);
}

// ---- gradient x input per question token: d logit / d q' through the scores
int vqa_att_attr_dq_grouped(const float* dscore, const float* vprime, const float* qp, const float* wx, int wx_ld,
                            const int32_t* order, const int32_t* offsets, float* dq_part, int N, int B, int P, int mid, int G,
                            int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_BWD, (hipStream_t)stream);
  return grouped_attr_dq("vqa_att_attr_dq_grouped", dscore, vprime, qp, wx, wx_ld, order, offsets, dq_part, N, B, P, mid, G, mode,
                         (hipStream_t)stream);
}

int vqa_att_attr_dq_grouped_f16(const float* dscore, const void* vprime_f16, const float* qp, const float* wx, int wx_ld,
                                const int32_t* order, const int32_t* offsets, float* dq_part, int N, int B, int P, int mid, int G,
                                int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_BWD, (hipStream_t)stream);
  return grouped_attr_dq("vqa_att_attr_dq_grouped_f16", dscore, static_cast<const __half*>(vprime_f16), qp, wx, wx_ld, order,
                         offsets, dq_part, N, B, P, mid, G, mode, (hipStream_t)stream);
}

// ---- integrated gradients along the path alpha * v' 
int vqa_att_path_scale_rows(float* x, int64_t ld, const float* alphas, int S, int64_t rows, int cols, vqa_stream_t stream) {
  const char* who = "vqa_att_path_scale_rows";
  VQA_REQUIRE(x, "%s: null pointer", who);
  const int rc = att_path_check(who, alphas, S);
  if (rc) return rc;
  VQA_REQUIRE(rows >= 0 && cols >= 1 && ld >= cols, "%s: rows=%lld, cols=%d, ld=%lld out of range (ld >= cols >= 1)", who,
              (long long)rows, cols, (long long)ld);
  if (rows == 0) return VQA_OK;
  hipLaunchKernelGGL(att_path_scale_rows_kernel, dim3(grid_for(rows * cols, 256)), dim3(256), 0, (hipStream_t)stream, x, ld, alphas,
                     S, rows, cols);
  return check_hip(hipGetLastError(), "att_path_scale_rows launch");
}

int vqa_att_path_score_grouped(const float* vprime, const float* qp, const float* wx, int wx_ld, const float* bx,
                               const float* alphas, const int32_t* order, const int32_t* offsets, float* score, int N, int B,
                               int S, int P, int mid, int G, int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_FWD, (hipStream_t)stream);
  return grouped_path_fwd("vqa_att_path_score_grouped", vprime, qp, nullptr, 0, wx, wx_ld, bx, alphas, order, offsets, score, N, B,
                          S, P, mid, G, mode, (hipStream_t)stream);
}

int vqa_att_path_score_grouped_pairs(const float* vprime, const float* qp, const int32_t* qrow, const float* wx, int wx_ld,
                                     const float* bx, const float* alphas, const int32_t* order, const int32_t* offsets,
                                     float* score, int N, int B, int M, int S, int P, int mid, int G, int mode,
                                     vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_FWD, (hipStream_t)stream);
  VQA_REQUIRE(qrow, "vqa_att_path_score_grouped_pairs: null qrow");
  VQA_REQUIRE(M >= 1, "vqa_att_path_score_grouped_pairs: M=%d question rows (>= 1)", M);
  return grouped_path_fwd("vqa_att_path_score_grouped_pairs", vprime, qp, qrow, M, wx, wx_ld, bx, alphas, order, offsets, score, N,
                          B, S, P, mid, G, mode, (hipStream_t)stream);
}

int vqa_att_path_score_grouped_f16(const void* vprime_f16, const float* qp, const float* wx, int wx_ld, const float* bx,
                                   const float* alphas, const int32_t* order, const int32_t* offsets, float* score, int N, int B,
                                   int S, int P, int mid, int G, int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_FWD, (hipStream_t)stream);
  return grouped_path_fwd("vqa_att_path_score_grouped_f16", static_cast<const __half*>(vprime_f16), qp, nullptr, 0, wx, wx_ld, bx,
                          alphas, order, offsets, score, N, B, S, P, mid, G, mode, (hipStream_t)stream);
}

int vqa_att_path_score_grouped_pairs_f16(const void* vprime_f16, const float* qp, const int32_t* qrow, const float* wx, int wx_ld,
                                         const float* bx, const float* alphas, const int32_t* order, const int32_t* offsets,
                                         float* score, int N, int B, int M, int S, int P, int mid, int G, int mode,
                                         vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_FWD, (hipStream_t)stream);
  VQA_REQUIRE(qrow, "vqa_att_path_score_grouped_pairs_f16: null qrow");
  VQA_REQUIRE(M >= 1, "vqa_att_path_score_grouped_pairs_f16: M=%d question rows (>= 1)", M);
  return grouped_path_fwd("vqa_att_path_score_grouped_pairs_f16", static_cast<const __half*>(vprime_f16), qp, qrow, M, wx, wx_ld,
                          bx, alphas, order, offsets, score, N, B, S, P, mid, G, mode, (hipStream_t)stream);
}

int vqa_att_path_attr_grouped(const float* r1, const float* dscore, const float* vprime, const float* qp, const float* wx,
                              int wx_ld, const float* alphas, float scale, const int32_t* order, const int32_t* offsets,
                              float* out, int N, int B, int S, int P, int mid, int G, int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_BWD, (hipStream_t)stream);
  return grouped_path_attr("vqa_att_path_attr_grouped", r1, dscore, vprime, qp, nullptr, 0, wx, wx_ld, alphas, scale, order,
                           offsets, out, N, B, S, P, mid, G, mode, (hipStream_t)stream);
}

int vqa_att_path_attr_grouped_pairs(const float* r1, const float* dscore, const float* vprime, const float* qp,
                                    const int32_t* qrow, const float* wx, int wx_ld, const float* alphas, float scale,
                                    const int32_t* order, const int32_t* offsets, float* out, int N, int B, int M, int S, int P,
                                    int mid, int G, int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_BWD, (hipStream_t)stream);
  VQA_REQUIRE(qrow, "vqa_att_path_attr_grouped_pairs: null qrow");
  VQA_REQUIRE(M >= 1, "vqa_att_path_attr_grouped_pairs: M=%d question rows (>= 1)", M);
  return grouped_path_attr("vqa_att_path_attr_grouped_pairs", r1, dscore, vprime, qp, qrow, M, wx, wx_ld, alphas, scale, order,
                           offsets, out, N, B, S, P, mid, G, mode, (hipStream_t)stream);
}

int vqa_att_path_attr_grouped_f16(const float* r1, const float* dscore, const void* vprime_f16, const float* qp, const float* wx,
                                  int wx_ld, const float* alphas, float scale, const int32_t* order, const int32_t* offsets,
                                  float* out, int N, int B, int S, int P, int mid, int G, int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_BWD, (hipStream_t)stream);
  return grouped_path_attr("vqa_att_path_attr_grouped_f16", r1, dscore, static_cast<const __half*>(vprime_f16), qp, nullptr, 0, wx,
                           wx_ld, alphas, scale, order, offsets, out, N, B, S, P, mid, G, mode, (hipStream_t)stream);
}

int vqa_att_path_attr_grouped_pairs_f16(const float* r1, const float* dscore, const void* vprime_f16, const float* qp,
                                        const int32_t* qrow, const float* wx, int wx_ld, const float* alphas, float scale,
                                        const int32_t* order, const int32_t* offsets, float* out, int N, int B, int M, int S,
                                        int P, int mid, int G, int mode, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_SCORE_BWD, (hipStream_t)stream);
  VQA_REQUIRE(qrow, "vqa_att_path_attr_grouped_pairs_f16: null qrow");
  VQA_REQUIRE(M >= 1, "vqa_att_path_attr_grouped_pairs_f16: M=%d question rows (>= 1)", M);
  return grouped_path_attr("vqa_att_path_attr_grouped_pairs_f16", r1, dscore, static_cast<const __half*>(vprime_f16), qp, qrow, M,
                           wx, wx_ld, alphas, scale, order, offsets, out, N, B, S, P, mid, G, mode, (hipStream_t)stream);
}

}  // extern "C"
