// Memory-bound stages of the VQA hot path: dropout, L2-norm, embedding+tanh, LSTM cell, attention
// softmax / weighted sum, soft-target cross entropy, reductions, Adam.
// All are HBM-bound streaming kernels: 16-byte per-lane accesses, wave64 shuffles for reductions.
#include <hip/hip_fp16.h>
#include "common.hpp"
#include "cache_load.hpp"

namespace vqa {

// ------------------------------------------------------------------ dropout
__global__ void dropout_kernel(const float* x, float* y, int64_t n, float p, float inv_keep, uint64_t seed) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = x[i] * drop_scale(seed, (uint64_t)i, p, inv_keep);
}

// y += dropout(x): 4 elements per thread and iteration
__global__ void dropout_add_kernel(const float* x, float* y, int64_t n, float p, float inv_keep, uint64_t seed) {
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 a = reinterpret_cast<const float4*>(x)[i];
    float4 b = reinterpret_cast<float4*>(y)[i];
    const float4 ds_ = drop_scale4(seed, (uint64_t)(4 * i), p, inv_keep);
    b.x += a.x * ds_.x; b.y += a.y * ds_.y; b.z += a.z * ds_.z; b.w += a.w * ds_.w;
    reinterpret_cast<float4*>(y)[i] = b;
  }
  if (blockIdx.x == 0 && threadIdx.x < n - 4 * n4) {
    const int64_t i = 4 * n4 + threadIdx.x;
    y[i] += x[i] * drop_scale(seed, (uint64_t)i, p, inv_keep);
  }
}

// ------------------------------------------------------------------ L2 norm (+ image dropout)
// one wave per row of C floats
// vdrop (optional, fp32 or bf16 by VB): dropout_{p2, seed2}(vn) written in the same pass
template <bool VB>
__global__ void l2norm_fwd_kernel(const float* pooled, float* vn, float* norm, int64_t rows, int C, float p,
                                  float inv_keep, uint64_t seed, void* vdrop, float p2, float inv_keep2, uint64_t seed2) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int nch = C >> 2;
  if (nch <= 64) {
    // C <= 256 (every config of the reference): a lane keeps its 4 channels in registers -- one pass over memory instead of
    // two -- and a wave has FOUR rows in flight (one 1-KB row per wave left the CU with 32 KB in flight: 3.9 TB/s).  Same
    // operations on every element as the general form below.
    constexpr int R = 4;
    const int c = lane;
    const bool cok = c < nch;
    for (int64_t r0 = R * wave; r0 < rows; r0 += R * nwaves) {
      float4 u[R];
#pragma unroll
      for (int k = 0; k < R; ++k)
        u[k] = (cok && r0 + k < rows) ? reinterpret_cast<const float4*>(pooled + (r0 + k) * C)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
      float ss[R];
#pragma unroll
      for (int k = 0; k < R; ++k) {
        if (p > 0.f) {
          const uint64_t e = (uint64_t)(r0 + k) * C + 4 * c;
          const float4 ds_ = drop_scale4(seed, e, p, inv_keep);
          u[k].x *= ds_.x; u[k].y *= ds_.y; u[k].z *= ds_.z; u[k].w *= ds_.w;
        }
        ss[k] = 0.f;
        ss[k] += u[k].x * u[k].x + u[k].y * u[k].y + u[k].z * u[k].z + u[k].w * u[k].w;
      }
#pragma unroll
      for (int k = 0; k < R; ++k) ss[k] = wave_sum(ss[k]);
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int64_t r = r0 + k;
        if (r >= rows) break;
        const float nrm = sqrtf(ss[k]);
        const float inv = 1.0f / (nrm + 1e-12f);
        if (lane == 0) norm[r] = nrm;
        if (!cok) continue;
        const float4 o = make_float4(u[k].x * inv, u[k].y * inv, u[k].z * inv, u[k].w * inv);
        reinterpret_cast<float4*>(vn + r * C)[c] = o;
        if (vdrop) {
          const uint64_t e = (uint64_t)r * C + 4 * c;
          float4 d = o;
          if (p2 > 0.f) {
            const float4 ds_ = drop_scale4(seed2, e, p2, inv_keep2);
            d.x *= ds_.x; d.y *= ds_.y; d.z *= ds_.z; d.w *= ds_.w;
          }
          if (VB) {
            uint2 w;
            w.x = f2bf16_pair(d.x, d.y); w.y = f2bf16_pair(d.z, d.w);
            reinterpret_cast<uint2*>(static_cast<uint16_t*>(vdrop) + r * C)[c] = w;
          } else {
            reinterpret_cast<float4*>(static_cast<float*>(vdrop) + r * C)[c] = d;
          }
        }
      }
    }
    return;
  }
  for (int64_t r = wave; r < rows; r += nwaves) {
    const float4* src = reinterpret_cast<const float4*>(pooled + r * C);
    float ss = 0.f;
    for (int c = lane; c < nch; c += 64) {
      float4 u = src[c];
      if (p > 0.f) {
        const uint64_t e = (uint64_t)r * C + 4 * c;
        { const float4 ds_ = drop_scale4(seed, e, p, inv_keep); u.x *= ds_.x; u.y *= ds_.y; u.z *= ds_.z; u.w *= ds_.w; }
      }
      ss += u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w;
    }
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss);
    const float inv = 1.0f / (nrm + 1e-12f);
    if (lane == 0) norm[r] = nrm;
    float4* dst = reinterpret_cast<float4*>(vn + r * C);
    for (int c = lane; c < nch; c += 64) {
      float4 u = src[c];
      if (p > 0.f) {
        const uint64_t e = (uint64_t)r * C + 4 * c;
        { const float4 ds_ = drop_scale4(seed, e, p, inv_keep); u.x *= ds_.x; u.y *= ds_.y; u.z *= ds_.z; u.w *= ds_.w; }
      }
      const float4 o = make_float4(u.x * inv, u.y * inv, u.z * inv, u.w * inv);
      dst[c] = o;
      if (vdrop) {
        const uint64_t e = (uint64_t)r * C + 4 * c;
        float4 d = o;
        if (p2 > 0.f) {
          { const float4 ds_ = drop_scale4(seed2, e, p2, inv_keep2); d.x *= ds_.x; d.y *= ds_.y; d.z *= ds_.z; d.w *= ds_.w; }
        }
        if (VB) {
          uint2 w;
          w.x = f2bf16_pair(d.x, d.y); w.y = f2bf16_pair(d.z, d.w);
          reinterpret_cast<uint2*>(static_cast<uint16_t*>(vdrop) + r * C)[c] = w;
        } else {
          reinterpret_cast<float4*>(static_cast<float*>(vdrop) + r * C)[c] = d;
        }
      }
    }
  }
}

// OB 1 / 2: the gradient is stored as bf16 (bf16 path: it is the pooled gradient of the last conv block, staged as bf16 anyway);
// 2: channel-blocked [image][C/16][position][16] -- what the routed patches of the patch convolutions read (a lane's 4
// channels are 8 bytes of one block; the four rows of a workgroup are consecutive positions = 128 contiguous bytes per block).
// G > 0: the incoming gradient is JOINED here instead of being read -- d loss / d vn = the weighted-sum branch
// sum_g probs[b][g][p] * dout[b][g][:] (what att_apply_bwd wrote as dvn) + dropout-mask * dv_in (what dropout_add added):
// two full passes over a [B*P][C] fp32 tensor less per step.  Same operations in the same order as the separate kernels.
template <int OB, int G>
__global__ void l2norm_bwd_kernel(const float* dvn, const float* vn, const float* norm, void* dpooled_,
                                  int64_t rows, int C, float p, float inv_keep, uint64_t seed, int positions,
                                  const float* dout, int64_t dout_ld, const float* probs, const float* dv_in, float p_v,
                                  float inv_keep_v, uint64_t seed_v) {
  float* const dpooled = static_cast<float*>(dpooled_);
  uint16_t* const dpooled16 = static_cast<uint16_t*>(dpooled_);
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int nch = C >> 2;
  if (nch <= 64) {
    // C <= 256 (every config of the reference): a lane holds its 4 channels of the row in registers -- one pass over memory
    // instead of two -- and a wave has TWO rows in flight
    const int c = lane;
    const bool cok = c < nch;
    for (int64_t r0 = 2 * wave; r0 < rows; r0 += 2 * nwaves) {
      float4 a[2], b[2];
      int64_t img[2], pos[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int64_t r = r0 + u < rows ? r0 + u : rows - 1;
        img[u] = G > 0 || OB == 2 ? r / positions : 0;
        pos[u] = r - img[u] * positions;
        b[u] = cok ? reinterpret_cast<const float4*>(vn + r * C)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        if (G == 0) {
          a[u] = cok ? reinterpret_cast<const float4*>(dvn + r * C)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
          float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
          if (cok) {
#pragma unroll
            for (int q = 0; q < (G > 0 ? G : 1); ++q) {
              const float pr = probs[(img[u] * G + q) * positions + pos[u]];
              const float4 go = reinterpret_cast<const float4*>(dout + img[u] * dout_ld + (int64_t)q * C)[c];
              o.x += pr * go.x; o.y += pr * go.y; o.z += pr * go.z; o.w += pr * go.w;
            }
            x = reinterpret_cast<const float4*>(dv_in + r * C)[c];
            if (p_v > 0.f) {
              const float4 ds_ = drop_scale4(seed_v, (uint64_t)r * C + 4 * c, p_v, inv_keep_v);
              x.x *= ds_.x; x.y *= ds_.y; x.z *= ds_.z; x.w *= ds_.w;
            }
          }
          a[u] = make_float4(o.x + x.x, o.y + x.y, o.z + x.z, o.w + x.w);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int64_t r = r0 + u;
        float dot = a[u].x * b[u].x + a[u].y * b[u].y + a[u].z * b[u].z + a[u].w * b[u].w;
        dot = wave_sum(dot);
        if (r >= rows) break;
        const float n = norm[r];
        const float inv = 1.0f / (n + 1e-12f);
        const float k = n > 0.f ? dot * (n + 1e-12f) / n : 0.f;
        if (!cok) continue;
        float4 d = make_float4((a[u].x - b[u].x * k) * inv, (a[u].y - b[u].y * k) * inv, (a[u].z - b[u].z * k) * inv,
                               (a[u].w - b[u].w * k) * inv);
        if (p > 0.f) {
          const float4 ds_ = drop_scale4(seed, (uint64_t)r * C + 4 * c, p, inv_keep);
          d.x *= ds_.x; d.y *= ds_.y; d.z *= ds_.z; d.w *= ds_.w;
        }
        if (OB) {
          typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
          const bf2 lo = {(__bf16)d.x, (__bf16)d.y}, hi = {(__bf16)d.z, (__bf16)d.w};
          const uint2 o = make_uint2(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi));
          if (OB == 2) *reinterpret_cast<uint2*>(dpooled16 + ((img[u] * (C >> 4) + (c >> 2)) * positions + pos[u]) * 16 + (c & 3) * 4) = o;
          else reinterpret_cast<uint2*>(dpooled16 + r * C)[c] = o;
        } else {
          reinterpret_cast<float4*>(dpooled + r * C)[c] = d;
        }
      }
    }
    return;
  }
  for (int64_t r = wave; r < rows; r += nwaves) {
    const float4* g = reinterpret_cast<const float4*>(dvn + r * C);
    const float4* v = reinterpret_cast<const float4*>(vn + r * C);
    const int64_t img = G > 0 || OB == 2 ? r / positions : 0;
    const int64_t pos = r - img * positions;
    float pr[G > 0 ? G : 1];
    if (G > 0) {
#pragma unroll
      for (int q = 0; q < G; ++q) pr[q] = probs[(img * G + q) * positions + pos];
    }
    auto grad = [&](int c) -> float4 {
      if (G == 0) return g[c];
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int q = 0; q < (G > 0 ? G : 1); ++q) {
        const float4 go = reinterpret_cast<const float4*>(dout + img * dout_ld + (int64_t)q * C)[c];
        o.x += pr[q] * go.x; o.y += pr[q] * go.y; o.z += pr[q] * go.z; o.w += pr[q] * go.w;
      }
      float4 x = reinterpret_cast<const float4*>(dv_in + r * C)[c];
      if (p_v > 0.f) {
        const float4 ds_ = drop_scale4(seed_v, (uint64_t)r * C + 4 * c, p_v, inv_keep_v);
        x.x *= ds_.x; x.y *= ds_.y; x.z *= ds_.z; x.w *= ds_.w;
      }
      return make_float4(o.x + x.x, o.y + x.y, o.z + x.z, o.w + x.w);
    };
    float dot = 0.f;
    for (int c = lane; c < nch; c += 64) {
      const float4 a = grad(c), b = v[c];
      dot += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    }
    dot = wave_sum(dot);
    const float n = norm[r];
    const float inv = 1.0f / (n + 1e-12f);
    const float k = n > 0.f ? dot * (n + 1e-12f) / n : 0.f;
    float4* dst = reinterpret_cast<float4*>(dpooled + r * C);
    uint2* dst16 = reinterpret_cast<uint2*>(dpooled16 + r * C);
    for (int c = lane; c < nch; c += 64) {
      const float4 a = grad(c), b = v[c];
      float4 d = make_float4((a.x - b.x * k) * inv, (a.y - b.y * k) * inv, (a.z - b.z * k) * inv, (a.w - b.w * k) * inv);
      if (p > 0.f) {
        const uint64_t e = (uint64_t)r * C + 4 * c;
        { const float4 ds_ = drop_scale4(seed, e, p, inv_keep); d.x *= ds_.x; d.y *= ds_.y; d.z *= ds_.z; d.w *= ds_.w; }
      }
      if (OB) {
        typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
        const bf2 lo = {(__bf16)d.x, (__bf16)d.y}, hi = {(__bf16)d.z, (__bf16)d.w};
        const uint2 o = make_uint2(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi));
        if (OB == 2) {
          *reinterpret_cast<uint2*>(dpooled16 + ((img * (C >> 4) + (c >> 2)) * positions + pos) * 16 + (c & 3) * 4) = o;
        } else {
          dst16[c] = o;
        }
      } else {
        dst[c] = d;
      }
    }
  }
}

// ------------------------------------------------------------------ embedding + dropout + tanh
// Token ids outside [0, V) (nn.Embedding raises for them, models/model.py:155) are COUNTED in *bad (device
// int32, optional) and treated as a zero embedding row in forward and backward alike; the host mirror raises
// from the counter (dl_vqa_amd/model.py).
__global__ void embed_tanh_fwd_kernel(const int64_t* q, const float* emb, float* x, int B, int T, int E, int V,
                                      float p, float inv_keep, uint64_t seed, int* bad) {
  const int64_t total = (int64_t)T * B * E;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int e = (int)(i % E);
    const int64_t tb = i / E;
    const int b = (int)(tb % B), t = (int)(tb / B);
    const int64_t tok = q[(int64_t)b * T + t];
    const bool ok = tok >= 0 && tok < V;
    if (!ok && e == 0 && bad) atomicAdd(bad, 1);
    float v = ok ? emb[tok * E + e] : 0.f;
    if (p > 0.f) v *= drop_scale(seed, ((uint64_t)b * T + t) * E + e, p, inv_keep);
    x[i] = tanhf(v);
  }
}

// One workgroup per vocabulary row v: scans the B*T token slots in index order, collects the slots whose token
// is v (ballot-ordered compaction through LDS) and adds their gradient rows in that fixed order, so the result
// is bitwise reproducible (no float atomics); rows that no slot references -- and row 0, the padding index,
// which receives no gradient -- are written as zeros, so demb needs no memset.
__global__ __launch_bounds__(256) void embed_tanh_bwd_kernel(const int64_t* q, const float* x, const float* dx,
                                                             float* demb, int B, int T, int E, int V, float p,
                                                             float inv_keep, uint64_t seed) {
  __shared__ int hits[256];
  __shared__ int wcount[4];
  const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = B * T;
  for (int e0 = 0; e0 < E; e0 += 1024) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (v != 0) {
      for (int s0 = 0; s0 < N; s0 += 256) {
        const int s = s0 + tid;
        const bool hit = s < N && q[s] == (int64_t)v;
        const int total = __syncthreads_count(hit);       // uniform; also fences the previous round's hits[]
        if (total == 0) continue;
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) wcount[wave] = __popcll(bal);
        __syncthreads();
        int base = 0;
        for (int w = 0; w < wave; ++w) base += wcount[w];
        if (hit) hits[base + __popcll(bal & ((1ull << lane) - 1ull))] = s;
        __syncthreads();
        for (int h = 0; h < total; ++h) {
          const int sl = hits[h];
          const int b = sl / T, t = sl - b * T;
          const int64_t row = ((int64_t)t * B + b) * E;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int e = e0 + tid + 256 * k;
            if (e < E) {
              const float xv = x[row + e];
              float g = dx[row + e] * (1.f - xv * xv);
              if (p > 0.f) g *= drop_scale(seed, ((uint64_t)b * T + t) * E + e, p, inv_keep);
              acc[k] += g;
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = e0 + tid + 256 * k;
      if (e < E) demb[(int64_t)v * E + e] = acc[k];
    }
  }
}

// The same result from a slot INDEX: the kernel above scans all B*T slots once per vocabulary row -- O(V * B*T)
// whatever the number of rows that are hit (hundreds of millions of reads at a real vocabulary with the stress shape).  With a
// workspace the slots are first binned by token (integer atomics: the bin CONTENTS are deterministic, their order is not), and a
// row's workgroup sorts its own bin ascending before it sums, so the summation order -- ascending slot index -- and therefore
// every bit of demb equal the scanning kernel's.  Bins above 1 024 slots (a token in more than 1 024 slots of one batch) fall
// back to the scan for that row only.
__global__ void embed_hist_kernel(const int64_t* q, int N, int V, int* counts) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N) return;
  const int64_t tok = q[s];
  if (tok > 0 && tok < V) atomicAdd(&counts[tok], 1);          // row 0 = padding index: no gradient
}
// offsets[v] = sum of counts[0..v), offsets[V] = total; cursor = a second copy for the fill pass.  One block of 1024 threads.
__global__ __launch_bounds__(1024) void embed_scan_kernel(const int* counts, int* offsets, int* cursor, int V) {
  __shared__ int part[1024];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int v0 = 0; v0 < V; v0 += 1024) {
    const int v = v0 + threadIdx.x;
    const int cnt = v < V ? counts[v] : 0;
    part[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                        // inclusive Hillis-Steele scan of the chunk
      const int add = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
      __syncthreads();
      part[threadIdx.x] += add;
      __syncthreads();
    }
    const int excl = carry + part[threadIdx.x] - cnt;
    if (v < V) { offsets[v] = excl; cursor[v] = excl; }
    __syncthreads();
    if (threadIdx.x == 1023) carry += part[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) offsets[V] = carry;
}
__global__ void embed_fill_kernel(const int64_t* q, int N, int V, int* cursor, int* slots) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N) return;
  const int64_t tok = q[s];
  if (tok > 0 && tok < V) slots[atomicAdd(&cursor[tok], 1)] = s;
}
constexpr int EMB_BIN_CAP = 1024;
__global__ __launch_bounds__(256) void embed_tanh_bwd_binned_kernel(const int64_t* q, const float* x, const float* dx, float* demb,
                                                                    int B, int T, int E, int V, float p, float inv_keep,
                                                                    uint64_t seed, const int* offsets, const int* slots) {
  __shared__ int bin[EMB_BIN_CAP];
  __shared__ int hits[256];
  __shared__ int wcount[4];
  const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = B * T;
  const int o0 = offsets[v], n = offsets[v + 1] - o0;
  if (n == 0) {                                                  // rows nothing references (and row 0): zeros
    for (int e = tid; e < E; e += 256) demb[(int64_t)v * E + e] = 0.f;
    return;
  }
  const bool binned = n <= EMB_BIN_CAP;
  if (binned) {
    int np2 = 2;
    while (np2 < n) np2 <<= 1;
    for (int i = tid; i < np2; i += 256) bin[i] = i < n ? slots[o0 + i] : 0x7fffffff;
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1)                           // bitonic sort, ascending
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < np2; i += 256) {
          const int l = i ^ j;
          if (l > i) {
            const int a = bin[i], bb = bin[l];
            const bool up = (i & k) == 0;
            if ((a > bb) == up) { bin[i] = bb; bin[l] = a; }
          }
        }
        __syncthreads();
      }
  }
  for (int e0 = 0; e0 < E; e0 += 1024) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    auto add_slot = [&](int sl) {
      const int b = sl / T, t = sl - b * T;
      const int64_t row = ((int64_t)t * B + b) * E;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = e0 + tid + 256 * k;
        if (e < E) {
          const float xv = x[row + e];
          float g = dx[row + e] * (1.f - xv * xv);
          if (p > 0.f) g *= drop_scale(seed, ((uint64_t)b * T + t) * E + e, p, inv_keep);
          acc[k] += g;
        }
      }
    };
    if (binned) {
      for (int h = 0; h < n; ++h) add_slot(bin[h]);
    } else {                                                     // an over-full bin: this row scans, as the kernel above
      for (int s0 = 0; s0 < N; s0 += 256) {
        const int s = s0 + tid;
        const bool hit = s < N && q[s] == (int64_t)v;
        const int total = __syncthreads_count(hit);
        if (total == 0) continue;
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) wcount[wave] = __popcll(bal);
        __syncthreads();
        int base = 0;
        for (int w = 0; w < wave; ++w) base += wcount[w];
        if (hit) hits[base + __popcll(bal & ((1ull << lane) - 1ull))] = s;
        __syncthreads();
        for (int h = 0; h < total; ++h) add_slot(hits[h]);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = e0 + tid + 256 * k;
      if (e < E) demb[(int64_t)v * E + e] = acc[k];
    }
  }
}

// ------------------------------------------------------------------ LSTM cell
__global__ void lstm_cell_fwd_kernel(const float* xg, const float* hg, const float* c_in, const float* h_in,
                                     const int64_t* q_len, int t, float* gates, float* c_out, float* h_out,
                                     float* c_final, int64_t cf_ld, int B, int H) {
  const int64_t total = (int64_t)B * H;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / H), j = (int)(i - (int64_t)b * H);
    const int64_t g0 = (int64_t)b * 4 * H + j;
    const float cp = c_in[i], hp = h_in[i];
    float cn = cp, hn = hp;
    float gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f;
    if ((int64_t)t < q_len[b]) {
      gi = sigmoidf_(xg[g0] + hg[g0]);
      gf = sigmoidf_(xg[g0 + H] + hg[g0 + H]);
      gg = tanhf(xg[g0 + 2 * H] + hg[g0 + 2 * H]);
      go = sigmoidf_(xg[g0 + 3 * H] + hg[g0 + 3 * H]);
      cn = gf * cp + gi * gg;
      hn = go * tanhf(cn);
    }
    gates[g0] = gi; gates[g0 + H] = gf; gates[g0 + 2 * H] = gg; gates[g0 + 3 * H] = go;
    c_out[i] = cn; h_out[i] = hn;
    if (c_final) c_final[(int64_t)b * cf_ld + j] = cn;
  }
}

__global__ void lstm_cell_bwd_kernel(const float* gates, const float* c_in, const float* c_out,
                                     const int64_t* q_len, int t, float* dh, float* dc, float* dgates, int B, int H) {
  const int64_t total = (int64_t)B * H;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / H), j = (int)(i - (int64_t)b * H);
    const int64_t g0 = (int64_t)b * 4 * H + j;
    float di = 0.f, df = 0.f, dg = 0.f, dgo = 0.f;
    if ((int64_t)t < q_len[b]) {
      const float gi = gates[g0], gf = gates[g0 + H], gg = gates[g0 + 2 * H], go = gates[g0 + 3 * H];
      const float tc = tanhf(c_out[i]);
      const float dhv = dh[i];
      const float dct = dc[i] + dhv * go * (1.f - tc * tc);
      di = dct * gg * gi * (1.f - gi);
      df = dct * c_in[i] * gf * (1.f - gf);
      dg = dct * gi * (1.f - gg * gg);
      dgo = dhv * tc * go * (1.f - go);
      dc[i] = dct * gf;
      dh[i] = 0.f;
    }
    dgates[g0] = di; dgates[g0 + H] = df; dgates[g0 + 2 * H] = dg; dgates[g0 + 3 * H] = dgo;
  }
}

// ------------------------------------------------------------------ softmax over positions + weighted sum
__device__ __forceinline__ float block_reduce(float v, float* red, bool is_max) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = is_max ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < nw; ++i) r = is_max ? fmaxf(r, red[i]) : r + red[i];
  return r;
}

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
// exit).  Otherwise n = b, and img / N are not read.
template <int G, bool GATHER>
__global__ void att_apply_fwd_v4_kernel(const float* score, const float* vn, const int* img, float* probs, float* out,
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

template <int G, bool GATHER>
__global__ void att_apply_fwd_kernel(const float* score, const float* vn, const int* img, float* probs, float* out,
                                     int64_t out_ld, int P, int C, int N) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  int n = blockIdx.x;
  if (GATHER) {
    n = img[blockIdx.x];
    if ((unsigned)n >= (unsigned)N) return;
  }
  att_apply_fwd_body<G>(sm, score, vn, probs, out, out_ld, P, C, blockIdx.x, n);
}

// vqa_att_apply_gather_fwd_f16: the two GATHER kernels above on a float16 vn (V4: C % 4 == 0 and vn 8-byte aligned)
template <int G, bool V4>
__global__ void att_apply_gather_fwd_f16_kernel(const float* score, const __half* vn, const int* img, float* probs, float* out,
                                                int64_t out_ld, int P, int C, int N) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int n = img[blockIdx.x];
  if ((unsigned)n >= (unsigned)N) return;
  if (V4) att_apply_fwd_v4_body<G>(sm, score, vn, probs, out, out_ld, P, C, blockIdx.x, n);
  else att_apply_fwd_body<G>(sm, score, vn, probs, out, out_ld, P, C, blockIdx.x, n);
}

// pass 1: one wave per (b,p): dprob -> dscore buffer, dvn row written
// One (sample b, position pp) row against the image row `v` that b weights there: dprob[b][g][pp] = <v, dout[b][g]> and
// (d != null) d[c] = sum_g probs[b][g][pp] * dout[b][g*C + c].  v: row b*P + pp in vqa_att_apply_bwd, row img[b]*P + pp in
// vqa_att_apply_gather_bwd -- the (sample, image) form, as in att_apply_fwd_body.  v: the row's first element, fp32 or fp16
// (cache_load.hpp), read a channel quad at a time.
template <int G, class VT>
__device__ __forceinline__ void att_apply_bwd_row(const float* dout, int64_t dout_ld, const float* probs, const VT* v,
                                                  float4* d, float* dprob, int64_t b, int pp, int P, int C, int lane) {
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
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float s = wave_sum(acc[g]);
    if (lane == 0) dprob[(b * G + g) * P + pp] = s;
  }
}

// GATHER (vqa_att_apply_gather_bwd, several questions per image): sample b weighted the rows of image img[b] of vn [N][P][C];
// dvn is null there -- the per-image sum is the kernel below.
template <int G, bool GATHER>
__global__ void att_apply_bwd_rows_kernel(const float* dout, int64_t dout_ld, const float* probs, const float* vn,
                                          const int* img, int N, float* dprob, float* dvn, int64_t M, int P, int C) {
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
    att_apply_bwd_row<G>(dout, dout_ld, probs, vn + vm * C, dvn ? reinterpret_cast<float4*>(dvn + m * C) : nullptr, dprob, b, pp,
                         P, C, lane);
  }
}

// vqa_att_apply_gather_dscore_f16: the GATHER rows kernel above on a float16 vn.  Nobody wants a gradient of a cache, so dvn
// is always null -- but it stays a run-time argument, as in the kernel above: the row body then compiles to the arithmetic
// (the same fused multiply-adds) of the fp32 instantiation, which a body specialised for d == null does not.
template <int G>
__global__ void att_apply_gather_rows_f16_kernel(const float* dout, int64_t dout_ld, const float* probs, const __half* vn,
                                                 const int* img, int N, float* dprob, float* dvn, int64_t M, int P, int C) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t m = wave; m < M; m += nwaves) {
    const int64_t b = m / P;
    const int pp = (int)(m - b * P);
    int n = img[b];
    n = n < 0 ? 0 : (n >= N ? N - 1 : n);                 // a malformed index reads nothing out of bounds
    att_apply_bwd_row<G>(dout, dout_ld, probs, vn + ((int64_t)n * P + pp) * C, dvn ? reinterpret_cast<float4*>(dvn + m * C) : nullptr,
                         dprob, b, pp, P, C, lane);
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

// ------------------------------------------------------------------ soft-target CE + VQA score
__global__ void softce_kernel(const float* logits, int64_t ld, const int64_t* a_idx, const int64_t* a_val, int kmax,
                              int A, float inv_batch, float* loss_rows, float* score_rows, float* dlogits, int64_t dld) {
  __shared__ float red[16];
  __shared__ int redi[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* row = logits + (int64_t)b * ld;
  float mx = -INFINITY;
  int am = 0x7fffffff;
  for (int i = tid; i < A; i += blockDim.x) { const float v = row[i]; if (v > mx) { mx = v; am = i; } }
  // arg-max with smallest-index tie break (torch.max returns the first maximal element)
  {
    const int lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(mx, o, 64);
      const int oi = __shfl_xor(am, o, 64);
      if (ov > mx || (ov == mx && oi < am)) { mx = ov; am = oi; }
    }
    if (lane == 0) { red[w] = mx; redi[w] = am; }
    __syncthreads();
    mx = red[0]; am = redi[0];
    for (int i = 1; i < nw; ++i) if (red[i] > mx || (red[i] == mx && redi[i] < am)) { mx = red[i]; am = redi[i]; }
  }
  float sum = 0.f;
  for (int i = tid; i < A; i += blockDim.x) sum += expf(row[i] - mx);
  sum = block_reduce(sum, red, false);
  // -log_softmax = log(sum) - (logit - max): both terms are >= 0, so nothing cancels.  (max + log(sum)) - logit rounds the
  // log-sum-exp at the magnitude of the logits: with a common offset of 1e4 that is 5e-4 absolute on a loss term of order 1.
  const float lsum = logf(sum);
  float wsum = 0.f, loss = 0.f, agree = 0.f;
  for (int k = 0; k < kmax; ++k) {
    const int64_t idx = a_idx[(int64_t)b * kmax + k];
    if (idx <= 0 || idx > A) continue;
    const float w = (float)a_val[(int64_t)b * kmax + k] / 10.0f;
    wsum += w;
    loss += w * (lsum - (row[idx - 1] - mx));
    if ((int)(idx - 1) == am) agree = (float)a_val[(int64_t)b * kmax + k];
  }
  if (tid == 0) {
    loss_rows[b] = loss * inv_batch;
    score_rows[b] = fminf(agree * 0.3f, 1.0f);
  }
  if (dlogits) {
    float* d = dlogits + (int64_t)b * dld;
    const float invs = 1.f / sum;
    for (int i = tid; i < A; i += blockDim.x) {
      float g = wsum * expf(row[i] - mx) * invs;
      for (int k = 0; k < kmax; ++k)
        if (a_idx[(int64_t)b * kmax + k] == (int64_t)i + 1) g -= (float)a_val[(int64_t)b * kmax + k] / 10.0f;
      d[i] = g * inv_batch;
    }
  }
}

// ------------------------------------------------------------------ column sums (two stage, deterministic)
// stage 1: grid (ceil(cols/64), splits); 256 threads = 4 row lanes x 64 columns
__global__ void colsum_stage1(const float* x, int64_t ld, const uint8_t* mask, int64_t rows, int cols,
                              int64_t rows_per, float* slab) {
  __shared__ float part[4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per;
  const int64_t r1 = r0 + rows_per < rows ? r0 + rows_per : rows;
  float acc = 0.f;
  if (c < cols)
    for (int64_t r = r0 + rl; r < r1; r += 4) {
      const float v = x[r * ld + c];
      if (!mask || mask[r * cols + c] != 4) acc += v;
    }
  part[rl][cl] = acc;
  __syncthreads();
  if (rl == 0 && c < cols) slab[(int64_t)blockIdx.y * cols + c] = part[0][cl] + part[1][cl] + part[2][cl] + part[3][cl];
}
__global__ void colsum_stage2(const float* slab, int splits, int cols, float* out, int accumulate) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  float v = 0.f;
  for (int s = 0; s < splits; ++s) v += slab[(int64_t)s * cols + c];
  out[c] = accumulate ? out[c] + v : v;
}

static void colsum_plan(int64_t rows, int cols, int* splits, int64_t* rows_per) {
  const int ctiles = (cols + 63) / 64;
  int64_t s = (1024 + ctiles - 1) / ctiles;          // aim for ~1024 workgroups
  const int64_t max_s = (rows + 63) / 64;            // at least 64 rows per split
  if (s > max_s) s = max_s;
  if (s < 1) s = 1;
  *rows_per = (rows + s - 1) / s;
  *splits = (int)((rows + *rows_per - 1) / *rows_per);
}
int64_t colsum_ws_bytes(int64_t rows, int cols) {
  int splits; int64_t rp;
  colsum_plan(rows, cols, &splits, &rp);
  return (int64_t)splits * cols * 4;
}
int colsum_launch(const float* x, int64_t ld, const uint8_t* mask, int64_t rows, int cols, float* out,
                  int accumulate, float* ws, int64_t ws_bytes, hipStream_t s) {
  int splits; int64_t rp;
  colsum_plan(rows, cols, &splits, &rp);
  if (!ws || ws_bytes < (int64_t)splits * cols * 4) {
    set_error("colsum: workspace %lld < %lld", (long long)ws_bytes, (long long)splits * cols * 4);
    return VQA_ERR_WORKSPACE;
  }
  hipLaunchKernelGGL(colsum_stage1, dim3((cols + 63) / 64, splits), dim3(256), 0, s, x, ld, mask, rows, cols, rp, ws);
  int rc = check_hip(hipGetLastError(), "colsum_stage1 launch");
  if (rc) return rc;
  hipLaunchKernelGGL(colsum_stage2, dim3((cols + 255) / 256), dim3(256), 0, s, ws, splits, cols, out, accumulate);
  return check_hip(hipGetLastError(), "colsum_stage2 launch");
}

// out[g] = sum_{b,p} x[b][g][p], deterministic two-stage sum inside one launch-pair-free kernel: grid (G), 1024
// threads; thread groups of 64 lanes take whole rows [b][g][:] (coalesced), partial sums combine in a fixed order.
// (The result is the x_conv bias gradient, ~0 by construction: softmax is shift invariant.)
__global__ __launch_bounds__(1024) void sum_bgp_kernel(const float* x, float* out, int B, int G, int P) {
  __shared__ float red[16];
  const int g = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;     // 16 waves, wave w takes samples w, w+16, ...
  float s = 0.f;
  for (int b = w; b < B; b += 16) {
    const float* row = x + ((int64_t)b * G + g) * P;
    for (int i = lane; i < P; i += 64) s += row[i];
  }
  s = block_reduce(s, red, false);
  if (threadIdx.x == 0) out[g] = s;
}

// out[b][n] = sum_r part[(b*parts + r)*cols + n]
__global__ void sum_parts_kernel(const float* part, float* out, int parts, int cols) {
  const int b = blockIdx.y;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  float v = 0.f;
  for (int r = 0; r < parts; ++r) v += part[((int64_t)b * parts + r) * cols + c];
  out[(int64_t)b * cols + c] = v;
}

__global__ void relu_drop_bwd_kernel(const float* y, const float* dy, float* dx, int64_t n, float p, float inv_keep,
                                     uint64_t seed) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float g = y[i] > 0.f ? dy[i] : 0.f;
    if (p > 0.f) g *= drop_scale(seed, (uint64_t)i, p, inv_keep);
    dx[i] = g;
  }
}

__global__ void add2d_kernel(const float* a, int64_t lda, const float* b, int64_t ldb, float* y, int64_t ldy,
                             int64_t rows, int cols) {
  const int64_t n = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols;
    const int c = (int)(i - r * cols);
    y[r * ldy + c] = a[r * lda + c] + (b ? b[r * ldb + c] : 0.f);
  }
}

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

template <bool VEC>
__global__ void gather_rows_drop_kernel(const float* src, const int* rows, float* dst, int n, int M, int64_t row_len,
                                        int64_t step_j, int64_t step_c, float p, float inv_keep, uint64_t seed) {
  gather_rows_drop_body<VEC>(src, rows, dst, n, M, row_len, step_j, step_c, p, inv_keep, seed);
}

// vqa_gather_rows_drop_f16: a float16 bank
template <bool VEC>
__global__ void gather_rows_drop_f16_kernel(const __half* src, const int* rows, float* dst, int n, int M, int64_t row_len,
                                            int64_t step_j, int64_t step_c, float p, float inv_keep, uint64_t seed) {
  gather_rows_drop_body<VEC>(src, rows, dst, n, M, row_len, step_j, step_c, p, inv_keep, seed);
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

__global__ void scale_by_kernel(float* x, int64_t n, const float* s) {
  const float k = *s;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] *= k;
}

__global__ void adam_kernel(float* p, const float* g, float* m, float* v, int64_t n, float step_size, float beta1,
                            float beta2, float eps, float inv_sqrt_bc2, float grad_scale) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float gr = g[i] * grad_scale;
    const float mi = beta1 * m[i] + (1.f - beta1) * gr;
    const float vi = beta2 * v[i] + (1.f - beta2) * gr * gr;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
    p[i] -= step_size * (mi / denom);
  }
}

// ---------------------------------------------------------------- Adam over a table of segments (vqa_adam_segments)
// A segment as the kernel reads it: bounds in float4 units, the host's bias-corrected scalars (as vqa_adam computes them),
// mode 0 = no decay (adam_kernel's arithmetic), 1 = L2 decay, 2 = decoupled decay (keep = 1 - lr * weight_decay).
struct AdamSeg {
  int64_t q0, q1;
  float step_size, beta1, beta2, eps, inv_sqrt_bc2, wd, keep;
  int mode;
};
struct AdamSegTable { AdamSeg s[VQA_ADAM_MAX_SEGMENTS]; };      // 3 KiB of the 4 KiB a launch may pass by value

// One element.  MODE 0 is adam_kernel's arithmetic, expression for expression and rounding for rounding: left to itself the
// compiler contracts the same expressions differently inside a float4 body (beta2 * v + t * gr becomes one packed fma here,
// a multiply and an add there), so contraction is off in this function and the three fused operations adam_kernel's code
// has -- the first moment, the denominator, the final update -- are written as fmaf.  tests/test_adam_groups_gpu.py holds the
// two kernels to the same bits.  The decay terms exist only in MODE 1 / 2.
template <int MODE>
__device__ __forceinline__ void adam_seg_elem(float& p, float g, float& m, float& v, const AdamSeg& s, float grad_scale) {
#pragma clang fp contract(off)
  float pi = p;
  float gr = g * grad_scale;
  if (MODE == 1) gr = gr + s.wd * pi;
  if (MODE == 2) pi = pi * s.keep;
  const float mi = fmaf(1.f - s.beta1, gr, s.beta1 * m);
  const float vi = s.beta2 * v + (1.f - s.beta2) * gr * gr;
  m = mi; v = vi;
  const float denom = fmaf(sqrtf(vi), s.inv_sqrt_bc2, s.eps);
  p = fmaf(-s.step_size, mi / denom, pi);
}
template <int MODE>
__device__ __forceinline__ void adam_seg_quad(float4& p, const float4& g, float4& m, float4& v, const AdamSeg& s, float grad_scale) {
  adam_seg_elem<MODE>(p.x, g.x, m.x, v.x, s, grad_scale);
  adam_seg_elem<MODE>(p.y, g.y, m.y, v.y, s, grad_scale);
  adam_seg_elem<MODE>(p.z, g.z, m.z, v.z, s, grad_scale);
  adam_seg_elem<MODE>(p.w, g.w, m.w, v.w, s, grad_scale);
}

// One lane owns a float4 and walks [first q0, last q1) with the grid's stride.  The table arrives by value; it is copied to LDS
// with a loop whose index is the same in every lane (a per-lane index into the argument would move it to scratch) and the lanes
// index the LDS copy.  The walk of a lane only moves forward, so its segment cursor does too: one 16-byte LDS read of the bounds
// per float4 while the lane stays inside a segment.  A float4 in a gap costs no global access.
__global__ __launch_bounds__(256) void adam_segments_kernel(float* p, const float* g, float* m, float* v, const AdamSegTable tab,
                                                             int n_segs, float grad_scale) {
  __shared__ AdamSeg seg[VQA_ADAM_MAX_SEGMENTS];
  for (int s = 0; s < n_segs; ++s)
    if (threadIdx.x == 0) seg[s] = tab.s[s];
  __syncthreads();
  const int64_t q_end = seg[n_segs - 1].q1, stride = (int64_t)gridDim.x * blockDim.x;
  int s = 0;
  for (int64_t q = seg[0].q0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < q_end; q += stride) {
    while (q >= seg[s].q1) ++s;                     // q < q_end = the last q1: s stays below n_segs
    if (q < seg[s].q0) continue;                    // between two segments
    const AdamSeg sg = seg[s];
    float4 pq = reinterpret_cast<const float4*>(p)[q];
    const float4 gq = reinterpret_cast<const float4*>(g)[q];
    float4 mq = reinterpret_cast<const float4*>(m)[q], vq = reinterpret_cast<const float4*>(v)[q];
    if (sg.mode == 0) adam_seg_quad<0>(pq, gq, mq, vq, sg, grad_scale);
    else if (sg.mode == 1) adam_seg_quad<1>(pq, gq, mq, vq, sg, grad_scale);
    else adam_seg_quad<2>(pq, gq, mq, vq, sg, grad_scale);
    reinterpret_cast<float4*>(m)[q] = mq;
    reinterpret_cast<float4*>(v)[q] = vq;
    reinterpret_cast<float4*>(p)[q] = pq;
  }
}

}  // namespace vqa

using namespace vqa;

#define STREAM ((hipStream_t)stream)

template <int G>
static void l2norm_bwd_launch(const float* dvn, const float* vn, const float* norm, void* dpooled, int mode, int64_t rows,
                              int positions, int C, float p, uint64_t seed, const float* dout, int64_t dout_ld,
                              const float* probs, const float* dv_in, float p_v, uint64_t seed_v, hipStream_t s) {
#define L2B(OB)                                                                                                            \
  hipLaunchKernelGGL((l2norm_bwd_kernel<OB, G>), dim3(grid_for(rows, 4)), dim3(256), 0, s, dvn, vn, norm, dpooled, rows, C, p, \
                     keep_scale(p), seed, positions, dout, dout_ld, probs, dv_in, p_v, keep_scale(p_v), seed_v)
  if (mode == 2) L2B(2); else if (mode == 1) L2B(1); else L2B(0);
#undef L2B
}

// ---------------------------------------------------------------- softmax + weighted sum: the host side of vqa_att_apply_*
// dynamic LDS of both forward kernels (the scalar one uses less of it): probs [G][P], 16 reduction slots, part [16][G][64]
static size_t att_apply_fwd_lds(int G, int P) { return ((size_t)G * P + 16 + 16 * G * 64) * 4; }

static uintptr_t quad_bits(const void* a, const void* b, const void* c) {
  return reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c);
}

// What the five entry points check, before any HIP call (`who` names the caller in the messages).  backward: the kernels
// read dout / vn and write dvn as float4, so C and the leading dimension are multiples of 4 and `quads` (quad_bits of those
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

// img == null: sample b weights its own image (vqa_att_apply_fwd), N is not read.  The 16-byte kernels need whole quads
// of channels and an aligned vn; anything else runs the scalar ones.
static int att_apply_fwd_launch(const float* score, const float* vn, const int32_t* img, float* probs, float* out,
                                int64_t out_ld, int N, int B, int P, int C, int G, hipStream_t s) {
  if (B == 0) return VQA_OK;
  const dim3 grid(B, (C + 63) / 64);
  const size_t lds = att_apply_fwd_lds(G, P);
  return with_int14(G, [&](auto g) {
    return with_flags(C % 4 == 0 && (reinterpret_cast<uintptr_t>(vn) & 15) == 0, img != nullptr, [&](auto v4, auto gather) {
      if (decltype(v4)::value)
        hipLaunchKernelGGL((att_apply_fwd_v4_kernel<decltype(g)::value, decltype(gather)::value>), grid, dim3(256), lds, s, score,
                           vn, img, probs, out, out_ld, P, C, N);
      else
        hipLaunchKernelGGL((att_apply_fwd_kernel<decltype(g)::value, decltype(gather)::value>), grid, dim3(256), lds, s, score,
                           vn, img, probs, out, out_ld, P, C, N);
      return check_hip(hipGetLastError(), "att_apply_fwd launch");
    });
  });
}

// img == null: the plain form, whose rows kernel writes dvn [B][P][C] itself (dvn == null: nobody wants it).  With img the
// rows kernel leaves dvn alone, and order / offsets (with dvn [N][P][C]) add the per-image sum; then the softmax backward.
static int att_apply_bwd_launch(const float* dout, int64_t dout_ld, const float* probs, const float* vn, const int32_t* img,
                                const int32_t* order, const int32_t* offsets, float* dscore, float* dvn, float* dscore_rowsum,
                                int N, int B, int P, int C, int G, hipStream_t s) {
  if (B == 0) return VQA_OK;
  const int64_t M = (int64_t)B * P, Mn = (int64_t)N * P;
  int rc = with_int14(G, [&](auto g) {
    return with_flag(img != nullptr, [&](auto gather) {
      hipLaunchKernelGGL((att_apply_bwd_rows_kernel<decltype(g)::value, decltype(gather)::value>), dim3(grid_for(M, 4)), dim3(256),
                         0, s, dout, dout_ld, probs, vn, img, N, dscore, decltype(gather)::value ? nullptr : dvn, M, P, C);
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

// The float16-vn forms (a float16 image-feature cache): the gather forward and the dscore half of the gather backward, the
// same grids, blocks and LDS sizes.  The forward's quad kernel needs whole quads of channels and an 8-byte aligned vn.
static int att_apply_gather_fwd_f16_launch(const float* score, const __half* vn, const int32_t* img, float* probs, float* out,
                                           int64_t out_ld, int N, int B, int P, int C, int G, hipStream_t s) {
  if (B == 0) return VQA_OK;
  const dim3 grid(B, (C + 63) / 64);
  const size_t lds = att_apply_fwd_lds(G, P);
  return with_int14(G, [&](auto g) {
    return with_flag(C % 4 == 0 && (reinterpret_cast<uintptr_t>(vn) & 7) == 0, [&](auto v4) {
      hipLaunchKernelGGL((att_apply_gather_fwd_f16_kernel<decltype(g)::value, decltype(v4)::value>), grid, dim3(256), lds, s, score,
                         vn, img, probs, out, out_ld, P, C, N);
      return check_hip(hipGetLastError(), "att_apply_gather_fwd_f16 launch");
    });
  });
}

static int att_apply_gather_dscore_f16_launch(const float* dout, int64_t dout_ld, const float* probs, const __half* vn,
                                              const int32_t* img, float* dscore, float* dscore_rowsum, int N, int B, int P, int C,
                                              int G, hipStream_t s) {
  if (B == 0) return VQA_OK;
  const int64_t M = (int64_t)B * P;
  const int rc = with_int14(G, [&](auto g) {
    hipLaunchKernelGGL(att_apply_gather_rows_f16_kernel<decltype(g)::value>, dim3(grid_for(M, 4)), dim3(256), 0, s, dout, dout_ld,
                       probs, vn, img, N, dscore, (float*)nullptr, M, P, C);
    return check_hip(hipGetLastError(), "att_apply_gather_rows_f16 launch");
  });
  if (rc) return rc;
  hipLaunchKernelGGL(softmax_bwd_kernel, dim3(B * G), dim3(256), 0, s, probs, dscore, P, dscore_rowsum);
  return check_hip(hipGetLastError(), "softmax_bwd launch");
}

extern "C" {

int vqa_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, vqa_stream_t stream) {
  set_launch_tag(n >= (1 << 22) ? 1 : 0);       // 1 = a large tensor (the attention dropout on v), 0 = the small sites
  ProfScope prof(VQA_K_DROPOUT, (hipStream_t)stream);
  VQA_REQUIRE(x && y && n >= 0 && p >= 0.f && p < 1.f, "vqa_dropout: bad args");
  if (n == 0) return VQA_OK;
  hipLaunchKernelGGL(dropout_kernel, dim3(grid_for(n, 256)), dim3(256), 0, STREAM, x, y, n, p, keep_scale(p), seed);
  return check_hip(hipGetLastError(), "dropout launch");
}

int vqa_dropout_add(const float* x, float* y, int64_t n, float p, uint64_t seed, vqa_stream_t stream) {
  set_launch_tag(n >= (1 << 22) ? 1 : 0);
  ProfScope prof(VQA_K_DROPOUT, (hipStream_t)stream);
  VQA_REQUIRE(x && y && n > 0 && p >= 0.f && p < 1.f, "vqa_dropout_add: bad args");
  VQA_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0, "vqa_dropout_add: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(dropout_add_kernel, dim3(grid_for(n / 4 + 1, 256)), dim3(256), 0, STREAM, x, y, n, p, keep_scale(p), seed);
  return check_hip(hipGetLastError(), "dropout_add launch");
}

int vqa_l2norm_fwd(const float* pooled, float* vn, float* norm, int64_t rows, int C, float p, uint64_t seed,
                   void* vdrop, int vdrop_is_bf16, float p2, uint64_t seed2, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_L2NORM_FWD, (hipStream_t)stream);
  VQA_REQUIRE(pooled && vn && norm && rows > 0 && C > 0 && C % 4 == 0, "vqa_l2norm_fwd: bad args (C=%d)", C);
  VQA_REQUIRE(p2 >= 0.f && p2 < 1.f, "vqa_l2norm_fwd: p2 must be in [0, 1)");
  if (vdrop && vdrop_is_bf16)
    hipLaunchKernelGGL(l2norm_fwd_kernel<true>, dim3(grid_for(rows, 4)), dim3(256), 0, STREAM, pooled, vn, norm, rows, C, p,
                       keep_scale(p), seed, vdrop, p2, keep_scale(p2), seed2);
  else
    hipLaunchKernelGGL(l2norm_fwd_kernel<false>, dim3(grid_for(rows, 4)), dim3(256), 0, STREAM, pooled, vn, norm, rows, C, p,
                       keep_scale(p), seed, vdrop, p2, keep_scale(p2), seed2);
  return check_hip(hipGetLastError(), "l2norm_fwd launch");
}

int vqa_l2norm_bwd(const float* dvn, const float* vn, const float* norm, void* dpooled, int dpooled_mode, int64_t rows,
                   int positions, int C, float p, uint64_t seed, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_L2NORM_BWD, (hipStream_t)stream);
  VQA_REQUIRE(dvn && vn && norm && dpooled && rows > 0 && C % 4 == 0 && dpooled_mode >= 0 && dpooled_mode <= 2, "vqa_l2norm_bwd: bad args");
  VQA_REQUIRE(dpooled_mode != 2 || (C % 16 == 0 && positions > 0 && rows % positions == 0),
              "vqa_l2norm_bwd: the channel-blocked output needs C %% 16 == 0 and rows = images x positions (C=%d, positions=%d)", C, positions);
  l2norm_bwd_launch<0>(dvn, vn, norm, dpooled, dpooled_mode, rows, positions > 0 ? positions : 1, C, p, seed, nullptr, 0, nullptr,
                       nullptr, 0.f, 0, STREAM);
  return check_hip(hipGetLastError(), "l2norm_bwd launch");
}

int vqa_l2norm_bwd_joined(const float* dout, int64_t dout_ld, const float* probs, int G, const float* dv_in, float p_v,
                          uint64_t seed_v, const float* vn, const float* norm, void* dpooled, int dpooled_mode, int64_t rows,
                          int positions, int C, float p, uint64_t seed, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_L2NORM_BWD, (hipStream_t)stream);
  VQA_REQUIRE(dout && probs && dv_in && vn && norm && dpooled && rows > 0 && C % 4 == 0 && dout_ld % 4 == 0 && dpooled_mode >= 0 &&
                  dpooled_mode <= 2 && positions > 0 && rows % positions == 0, "vqa_l2norm_bwd_joined: bad args");
  VQA_REQUIRE(dpooled_mode != 2 || C % 16 == 0, "vqa_l2norm_bwd_joined: the channel-blocked output needs C %% 16 == 0 (C=%d)", C);
  VQA_REQUIRE(G >= 1 && G <= 4, "glimpses=%d unsupported (1..4)", G);
  return with_int14(G, [&](auto g) {
    l2norm_bwd_launch<decltype(g)::value>(nullptr, vn, norm, dpooled, dpooled_mode, rows, positions, C, p, seed, dout, dout_ld,
                                          probs, dv_in, p_v, seed_v, STREAM);
    return check_hip(hipGetLastError(), "l2norm_bwd_joined launch");
  });
}

int vqa_embed_tanh_fwd(const int64_t* q, const float* emb, float* x, int B, int T, int E, int V, float p,
                       uint64_t seed, int32_t* bad_tokens, vqa_stream_t stream) {
  VQA_REQUIRE(q && emb && x && B > 0 && T > 0 && E > 0 && V > 0, "vqa_embed_tanh_fwd: bad args");
  hipLaunchKernelGGL(embed_tanh_fwd_kernel, dim3(grid_for((int64_t)B * T * E, 256)), dim3(256), 0, STREAM, q, emb, x,
                     B, T, E, V, p, keep_scale(p), seed, bad_tokens);
  return check_hip(hipGetLastError(), "embed_tanh_fwd launch");
}

int64_t vqa_embed_tanh_bwd_workspace_bytes(int B, int T, int V) {
  if (B <= 0 || T <= 0 || V <= 0) return 0;
  return ((int64_t)3 * V + 2 + (int64_t)B * T) * 4;             // counts[V] offsets[V+1] cursor[V] slots[B*T] (int32)
}

int vqa_embed_tanh_bwd(const int64_t* q, const float* x, const float* dx, float* demb, int B, int T, int E, int V,
                       float p, uint64_t seed, void* workspace, int64_t workspace_bytes, vqa_stream_t stream) {
  VQA_REQUIRE(q && x && dx && demb && B > 0 && T > 0 && E > 0 && V > 0, "vqa_embed_tanh_bwd: bad args");
  if (!workspace) {                                              // no workspace: the scanning kernel, O(V * B*T)
    hipLaunchKernelGGL(embed_tanh_bwd_kernel, dim3(V), dim3(256), 0, STREAM, q, x, dx, demb, B, T, E, V, p, keep_scale(p), seed);
    return check_hip(hipGetLastError(), "embed_tanh_bwd launch");
  }
  if (workspace_bytes < vqa_embed_tanh_bwd_workspace_bytes(B, T, V)) {
    set_error("vqa_embed_tanh_bwd: workspace %lld < %lld", (long long)workspace_bytes,
              (long long)vqa_embed_tanh_bwd_workspace_bytes(B, T, V));
    return VQA_ERR_WORKSPACE;
  }
  const int N = B * T;
  int* const counts = static_cast<int*>(workspace);
  int* const offsets = counts + V;
  int* const cursor = offsets + V + 1;
  int* const slots = cursor + V;
  int rc = check_hip(hipMemsetAsync(counts, 0, (size_t)V * 4, STREAM), "embed_tanh_bwd memset");
  if (rc) return rc;
  hipLaunchKernelGGL(embed_hist_kernel, dim3((N + 255) / 256), dim3(256), 0, STREAM, q, N, V, counts);
  hipLaunchKernelGGL(embed_scan_kernel, dim3(1), dim3(1024), 0, STREAM, counts, offsets, cursor, V);
  hipLaunchKernelGGL(embed_fill_kernel, dim3((N + 255) / 256), dim3(256), 0, STREAM, q, N, V, cursor, slots);
  hipLaunchKernelGGL(embed_tanh_bwd_binned_kernel, dim3(V), dim3(256), 0, STREAM, q, x, dx, demb, B, T, E, V, p, keep_scale(p), seed,
                     offsets, slots);
  return check_hip(hipGetLastError(), "embed_tanh_bwd(binned) launch");
}

int vqa_lstm_cell_fwd(const float* xg, const float* hg, const float* c_in, const float* h_in, const int64_t* q_len,
                      int t, float* gates, float* c_out, float* h_out, float* c_final, int64_t cf_ld, int B, int H,
                      vqa_stream_t stream) {
  VQA_REQUIRE(xg && hg && c_in && h_in && q_len && gates && c_out && h_out, "vqa_lstm_cell_fwd: null pointer");
  hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(grid_for((int64_t)B * H, 256)), dim3(256), 0, STREAM, xg, hg, c_in,
                     h_in, q_len, t, gates, c_out, h_out, c_final, cf_ld, B, H);
  return check_hip(hipGetLastError(), "lstm_cell_fwd launch");
}

int vqa_lstm_cell_bwd(const float* gates, const float* c_in, const float* c_out, const int64_t* q_len, int t,
                      float* dh, float* dc, float* dgates, int B, int H, vqa_stream_t stream) {
  VQA_REQUIRE(gates && c_in && c_out && q_len && dh && dc && dgates, "vqa_lstm_cell_bwd: null pointer");
  hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(grid_for((int64_t)B * H, 256)), dim3(256), 0, STREAM, gates, c_in,
                     c_out, q_len, t, dh, dc, dgates, B, H);
  return check_hip(hipGetLastError(), "lstm_cell_bwd launch");
}

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
                                 quad_bits(dout, vn, dvn));
  return rc ? rc : att_apply_bwd_launch(dout, dout_ld, probs, vn, nullptr, nullptr, nullptr, dscore, dvn, dscore_rowsum, 0, B, P,
                                        C, G, STREAM);
}

int vqa_att_apply_gather_bwd(const float* dout, int64_t dout_ld, const float* probs, const float* vn, const int32_t* img,
                             const int32_t* order, const int32_t* offsets, float* dscore, float* dvn, float* dscore_rowsum,
                             int N, int B, int P, int C, int G, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_APPLY_BWD, (hipStream_t)stream);
  const int rc = att_apply_check("vqa_att_apply_gather_bwd", true, dout && probs && vn && dscore && dvn, img && order && offsets,
                                 N, B, P, C, G, dout_ld, quad_bits(dout, vn, dvn));
  return rc ? rc : att_apply_bwd_launch(dout, dout_ld, probs, vn, img, order, offsets, dscore, dvn, dscore_rowsum, N, B, P, C, G,
                                        STREAM);
}

int vqa_att_apply_gather_dscore(const float* dout, int64_t dout_ld, const float* probs, const float* vn, const int32_t* img,
                                float* dscore, float* dscore_rowsum, int N, int B, int P, int C, int G, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_APPLY_BWD, (hipStream_t)stream);
  const int rc = att_apply_check("vqa_att_apply_gather_dscore", true, dout && probs && vn && dscore, img, N, B, P, C, G, dout_ld,
                                 quad_bits(dout, vn, nullptr));
  return rc ? rc : att_apply_bwd_launch(dout, dout_ld, probs, vn, img, nullptr, nullptr, dscore, nullptr, dscore_rowsum, N, B, P,
                                        C, G, STREAM);
}

int vqa_softce_fwd_bwd(const float* logits, int64_t ld, const int64_t* a_idx, const int64_t* a_val, int kmax, int B,
                       int A, float inv_batch, float* loss_rows, float* score_rows, float* dlogits, int64_t dld,
                       vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_SOFTCE, (hipStream_t)stream);
  VQA_REQUIRE(logits && a_idx && a_val && loss_rows && score_rows && B > 0 && A > 0 && kmax >= 0,
              "vqa_softce_fwd_bwd: bad args");
  hipLaunchKernelGGL(softce_kernel, dim3(B), dim3(256), 0, STREAM, logits, ld, a_idx, a_val, kmax, A, inv_batch,
                     loss_rows, score_rows, dlogits, dld);
  return check_hip(hipGetLastError(), "softce launch");
}

int64_t vqa_colsum_workspace_bytes(int64_t rows, int cols) { return colsum_ws_bytes(rows, cols); }

int vqa_colsum(const float* x, int64_t ld, const uint8_t* mask, int64_t rows, int cols, float* out, int accumulate,
               float* workspace, int64_t workspace_bytes, vqa_stream_t stream) {
  VQA_REQUIRE(x && out && rows > 0 && cols > 0, "vqa_colsum: bad args");
  VQA_REQUIRE(!mask || ld == cols, "vqa_colsum: masked form needs ld == cols");
  return colsum_launch(x, ld, mask, rows, cols, out, accumulate, workspace, workspace_bytes, STREAM);
}

int vqa_sum_bgp(const float* x, float* out, int B, int G, int P, vqa_stream_t stream) {
  VQA_REQUIRE(x && out, "vqa_sum_bgp: null pointer");
  hipLaunchKernelGGL(sum_bgp_kernel, dim3(G), dim3(1024), 0, STREAM, x, out, B, G, P);
  return check_hip(hipGetLastError(), "sum_bgp launch");
}

int vqa_sum_parts(const float* part, float* out, int batch, int parts, int cols, vqa_stream_t stream) {
  VQA_REQUIRE(part && out && batch > 0 && parts > 0 && cols > 0, "vqa_sum_parts: bad args");
  hipLaunchKernelGGL(sum_parts_kernel, dim3((cols + 255) / 256, batch), dim3(256), 0, STREAM, part, out, parts, cols);
  return check_hip(hipGetLastError(), "sum_parts launch");
}

int vqa_relu_drop_bwd(const float* y, const float* dy, float* dx, int64_t n, float p, uint64_t seed,
                      vqa_stream_t stream) {
  VQA_REQUIRE(y && dy && dx, "vqa_relu_drop_bwd: null pointer");
  hipLaunchKernelGGL(relu_drop_bwd_kernel, dim3(grid_for(n, 256)), dim3(256), 0, STREAM, y, dy, dx, n, p, keep_scale(p), seed);
  return check_hip(hipGetLastError(), "relu_drop_bwd launch");
}

int vqa_add2d(const float* a, int64_t lda, const float* b, int64_t ldb, float* y, int64_t ldy, int64_t rows,
              int cols, vqa_stream_t stream) {
  VQA_REQUIRE(a && y && rows > 0 && cols > 0, "vqa_add2d: bad args");
  hipLaunchKernelGGL(add2d_kernel, dim3(grid_for(rows * cols, 256)), dim3(256), 0, STREAM, a, lda, b, ldb, y, ldy,
                     rows, cols);
  return check_hip(hipGetLastError(), "add2d launch");
}

int vqa_gather_rows(const float* src, int64_t src_ld, const int32_t* rows, float* dst, int64_t dst_ld, int B, int M, int cols,
                    vqa_stream_t stream) {
  VQA_REQUIRE(src && rows && dst, "vqa_gather_rows: null pointer");
  VQA_REQUIRE(B >= 0 && M >= 1 && cols >= 1, "vqa_gather_rows: B=%d, M=%d, cols=%d out of range", B, M, cols);
  VQA_REQUIRE(src_ld >= cols && dst_ld >= cols, "vqa_gather_rows: src_ld=%lld and dst_ld=%lld must be >= cols=%d",
              (long long)src_ld, (long long)dst_ld, cols);
  if (B == 0) return VQA_OK;
  const bool vec = cols % 4 == 0 && src_ld % 4 == 0 && dst_ld % 4 == 0 &&
                   ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
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
  VQA_REQUIRE(src && rows && dst, "vqa_gather_rows_drop: null pointer");
  VQA_REQUIRE(n >= 0 && M >= 1 && row_len >= 1, "vqa_gather_rows_drop: n=%d, M=%d, row_len=%lld out of range", n, M,
              (long long)row_len);
  VQA_REQUIRE(p >= 0.f && p < 1.f, "vqa_gather_rows_drop: p=%g outside [0, 1)", (double)p);
  if (n == 0) return VQA_OK;
  const bool vec = row_len % 4 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  const int64_t rw = vec ? row_len / 4 : row_len;
  const int grid = grid_for((int64_t)n * rw, 256);
  const int64_t stride = (int64_t)grid * 256;
  if (vec)
    hipLaunchKernelGGL(gather_rows_drop_kernel<true>, dim3(grid), dim3(256), 0, STREAM, src, rows, dst, n, M, row_len,
                       stride / rw, stride % rw, p, keep_scale(p), seed);
  else
    hipLaunchKernelGGL(gather_rows_drop_kernel<false>, dim3(grid), dim3(256), 0, STREAM, src, rows, dst, n, M, row_len,
                       stride / rw, stride % rw, p, keep_scale(p), seed);
  return check_hip(hipGetLastError(), "gather_rows_drop launch");
}

int vqa_half_to_float(const void* x_f16, float* y, int64_t n, vqa_stream_t stream) {
  VQA_REQUIRE(x_f16 && y && n > 0, "vqa_half_to_float: bad args");
  VQA_REQUIRE(((uintptr_t)x_f16 % 16) == 0 && ((uintptr_t)y % 16) == 0, "vqa_half_to_float: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(half_to_float_kernel, dim3(grid_for(n / 8 + 1, 256)), dim3(256), 0, STREAM,
                     static_cast<const __half*>(x_f16), y, n);
  return check_hip(hipGetLastError(), "half_to_float launch");
}

// ---- float16 image-feature caches: the converter and the cache readers of this file on a half operand
int vqa_float_to_half(const float* x, void* y_f16, int64_t n, vqa_stream_t stream) {
  VQA_REQUIRE(x && y_f16 && n >= 0, "vqa_float_to_half: bad args");
  VQA_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)y_f16 % 16) == 0, "vqa_float_to_half: pointers must be 16-byte aligned");
  if (n == 0) return VQA_OK;
  hipLaunchKernelGGL(float_to_half_kernel, dim3(grid_for(n / 8 + 1, 256)), dim3(256), 0, STREAM, x, static_cast<__half*>(y_f16), n);
  return check_hip(hipGetLastError(), "float_to_half launch");
}

int vqa_gather_rows_drop_f16(const void* src_f16, const int32_t* rows, float* dst, int n, int M, int64_t row_len, float p,
                             uint64_t seed, vqa_stream_t stream) {
  VQA_REQUIRE(src_f16 && rows && dst, "vqa_gather_rows_drop_f16: null pointer");
  VQA_REQUIRE(n >= 0 && M >= 1 && row_len >= 1, "vqa_gather_rows_drop_f16: n=%d, M=%d, row_len=%lld out of range", n, M,
              (long long)row_len);
  VQA_REQUIRE(p >= 0.f && p < 1.f, "vqa_gather_rows_drop_f16: p=%g outside [0, 1)", (double)p);
  VQA_REQUIRE((reinterpret_cast<uintptr_t>(src_f16) & 1) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0,
              "vqa_gather_rows_drop_f16: src must be 2-byte and dst 4-byte aligned");
  if (n == 0) return VQA_OK;
  const __half* src = static_cast<const __half*>(src_f16);
  // the quad path: 8-byte loads of the bank, 16-byte stores
  const bool vec = row_len % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 7) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  const int64_t rw = vec ? row_len / 4 : row_len;
  const int grid = grid_for((int64_t)n * rw, 256);
  const int64_t stride = (int64_t)grid * 256;
  if (vec)
    hipLaunchKernelGGL(gather_rows_drop_f16_kernel<true>, dim3(grid), dim3(256), 0, STREAM, src, rows, dst, n, M, row_len,
                       stride / rw, stride % rw, p, keep_scale(p), seed);
  else
    hipLaunchKernelGGL(gather_rows_drop_f16_kernel<false>, dim3(grid), dim3(256), 0, STREAM, src, rows, dst, n, M, row_len,
                       stride / rw, stride % rw, p, keep_scale(p), seed);
  return check_hip(hipGetLastError(), "gather_rows_drop_f16 launch");
}

int vqa_att_apply_gather_fwd_f16(const float* score, const void* vn_f16, const int32_t* img, float* probs, float* out,
                                 int64_t out_ld, int N, int B, int P, int C, int G, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_APPLY_FWD, (hipStream_t)stream);
  const int rc = att_apply_check("vqa_att_apply_gather_fwd_f16", false, score && vn_f16 && probs && out, img, N, B, P, C, G, out_ld,
                                 0);
  if (rc) return rc;
  VQA_REQUIRE((reinterpret_cast<uintptr_t>(vn_f16) & 1) == 0, "vqa_att_apply_gather_fwd_f16: vn must be 2-byte aligned");
  return att_apply_gather_fwd_f16_launch(score, static_cast<const __half*>(vn_f16), img, probs, out, out_ld, N, B, P, C, G, STREAM);
}

int vqa_att_apply_gather_dscore_f16(const float* dout, int64_t dout_ld, const float* probs, const void* vn_f16,
                                    const int32_t* img, float* dscore, float* dscore_rowsum, int N, int B, int P, int C, int G,
                                    vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ATT_APPLY_BWD, (hipStream_t)stream);
  const int rc = att_apply_check("vqa_att_apply_gather_dscore_f16", true, dout && probs && vn_f16 && dscore, img, N, B, P, C, G,
                                 dout_ld, quad_bits(dout, nullptr, nullptr));
  if (rc) return rc;
  // the rows kernel reads a quad of halves as 8 bytes where the fp32 form reads 16
  VQA_REQUIRE((reinterpret_cast<uintptr_t>(vn_f16) & 7) == 0, "vqa_att_apply_gather_dscore_f16: vn must be 8-byte aligned");
  return att_apply_gather_dscore_f16_launch(dout, dout_ld, probs, static_cast<const __half*>(vn_f16), img, dscore, dscore_rowsum, N,
                                            B, P, C, G, STREAM);
}

int vqa_scale_by(float* x, int64_t n, const float* scalar, vqa_stream_t stream) {
  VQA_REQUIRE(x && scalar && n > 0, "vqa_scale_by: bad args");
  hipLaunchKernelGGL(scale_by_kernel, dim3(grid_for(n, 256)), dim3(256), 0, STREAM, x, n, scalar);
  return check_hip(hipGetLastError(), "scale_by launch");
}

int vqa_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
             float beta2, float eps, int step, float grad_scale, vqa_stream_t stream) {
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ADAM, (hipStream_t)stream);
  VQA_REQUIRE(param && grad && exp_avg && exp_avg_sq && n > 0 && step >= 1, "vqa_adam: bad args");
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  const float step_size = (float)((double)lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n, 256)), dim3(256), 0, STREAM, param, grad, exp_avg, exp_avg_sq, n,
                     step_size, beta1, beta2, eps, inv_sqrt_bc2, grad_scale);
  return check_hip(hipGetLastError(), "adam launch");
}

int vqa_adam_segments(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                      const vqa_adam_segment* segs, int n_segs, float grad_scale, vqa_stream_t stream) {
  VQA_REQUIRE(param && grad && exp_avg && exp_avg_sq && segs, "vqa_adam_segments: null pointer");
  VQA_REQUIRE(((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
                reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15) == 0,
              "vqa_adam_segments: param, grad, exp_avg and exp_avg_sq must be 16-byte aligned");
  VQA_REQUIRE(n >= 1 && n_segs >= 1 && n_segs <= VQA_ADAM_MAX_SEGMENTS, "vqa_adam_segments: n=%lld, n_segs=%d out of range (1..%d segments)",
              (long long)n, n_segs, VQA_ADAM_MAX_SEGMENTS);
  AdamSegTable tab;
  memset(&tab, 0, sizeof(tab));
  int64_t prev_end = 0;
  for (int i = 0; i < n_segs; ++i) {
    const vqa_adam_segment& s = segs[i];
    VQA_REQUIRE(s.begin % 4 == 0 && s.end % 4 == 0, "vqa_adam_segments: segment %d [%lld, %lld) is not aligned to 4 elements", i,
                (long long)s.begin, (long long)s.end);
    VQA_REQUIRE(s.begin >= 0 && s.begin < s.end && s.end <= n, "vqa_adam_segments: segment %d [%lld, %lld) out of range (n=%lld)", i,
                (long long)s.begin, (long long)s.end, (long long)n);
    VQA_REQUIRE(s.begin >= prev_end, "vqa_adam_segments: segment %d [%lld, %lld) overlaps or precedes segment %d (sorted, disjoint)",
                i, (long long)s.begin, (long long)s.end, i - 1);
    VQA_REQUIRE(s.step >= 1, "vqa_adam_segments: segment %d has step=%d (>= 1)", i, s.step);
    VQA_REQUIRE(s.weight_decay >= 0.f && (s.decoupled == 0 || s.decoupled == 1),
                "vqa_adam_segments: segment %d has weight_decay=%g, decoupled=%d", i, (double)s.weight_decay, s.decoupled);
    prev_end = s.end;
    const double bc1 = 1.0 - pow((double)s.beta1, s.step), bc2 = 1.0 - pow((double)s.beta2, s.step);
    AdamSeg& d = tab.s[i];
    d.q0 = s.begin / 4;
    d.q1 = s.end / 4;
    d.step_size = (float)((double)s.lr / bc1);
    d.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    d.beta1 = s.beta1; d.beta2 = s.beta2; d.eps = s.eps; d.wd = s.weight_decay;
    d.keep = (float)(1.0 - (double)s.lr * (double)s.weight_decay);
    d.mode = s.weight_decay == 0.f ? 0 : (s.decoupled ? 2 : 1);
  }
  set_launch_tag(-1);
  ProfScope prof(VQA_K_ADAM, (hipStream_t)stream);
  const int64_t quads = tab.s[n_segs - 1].q1 - tab.s[0].q0;
  hipLaunchKernelGGL(adam_segments_kernel, dim3(grid_for(quads, 256, VQA_ADAM_SEGMENTS_MAX_BLOCKS)), dim3(256), 0, STREAM, param, grad,
                     exp_avg, exp_avg_sq, tab, n_segs, grad_scale);
  return check_hip(hipGetLastError(), "adam_segments launch");
}

}  // extern "C"
