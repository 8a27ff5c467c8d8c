// Memory-bound stages of the VQA hot path: dropout, L2-norm, embedding+tanh, LSTM cell, soft-target cross entropy,
// reductions.  (The attention softmax / weighted sum: att_apply.hip; row gathers and fp16 converters: gather.hip; Adam: adam.hip.)
// All are HBM-bound streaming kernels: 16-byte per-lane accesses, wave64 shuffles for reductions.
#include "common.hpp"

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

// Gradient x input per token slot (vqa_embed_attr; eval mode, no dropout): with e = emb[q[b][t]] the
// embedding output before tanh, x = tanh(e) as the forward wrote it and dx = dx0 (+ dx1) the gradient of one logit at x,
//   words[b][t] = sum_e emb[q[b][t]][e] * (1 - x[t][b][e]^2) * dx[t*B + b][e]
// -- embed_tanh_bwd's element without the sum over the slots that share a token.  One wave per slot, slots walked by a
// grid stride.  The summation order is a property of the slot, not of the grid: lane l adds the terms of its elements
// 4*(l + 64*i) + k in ascending i and, inside a quad, k = 0, 1, 2, 3, each term rounded before it is added (no fused
// multiply-add across the term and the sum); then the wave butterfly.  VEC reads the four operands' quads as 16-byte
// loads, !VEC the same elements one by one: the same values in the same order, hence the same bits.  Every words[b][t] is
// written: +0.0 for t >= q_len[b] and for a token id outside [0, V) (counted by the forward, a zero row there and here).
__device__ __forceinline__ float embed_attr_add(float acc, float e, float x, float d) {
#pragma clang fp contract(off)
  const float g = 1.f - x * x;
  const float term = e * g * d;
  return acc + term;
}

template <bool VEC>
__global__ __launch_bounds__(256) void embed_attr_kernel(const int64_t* q, const float* emb, const float* x, const float* dx0,
                                                         const float* dx1, const int64_t* q_len, float* words, int B, int T,
                                                         int E, int V) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int nq = (E + 3) >> 2;                              // quads, the last one ragged when E % 4 != 0 (!VEC only)
  for (int64_t s = wave; s < (int64_t)B * T; s += nwaves) {
    const int b = (int)(s / T), t = (int)(s - (int64_t)b * T);
    const int64_t tok = q[s];
    float acc = 0.f;
    if ((int64_t)t < q_len[b] && tok >= 0 && tok < V) {     // wave-uniform
      const float* er = emb + tok * E;
      const int64_t row = ((int64_t)t * B + b) * E;
      const float *xr = x + row, *d0 = dx0 + row, *d1 = dx1 ? dx1 + row : nullptr;
      for (int c = lane; c < nq; c += 64) {
        if (VEC) {
          const float4 e4 = reinterpret_cast<const float4*>(er)[c], x4 = reinterpret_cast<const float4*>(xr)[c];
          float4 d4 = reinterpret_cast<const float4*>(d0)[c];
          if (d1) {
            const float4 o = reinterpret_cast<const float4*>(d1)[c];
            d4.x += o.x; d4.y += o.y; d4.z += o.z; d4.w += o.w;
          }
          acc = embed_attr_add(acc, e4.x, x4.x, d4.x);
          acc = embed_attr_add(acc, e4.y, x4.y, d4.y);
          acc = embed_attr_add(acc, e4.z, x4.z, d4.z);
          acc = embed_attr_add(acc, e4.w, x4.w, d4.w);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int i = 4 * c + k;
            if (i < E) acc = embed_attr_add(acc, er[i], xr[i], d1 ? d0[i] + d1[i] : d0[i]);
          }
        }
      }
      acc = wave_sum(acc);
    }
    if (lane == 0) words[s] = acc;
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
  VQA_REQUIRE((ptr_bits(x, y) & 15) == 0, "vqa_dropout_add: pointers must be 16-byte aligned");
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

int vqa_embed_attr(const int64_t* q, const float* emb, const float* x, const float* dx0, const float* dx1,
                   const int64_t* q_len, float* words, int B, int T, int E, int V, vqa_stream_t stream) {
  VQA_REQUIRE(q && emb && x && dx0 && q_len && words, "vqa_embed_attr: null pointer");
  VQA_REQUIRE(B >= 0 && T >= 1 && E >= 1 && V >= 1, "vqa_embed_attr: B=%d, T=%d, E=%d, V=%d out of range", B, T, E, V);
  if (B == 0) return VQA_OK;
  const dim3 grid(grid_for((int64_t)B * T, 4));             // four waves, four slots per workgroup
  with_flag(E % 4 == 0 && (ptr_bits(emb, x, dx0, dx1) & 15) == 0, [&](auto vec) {
    hipLaunchKernelGGL((embed_attr_kernel<decltype(vec)::value>), grid, dim3(256), 0, STREAM, q, emb, x, dx0, dx1, q_len, words,
                       B, T, E, V);
    return 0;
  });
  return check_hip(hipGetLastError(), "embed_attr launch");
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

}  // extern "C"
