// Exact word occlusion from cached features (VqaNet.explain_words_occlusion): the fall of one logit per
// question when the embedding output of ONE token slot is replaced by the zero vector, for every slot.  A variant is a pair
// (b, t), t < q_len[b].  Zeroing slot t leaves the forward direction's state before t and the reverse direction's state
// after t as the base question's encoder run left them, so a variant's chain starts from a saved base state and runs the
// remaining steps only.  Two streaming kernels:
//   vqa_lstm_occl_cell_fwd   one recurrence step of a set of variant rows (the recurrent product h_var . W_hh^T is vqa_gemm's);
//   vqa_occl_words           the tail: one column of lin2 per variant row, and the zeros of the slots past a question's end.
// Neither needs LDS or atomics; every row's result depends on that row alone.
#include "common.hpp"

namespace vqa {

// One element of the cell: vqa_lstm_cell_fwd's formulas with its device functions (sigmoidf_ of common.hpp, tanhf), gate
// order i, f, g, o.  Nothing is contracted across a product and a sum, so the 16-byte and the scalar form of the kernel
// below give the same bits.
__device__ __forceinline__ void occl_cell_elem(float pi, float pf, float pg, float po, float cp, float& cn, float& hn) {
#pragma clang fp contract(off)
  const float gi = sigmoidf_(pi), gf = sigmoidf_(pf), gg = tanhf(pg), go = sigmoidf_(po);
  const float a = gf * cp, b = gi * gg;
  cn = a + b;
  hn = go * tanhf(cn);
}

// VEC: a thread owns the quad (row r, units 4*c .. 4*c + 3), !VEC: one unit.  Rows and columns by a grid stride.
template <bool VEC>
__global__ __launch_bounds__(256) void lstm_occl_cell_kernel(const float* xg_base, const float* xg0, const float* hg, float* h_var,
                                                             float* c_var, int64_t st_ld, const int64_t* q_len,
                                                             const int32_t* var_b, const int32_t* var_t, int s, float* c_final,
                                                             int64_t cf_ld, const int32_t* cf_row, int n, int B, int T, int H) {
  constexpr int W = VEC ? 4 : 1;
  const int per = H / W;                                        // VEC: H % 4 == 0
  const int64_t total = (int64_t)n * per;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / per), j = (int)(i - (int64_t)r * per) * W;
    const int b = var_b[r], t = var_t[r];
    if ((unsigned)b >= (unsigned)B || (unsigned)t >= (unsigned)T) continue;       // not a variant: the row is left alone
    if ((int64_t)s >= q_len[b]) continue;                                         // past the question's end: the state is held
    const float* xr = (s == t) ? xg0 : xg_base + ((int64_t)s * B + b) * 4 * H;
    const float* hr = hg + (int64_t)r * 4 * H;
    float* cr = c_var + (int64_t)r * st_ld;
    float* hs = h_var + (int64_t)r * st_ld;
    float* cf = c_final ? c_final + (int64_t)(cf_row ? cf_row[r] : r) * cf_ld : nullptr;
    if (VEC) {
      float4 x[4], g[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        x[k] = *reinterpret_cast<const float4*>(xr + k * H + j);
        g[k] = *reinterpret_cast<const float4*>(hr + k * H + j);
      }
      const float4 cp = *reinterpret_cast<const float4*>(cr + j);
      float4 cn, hn;
      occl_cell_elem(x[0].x + g[0].x, x[1].x + g[1].x, x[2].x + g[2].x, x[3].x + g[3].x, cp.x, cn.x, hn.x);
      occl_cell_elem(x[0].y + g[0].y, x[1].y + g[1].y, x[2].y + g[2].y, x[3].y + g[3].y, cp.y, cn.y, hn.y);
      occl_cell_elem(x[0].z + g[0].z, x[1].z + g[1].z, x[2].z + g[2].z, x[3].z + g[3].z, cp.z, cn.z, hn.z);
      occl_cell_elem(x[0].w + g[0].w, x[1].w + g[1].w, x[2].w + g[2].w, x[3].w + g[3].w, cp.w, cn.w, hn.w);
      *reinterpret_cast<float4*>(cr + j) = cn;
      *reinterpret_cast<float4*>(hs + j) = hn;
      if (cf) *reinterpret_cast<float4*>(cf + j) = cn;
    } else {
      float cn, hn;
      occl_cell_elem(xr[j] + hr[j], xr[H + j] + hr[H + j], xr[2 * H + j] + hr[2 * H + j], xr[3 * H + j] + hr[3 * H + j], cr[j],
                     cn, hn);
      cr[j] = cn;
      hs[j] = hn;
      if (cf) cf[j] = cn;
    }
  }
}

// One term of the tail's dot product, rounded before it is added (vqa_embed_attr's rule).
__device__ __forceinline__ float occl_words_add(float acc, float w, float h) {
#pragma clang fp contract(off)
  const float term = w * h;
  return acc + term;
}

constexpr int OW_THREADS = 256;       // 4 waves: 4 variant rows, or 256 slots of the zero fill, per workgroup

// Workgroups [0, row_blocks): one wave per variant row r = (b, t): lane l adds the terms of the quads l + 64*i of hid in
// ascending i and, inside a quad, k = 0..3, then the wave butterfly -- one order per row, whatever the grid.  VEC reads the
// quads as 16-byte loads, !VEC the same elements one by one (the last quad ragged when hid % 4 != 0).  The workgroups
// behind them walk the slots of the questions [b0, b0 + nb) and write +0.0 where t >= q_len[b]: the two sets are
// disjoint (a variant has t < q_len[b]), so every element of those rows is written exactly once.
template <bool VEC>
__global__ __launch_bounds__(OW_THREADS) void occl_words_kernel(const float* h1, int64_t h1_ld, const float* W2, int64_t w2_ld,
                                                                const float* b2, const int32_t* answers, const float* logits,
                                                                int64_t logits_ld, const int32_t* var_b, const int32_t* var_t,
                                                                const int64_t* q_len, float* words, int n, int row_blocks, int b0,
                                                                int nb, int T, int hid, int A) {
  if ((int)blockIdx.x >= row_blocks) {
    const int64_t total = (int64_t)nb * T;
    const int64_t stride = (int64_t)(gridDim.x - row_blocks) * OW_THREADS;
    for (int64_t i = (int64_t)(blockIdx.x - row_blocks) * OW_THREADS + threadIdx.x; i < total; i += stride) {
      const int b = b0 + (int)(i / T), t = (int)(i % T);
      if ((int64_t)t >= q_len[b]) words[(int64_t)b * T + t] = 0.f;
    }
    return;
  }
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (OW_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= n) return;                                                       // wave-uniform from here on
  const int b = var_b[r], t = var_t[r];
  if (b < b0 || b >= b0 + nb || (unsigned)t >= (unsigned)T || (int64_t)t >= q_len[b]) return;      // not a variant of these rows
  const int a = answers[b];
  float out = 0.f;
  if ((unsigned)a < (unsigned)A) {
    const float* hr = h1 + (int64_t)r * h1_ld;
    const float* wr = W2 + (int64_t)a * w2_ld;
    const int nq = (hid + 3) >> 2;
    float acc = 0.f;
    for (int c = lane; c < nq; c += 64) {
      if (VEC) {
        const float4 w4 = reinterpret_cast<const float4*>(wr)[c], h4 = reinterpret_cast<const float4*>(hr)[c];
        acc = occl_words_add(acc, w4.x, h4.x);
        acc = occl_words_add(acc, w4.y, h4.y);
        acc = occl_words_add(acc, w4.z, h4.z);
        acc = occl_words_add(acc, w4.w, h4.w);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = 4 * c + k;
          if (i < hid) acc = occl_words_add(acc, wr[i], hr[i]);
        }
      }
    }
    acc = wave_sum(acc);
    out = logits[(int64_t)b * logits_ld + a] - (acc + b2[a]);
  }
  if (lane == 0) words[(int64_t)b * T + t] = out;
}

}  // namespace vqa

using namespace vqa;

extern "C" {

int vqa_lstm_occl_cell_fwd(const float* xg_base, const float* xg0, const float* hg, float* h_var, float* c_var, int64_t st_ld,
                           const int64_t* q_len, const int32_t* var_b, const int32_t* var_t, int s, float* c_final, int64_t cf_ld,
                           const int32_t* cf_row, int n, int B, int T, int H, vqa_stream_t stream) {
  const char* who = "vqa_lstm_occl_cell_fwd";
  VQA_REQUIRE(xg_base && xg0 && hg && h_var && c_var && q_len && var_b && var_t, "%s: null pointer", who);
  VQA_REQUIRE(n >= 0 && B >= 1 && T >= 1 && H >= 1 && s >= 0 && s < T, "%s: n=%d, B=%d, T=%d, H=%d, s=%d out of range", who, n, B,
              T, H, s);
  VQA_REQUIRE(st_ld >= H, "%s: row stride %lld below H=%d", who, (long long)st_ld, H);
  VQA_REQUIRE(!c_final || cf_ld >= H, "%s: c_final leading dimension %lld below H=%d", who, (long long)cf_ld, H);
  VQA_REQUIRE(c_final || !cf_row, "%s: cf_row without c_final", who);
  if (n == 0) return VQA_OK;
  const bool vec = H % 4 == 0 && st_ld % 4 == 0 && (!c_final || cf_ld % 4 == 0) &&
                   (ptr_bits(xg_base, xg0, hg, h_var, c_var, c_final) & 15) == 0;
  const int64_t items = (int64_t)n * (vec ? H / 4 : H);
  with_flag(vec, [&](auto v) {
    hipLaunchKernelGGL((lstm_occl_cell_kernel<decltype(v)::value>), dim3(grid_for(items, 256)), dim3(256), 0, (hipStream_t)stream,
                       xg_base, xg0, hg, h_var, c_var, st_ld, q_len, var_b, var_t, s, c_final, cf_ld, cf_row, n, B, T, H);
    return 0;
  });
  return check_hip(hipGetLastError(), "lstm_occl_cell_fwd launch");
}

int vqa_occl_words(const float* h1, int64_t h1_ld, const float* W2, int64_t w2_ld, const float* b2, const int32_t* answers,
                   const float* logits, int64_t logits_ld, const int32_t* var_b, const int32_t* var_t, const int64_t* q_len,
                   float* words, int n, int b0, int nb, int T, int hid, int A, vqa_stream_t stream) {
  const char* who = "vqa_occl_words";
  VQA_REQUIRE(W2 && b2 && answers && logits && q_len && words, "%s: null pointer", who);
  VQA_REQUIRE(n == 0 || (h1 && var_b && var_t), "%s: null pointer", who);
  VQA_REQUIRE(n >= 0 && b0 >= 0 && nb >= 0 && T >= 1 && hid >= 1 && A >= 1, "%s: n=%d, b0=%d, nb=%d, T=%d, hid=%d, A=%d out of range",
              who, n, b0, nb, T, hid, A);
  VQA_REQUIRE((int64_t)n <= (int64_t)nb * T, "%s: %d variant rows for %d questions of %d slots", who, n, nb, T);
  VQA_REQUIRE(h1_ld >= hid && w2_ld >= hid && logits_ld >= A, "%s: h1_ld=%lld, w2_ld=%lld (hid=%d), logits_ld=%lld (A=%d) out of range",
              who, (long long)h1_ld, (long long)w2_ld, hid, (long long)logits_ld, A);
  if (nb == 0) return VQA_OK;
  const bool vec = hid % 4 == 0 && h1_ld % 4 == 0 && w2_ld % 4 == 0 && (ptr_bits(h1, W2) & 15) == 0;
  const int row_blocks = (n + OW_THREADS / 64 - 1) / (OW_THREADS / 64);
  const int fill_blocks = grid_for((int64_t)nb * T, OW_THREADS, 1024);
  with_flag(vec, [&](auto v) {
    hipLaunchKernelGGL((occl_words_kernel<decltype(v)::value>), dim3(row_blocks + fill_blocks), dim3(OW_THREADS), 0,
                       (hipStream_t)stream, h1, h1_ld, W2, w2_ld, b2, answers, logits, logits_ld, var_b, var_t, q_len, words, n,
                       row_blocks, b0, nb, T, hid, A);
    return 0;
  });
  return check_hip(hipGetLastError(), "occl_words launch");
}

}  // extern "C"
