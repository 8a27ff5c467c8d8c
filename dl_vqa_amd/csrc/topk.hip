// The k best answers of every logits row with their softmax probabilities, in ONE launch (vqa_softmax_topk; VqaNet.predict,
// dl_vqa_amd.topk_answers).  The order is the score kernel's: larger value first, equal values by smaller column
// (softce_kernel, elementwise.hip: `ov > mx || (ov == mx && oi < am)`), so idx[b][0] is the arg-max the VQA score is taken at.
//
// One wave per row, four rows per workgroup; lane l owns the columns l + 64*j.  A value becomes an ordered 32-bit key
// (-0.0 canonicalised to +0.0, NaN sent to the top key, 0 = no such column), and key and column together one 64-bit word
//   K = key << 32 | (0x7fffffff - column)
// whose unsigned order IS the total order: a selection round takes the largest K strictly below the previous pick -- per
// lane over its columns, then the wave butterfly -- so k rounds list the first k columns and no pick is ever marked or
// written back.  Pass 1 finds the row maximum and the sum of exponentials: per lane four partial sums over j = 0, 1, 2, 3
// (mod 4) in ascending j, joined as (s0 + s1) + (s2 + s3), then the wave butterfly (every lane adds the same pairs, so all
// 64 hold the same bits): one fixed order, no atomics.
// NJ > 0: the row (up to 64*NJ columns) lives in NJ key registers per lane, every loop fully unrolled (static indices:
// nothing lands in scratch); NJ == 0: any A, the row is read again through the cache in every round.
// vqa_softmax_pick (probability curves) is the same row code with k = 1 and a tail that also gives the
// probability of one GIVEN column per row from the row's own maximum and sum: softmax_topk_row is written once, each kernel
// hands it what to do with (row, x, max, sum) at the end.
#include "common.hpp"

namespace vqa {

__device__ __forceinline__ uint32_t topk_key(float x) {
  uint32_t u = __float_as_uint(x);
  if (x != x) return 0xffffffffu;                      // NaN (either sign) ranks above +inf, as torch.topk has it
  if (u == 0x80000000u) u = 0u;                        // -0.0 == +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // -inf -> 0x007fffff .. +inf -> 0xff800000: never 0
}
__device__ __forceinline__ float topk_value(uint32_t key) {   // the inverse (NaN -> a NaN, -0.0 -> +0.0)
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// One wave's row.  tail(row, x, mx, sum, lane): what the kernel adds once max and sum are known (every lane holds both).
template <int NJ, class Tail>
__device__ __forceinline__ void softmax_topk_row(const float* logits, int64_t ld, int B, int A, int k, int32_t* idx, float* prob,
                                                 float* lse, Tail tail) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;                                // wave-uniform; the kernel has no workgroup barrier
  const float* x = logits + row * ld;
  const int nj = NJ > 0 ? NJ : (A - 1) / 64 + 1;
  uint32_t keys[NJ > 0 ? NJ : 1];
  if (NJ > 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const unsigned c = (unsigned)lane + 64u * j;
      keys[j] = c < (unsigned)A ? topk_key(x[c]) : 0u;
    }
  }
  // key of this lane's j-th column; 0 past the end of the row
  auto key_at = [&](int j) -> uint32_t {
    if (NJ > 0) return keys[j];
    const unsigned c = (unsigned)lane + 64u * j;
    return c < (unsigned)A ? topk_key(x[c]) : 0u;
  };

  // ---- pass 1: row maximum, then the sum of exponentials
  uint32_t kmax = 0u;
#pragma unroll
  for (int j = 0; j < nj; ++j) { const uint32_t kj = key_at(j); kmax = kj > kmax ? kj : kmax; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const uint32_t ok = __shfl_xor(kmax, o, 64); kmax = ok > kmax ? ok : kmax; }
  const float mx = topk_value(kmax);                   // NaN if the row holds one: every exponential below is NaN then
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (NJ > 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const uint32_t kj = keys[j];
      if (kj) s[j & 3] += expf(topk_value(kj) - mx);
    }
  } else {
    for (int j = 0; j < nj; j += 4) {                  // j + u may pass nj: key_at is 0 there
#pragma unroll
      for (int u = 0; u < 4; ++u) { const uint32_t kj = key_at(j + u); if (kj) s[u] += expf(topk_value(kj) - mx); }
    }
  }
  const float sum = wave_sum((s[0] + s[1]) + (s[2] + s[3]));

  // ---- pass 2: k selection rounds; lane r keeps the pick of round r
  const uint32_t low0 = 0x7fffffffu - (uint32_t)lane;  // low word of K at j = 0; 64 less per j
  uint64_t prev = ~0ull;                               // above every K
  uint64_t mine = 0ull;
  for (int r = 0; r < k; ++r) {
    uint64_t best = 0ull;
#pragma unroll
    for (int j = 0; j < nj; ++j) {
      const uint64_t K = ((uint64_t)key_at(j) << 32) | (uint64_t)(low0 - 64u * (uint32_t)j);
      if (K < prev && K > best) best = K;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t ob = __shfl_xor((unsigned long long)best, o, 64);
      best = ob > best ? ob : best;
    }
    if (lane == r) mine = best;
    prev = best;
  }
  if (lane < k) {                                      // k <= A: every round found a column, key != 0
    const int64_t o = row * k + lane;
    idx[o] = (int32_t)(0x7fffffffu - (uint32_t)mine);
    prob[o] = expf(topk_value((uint32_t)(mine >> 32)) - mx) / sum;
  }
  if (lse && lane == 0) lse[row] = mx + logf(sum);
  tail(row, x, mx, sum, lane);
}

template <int NJ>
__global__ __launch_bounds__(256) void softmax_topk_kernel(const float* logits, int64_t ld, int B, int A, int k, int32_t* idx,
                                                           float* prob, float* lse) {
  softmax_topk_row<NJ>(logits, ld, B, A, k, idx, prob, lse, [](int64_t, const float*, float, float, int) {});
}

// vqa_softmax_pick: k = 1 into top / top_prob, and prob_at[row] = exp(x[a] - max) / sum for the column a = answers[row / rpq]
// -- top_prob's own expression, so a row whose given column is its arg-max holds the same bits twice -- or +0.0 for a column
// outside [0, A).  x[a] is one more 4-byte load of a row the wave has just read.
template <int NJ>
__global__ __launch_bounds__(256) void softmax_pick_kernel(const float* logits, int64_t ld, int B, int A, const int32_t* answers,
                                                           int rpq, int32_t* top, float* top_prob, float* prob_at) {
  softmax_topk_row<NJ>(logits, ld, B, A, 1, top, top_prob, nullptr,
                       [=](int64_t row, const float* x, float mx, float sum, int lane) {
                         if (lane != 0) return;
                         const int a = answers[row / rpq];
                         prob_at[row] = (unsigned)a < (unsigned)A ? expf(x[a] - mx) / sum : 0.f;
                       });
}

// NJ of a row of A columns, as a compile-time constant handed to f: the ladder both entry points launch by
template <class F>
static void with_topk_nj(int A, F&& f) {
  if (A <= 64) f(std::integral_constant<int, 1>{});
  else if (A <= 256) f(std::integral_constant<int, 4>{});
  else if (A <= 1024) f(std::integral_constant<int, 16>{});
  else if (A <= 3072) f(std::integral_constant<int, 48>{});
  else f(std::integral_constant<int, 0>{});
}

}  // namespace vqa

using namespace vqa;

extern "C" {

int vqa_softmax_topk(const float* logits, int64_t ld, int B, int A, int k, int32_t* idx, float* prob, float* lse,
                     vqa_stream_t stream) {
  VQA_REQUIRE(B >= 0 && A >= 1 && ld >= (int64_t)A, "vqa_softmax_topk: B=%d, A=%d, ld=%lld out of range (B >= 0, A >= 1, ld >= A)", B,
              A, (long long)ld);
  VQA_REQUIRE(k >= 1 && k <= 64 && k <= A, "vqa_softmax_topk: k=%d out of range (1 <= k <= min(64, A), A=%d)", k, A);
  if (B == 0) return VQA_OK;
  VQA_REQUIRE(logits && idx && prob, "vqa_softmax_topk: null pointer (logits, idx and prob are required; lse is optional)");
  const dim3 grid((unsigned)(((int64_t)B + 3) / 4));
  hipStream_t s = (hipStream_t)stream;
  with_topk_nj(A, [&](auto nj) {
    hipLaunchKernelGGL(softmax_topk_kernel<decltype(nj)::value>, grid, dim3(256), 0, s, logits, ld, B, A, k, idx, prob, lse);
  });
  return check_hip(hipGetLastError(), "softmax_topk launch");
}

int vqa_softmax_pick(const float* logits, int64_t ld, int rows, int A, const int32_t* answers, int rows_per_question, int32_t* top,
                     float* top_prob, float* prob_at, vqa_stream_t stream) {
  VQA_REQUIRE(rows >= 0 && A >= 1 && ld >= (int64_t)A, "vqa_softmax_pick: rows=%d, A=%d, ld=%lld out of range (rows >= 0, A >= 1, ld >= A)",
              rows, A, (long long)ld);
  VQA_REQUIRE(rows_per_question >= 1 && rows % rows_per_question == 0,
              "vqa_softmax_pick: rows_per_question=%d must be >= 1 and divide rows=%d", rows_per_question, rows);
  if (rows == 0) return VQA_OK;
  VQA_REQUIRE(logits && answers && top && top_prob && prob_at, "vqa_softmax_pick: null pointer");
  const dim3 grid((unsigned)(((int64_t)rows + 3) / 4));
  hipStream_t s = (hipStream_t)stream;
  with_topk_nj(A, [&](auto nj) {
    hipLaunchKernelGGL(softmax_pick_kernel<decltype(nj)::value>, grid, dim3(256), 0, s, logits, ld, rows, A, answers,
                       rows_per_question, top, top_prob, prob_at);
  });
  return check_hip(hipGetLastError(), "softmax_pick launch");
}

}  // extern "C"
