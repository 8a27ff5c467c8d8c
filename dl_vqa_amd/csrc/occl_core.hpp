// What the occlusion maps (occlusion.hip) and the deletion / insertion curves (faithfulness.hip, 4.20) share:
// the head of the closed form, the row-window test of the chunked-U protocol and the operand checks of the two entry points.
#pragma once
#include "common.hpp"

namespace vqa {

// The caller walks U in chunks of images, R rows from slot0 at a time: the row of U of question b in this window, or -1 for
// a question whose image is not in it (every kernel of the call leaves such a question alone).
__device__ __forceinline__ int occl_row(const int* slot, int b, int slot0, int R) {
  const int row = slot[b] - slot0;
  return (unsigned)row < (unsigned)R ? row : -1;
}

// dynamic LDS of a kernel that runs the head: `rows` rows of hid floats, 16 reduction slots and r [G] (4 floats kept for it)
static size_t occl_lds(int rows, int hid) { return ((size_t)rows * hid + 16 + 4) * 4; }

// The head, by a workgroup of THREADS threads for question b and answer column a: base[b] and W2[a] into s_base / s_w2 [hid],
//   s_r[g] = exp(cnull[b][g] - m) / sum_p exp(score[b][g][p] - m),  m = max_p score[b][g][p]
// by the block reduction (red [16]) that every workgroup of b runs in the same order -- maps and curves agree on r because
// both get it here.  Ends with the barrier after which these, and what the caller staged into LDS before, are readable.
// WITH_W2 == false (the hidden-row walk of faithfulness.hip, which explains no column): W2, a and s_w2 are not looked at.
template <int G, int THREADS, bool WITH_W2 = true>
__device__ __forceinline__ void occl_head(const float* base, const float* score, const float* cnull, const float* W2, int64_t w2_ld,
                                          int b, int a, int P, int hid, float* s_base, float* s_w2, float* red, float* s_r) {
  const int tid = threadIdx.x;
  for (int c = tid; c < (hid >> 2); c += THREADS) {
    reinterpret_cast<float4*>(s_base)[c] = reinterpret_cast<const float4*>(base + (int64_t)b * hid)[c];
    if constexpr (WITH_W2) reinterpret_cast<float4*>(s_w2)[c] = reinterpret_cast<const float4*>(W2 + (int64_t)a * w2_ld)[c];
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float* s = score + ((int64_t)b * G + g) * P;
    float mx = -INFINITY;
    for (int i = tid; i < P; i += THREADS) mx = fmaxf(mx, s[i]);
    mx = block_reduce(mx, red, true);
    float sum = 0.f;
    for (int i = tid; i < P; i += THREADS) sum += expf(s[i] - mx);
    sum = block_reduce(sum, red, false);
    if (tid == 0) s_r[g] = expf(cnull[b * G + g] - mx) / sum;
  }
  __syncthreads();
}

// What vqa_occl_logit and vqa_occl_curves check alike, before any HIP call (`who` names the caller), and where they differ:
// pointers -- its data pointers are all there; lds_rows and its text -- occl_lds of its kernel; quads / quad_names -- ptr_bits
// of what its kernels read as float4; in_range, range_fmt (takes `who` first), range... -- its own ranges of R, B, A, the grid.
template <class... Range>
static int occl_check(const char* who, int G, bool pointers, int hid, int64_t w2_ld, int lds_rows, const char* lds_rows_text,
                      uintptr_t quads, const char* quad_names, bool in_range, const char* range_fmt, Range... range) {
  VQA_REQUIRE(G >= 1 && G <= 4, "%s: glimpses=%d unsupported (1..4)", who, G);
  VQA_REQUIRE(pointers, "%s: null pointer", who);
  VQA_REQUIRE(hid >= 4 && hid % 4 == 0 && w2_ld % 4 == 0 && w2_ld >= hid, "%s: hid=%d (a multiple of 4), w2_ld=%lld out of range",
              who, hid, (long long)w2_ld);
  VQA_REQUIRE(in_range, range_fmt, who, range...);
  VQA_REQUIRE(occl_lds(lds_rows, hid) <= 64 * 1024, "%s: %s*hid=%d too large for LDS", who, lds_rows_text, lds_rows * hid);
  VQA_REQUIRE((quads & 15) == 0, "%s: %s must be 16-byte aligned", who, quad_names);
  return VQA_OK;
}

}  // namespace vqa
