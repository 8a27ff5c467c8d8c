// Occlusion maps from cached features (vqa_occl_logit): the logit of one answer column with a window of grid
// positions taken out of the image, for every position, from the attention weights answer() already has and U = W1_g . vn --
// the classifier's first layer applied to every feature row once per image.  One streaming kernel: U is read once per
// question (window x window times for a larger window, from the cache), everything else is small and lives in LDS.
#include "occl_core.hpp"

namespace vqa {

constexpr int OCCL_THREADS = 256;     // 4 waves
constexpr int OCCL_PPB = 16;          // positions per workgroup: 4 per wave, walked in order

// Workgroup = (question b, 16 consecutive positions).  The question's Z into LDS, then occl_head (occl_core.hpp): base, the
// W2 row and r[g]; dynamic LDS occl_lds(G + 2, hid).  Then one wave per position p: lane l owns the quads l, l + 64, ... of
// hid, adds its terms in that order, and the wave butterfly finishes the dot product with W2[a] -- one summation order per
// (b, p), whatever the grid.  A question whose row of U is not in [slot0, slot0 + R) is left alone (the
// caller walks U in chunks of images); an answer column outside [0, A) gives a row of zeros.
template <int G>
__global__ void __launch_bounds__(OCCL_THREADS)
occl_logit_kernel(const float* base, const float* Z, const float* U, const int* slot, int slot0, int R, const float* probs,
                  const float* score, const float* cnull, const float* W2, int64_t w2_ld, const float* b2, const int* answers,
                  const float* logits, int64_t logits_ld, float* maps, int nchunk, int gh, int gw, int hid, int A, int half) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int P = gh * gw;
  const int b = blockIdx.x / nchunk;
  const int p0 = (blockIdx.x - b * nchunk) * OCCL_PPB;
  const int row = occl_row(slot, b, slot0, R);
  if (row < 0) return;                                              // block-uniform
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = answers[b];
  if ((unsigned)a >= (unsigned)A) {
    if (tid < OCCL_PPB && p0 + tid < P) maps[(int64_t)b * P + p0 + tid] = 0.f;
    return;
  }
  float* s_base = sm;                       // [hid]
  float* s_z = sm + hid;                    // [G][hid]
  float* s_w2 = sm + (size_t)(G + 1) * hid; // [hid]
  float* red = sm + (size_t)(G + 2) * hid;  // [16]
  float* s_r = red + 16;                    // [G]
  const int nq = hid >> 2;
  for (int c = tid; c < G * nq; c += OCCL_THREADS)
    reinterpret_cast<float4*>(s_z)[c] = reinterpret_cast<const float4*>(Z + (int64_t)b * G * hid)[c];
  occl_head<G, OCCL_THREADS>(base, score, cnull, W2, w2_ld, b, a, P, hid, s_base, s_w2, red, s_r);
  const float logit = logits[(int64_t)b * logits_ld + a];
  const float bias = b2[a];
  const float* Ub = U + (int64_t)row * P * G * hid;
  const float* pb = probs + (int64_t)b * G * P;
  for (int k = wave; k < OCCL_PPB; k += OCCL_THREADS / 64) {
    const int p = p0 + k;
    if (p >= P) break;                                              // wave-uniform
    const int py = p / gw, px = p - py * gw;
    const int y0 = max(py - half, 0), y1 = min(py + half, gh - 1);
    const int x0 = max(px - half, 0), x1 = min(px + half, gw - 1);
    const float count = (float)((y1 - y0 + 1) * (x1 - x0 + 1));
    // mass and alpha: the window's positions row by row, the same on every lane
    float alpha[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float mass = 0.f;
      for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) mass += pb[g * P + y * gw + x];
      alpha[g] = 1.f / (1.f - mass + count * s_r[g]);
    }
    float dot = 0.f;
    for (int c = lane; c < nq; c += 64) {
      float4 acc[G];
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
          const int s = y * gw + x;
          const float4* us = reinterpret_cast<const float4*>(Ub + (int64_t)s * G * hid);
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const float w = pb[g * P + s];
            const float4 u = us[g * nq + c];
            acc[g].x += w * u.x; acc[g].y += w * u.y; acc[g].z += w * u.z; acc[g].w += w * u.w;
          }
        }
      float4 pre = reinterpret_cast<const float4*>(s_base)[c];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float4 z = reinterpret_cast<const float4*>(s_z)[g * nq + c];
        pre.x += alpha[g] * (z.x - acc[g].x); pre.y += alpha[g] * (z.y - acc[g].y);
        pre.z += alpha[g] * (z.z - acc[g].z); pre.w += alpha[g] * (z.w - acc[g].w);
      }
      const float4 w2 = reinterpret_cast<const float4*>(s_w2)[c];
      dot += w2.x * fmaxf(pre.x, 0.f) + w2.y * fmaxf(pre.y, 0.f) + w2.z * fmaxf(pre.z, 0.f) + w2.w * fmaxf(pre.w, 0.f);
    }
    dot = wave_sum(dot);
    if (lane == 0) maps[(int64_t)b * P + p] = logit - (dot + bias);
  }
}

}  // namespace vqa

using namespace vqa;

extern "C" {

int vqa_occl_logit(const float* base, const float* Z, const float* U, const int32_t* slot, int slot0, const float* probs,
                   const float* score, const float* cnull, const float* W2, int64_t w2_ld, const float* b2,
                   const int32_t* answers, const float* logits, int64_t logits_ld, float* maps, int R, int B, int gh, int gw,
                   int hid, int G, int A, int window, vqa_stream_t stream) {
  set_launch_tag(-1);
  const char* who = "vqa_occl_logit";
  VQA_REQUIRE(window >= 1 && window <= 7 && (window & 1), "%s: window=%d unsupported (odd, 1..7)", who, window);
  const bool pointers = base && Z && U && slot && probs && score && cnull && W2 && b2 && answers && logits && maps;
  if (const int rc = occl_check(who, G, pointers, hid, w2_ld, G + 2, "(G+2)", ptr_bits(base, Z, U, W2), "base, Z, U and W2",
                                R >= 1 && B >= 0 && gh >= 1 && gw >= 1 && (int64_t)gh * gw <= (1 << 20) && A >= 1 && logits_ld >= A,
                                "%s: R=%d, B=%d, grid %d x %d, A=%d, logits_ld=%lld out of range", R, B, gh, gw, A,
                                (long long)logits_ld))
    return rc;
  if (B == 0) return VQA_OK;
  const int P = gh * gw;
  const int nchunk = (P + OCCL_PPB - 1) / OCCL_PPB;
  VQA_REQUIRE((int64_t)B * nchunk < (1LL << 31), "%s: B=%d x %d position chunks exceed the grid", who, B, nchunk);
  return with_int14(G, [&](auto g) {
    // the attribute is set once per kernel, so for the largest LDS size the check above admits
    const int rc = set_smem(occl_logit_kernel<decltype(g)::value>, 64 * 1024, "attr(occl_logit)");
    if (rc) return rc;
    hipLaunchKernelGGL(occl_logit_kernel<decltype(g)::value>, dim3(B * nchunk), dim3(OCCL_THREADS), occl_lds(G + 2, hid),
                       (hipStream_t)stream, base, Z, U, slot, slot0, R, probs, score, cnull, W2, w2_ld, b2, answers, logits,
                       logits_ld, maps, nchunk, gh, gw, hid, A, window / 2);
    return check_hip(hipGetLastError(), "occl_logit launch");
  });
}

}  // extern "C"
