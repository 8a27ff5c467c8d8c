// Shared host/device helpers for the VQA HIP kernel library (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "../../include/vqa_hip.h"

namespace vqa {

// ---------------------------------------------------------------- errors (runtime.hip, as the launch plumbing, knobs and profiling hook)
void set_error(const char* fmt, ...);
int check_hip(hipError_t e, const char* what);

#define VQA_REQUIRE(cond, ...)                 \
  do {                                         \
    if (!(cond)) {                             \
      ::vqa::set_error(__VA_ARGS__);           \
      return VQA_ERR_INVALID;                  \
    }                                          \
  } while (0)

// ---------------------------------------------------------------- launch plumbing
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) for a kernel, once per (device, kernel); thread-safe.
int ensure_dyn_smem(const void* kernel, int bytes, const char* what);
template <class K>
static int set_smem(K kern, int bytes, const char* what) {
  return ensure_dyn_smem(reinterpret_cast<const void*>(kern), bytes, what);
}

struct KernelNames { const char *attr, *launch; };      // what ensure_dyn_smem / check_hip report
template <class K, class... A>
static int launch_kernel(K kern, KernelNames n, dim3 grid, int threads, int lds, hipStream_t s, A... args) {
  int rc = set_smem(kern, lds, n.attr);
  if (rc) return rc;
  hipLaunchKernelGGL(kern, grid, dim3(threads), lds, s, args...);
  return check_hip(hipGetLastError(), n.launch);
}

// Workgroups of a persistent kernel that are resident at once on the current device: min(planned, occupancy query) per CU x CUs,
// cached per (device, kernel).  <= 0: the query failed (vqa_last_error says why).
int persistent_slots(const void* kernel, int threads, int smem_bytes, int planned_per_cu);

// Blocks of a grid-stride launch over n items, per_block items a block: at least 1, at most cap.
static inline int grid_for(int64_t n, int per_block, int cap = 8192) {
  int64_t b = (n + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}

// runtime flag -> template flag: f is a generic lambda that reads decltype(flag)::value, so a tile choice is written once
template <bool V> struct Flag { static constexpr bool value = V; };
template <class F>
static int with_flag(bool v, F&& f) { return v ? f(Flag<true>{}) : f(Flag<false>{}); }
template <class F>
static int with_flags(bool a, bool b, F&& f) {
  return with_flag(a, [&](auto fa) { return with_flag(b, [&](auto fb) { return f(fa, fb); }); });
}
// the same for a run-time count in 1..4 (glimpses, 256-channel steps): f reads decltype(n)::value.  The caller has checked
// the range -- there is no error path in here, and a value outside it would run as 4.
template <class F>
static int with_int14(int v, F&& f) {
  switch (v) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

// The addresses of the arguments ORed together (host only): (ptr_bits(a, b, c) & 15) == 0 says that all of them are 16-byte
// aligned.  A null pointer contributes nothing, so an operand that is not there counts as aligned.
template <class... P>
static inline uintptr_t ptr_bits(const P*... p) { return (uintptr_t{0} | ... | reinterpret_cast<uintptr_t>(p)); }

// what a kept element is multiplied by under dropout p: 1 / (1 - p), 1 at p = 0
static inline float keep_scale(float p) { return p > 0.f ? 1.0f / (1.0f - p) : 1.0f; }

// VQA_* environment knobs (diagnostics / forced tile variants for the parity tests).  Read ONCE, when the
// library is first used; vqa_reload_knobs() re-reads them (tests that switch variants inside one process).
//   -1 = unset (the planner decides)
struct Knobs {
  int split_target;       // VQA_SPLIT_TARGET: resident-workgroup target of the split-K planner (default 512)
  int big_tiles;          // VQA_BIG_TILES 0/1/2/3
  int persistent;         // VQA_PERSISTENT 0/1
  int weight_stationary;  // VQA_WEIGHT_STATIONARY 0/1
  int wgrad_192;          // VQA_WGRAD_192 0/1
  int wgrad_384;          // VQA_WGRAD_384 0/1
  int conv_chunk;         // VQA_CONV_CHUNK: images per conv launch (tests)
  int tall_bm;            // VQA_TALL_BM: 128 = the tall bf16 GEMM on 128 x 128 tiles; anything else: 256 x 128
};
const Knobs& knobs();

// ---------------------------------------------------------------- profiling hook
// When a kernel id is armed (vqa_prof_arm), every launch of that kernel is bracketed by HIP
// events recorded on the launch stream; vqa_prof_read() returns count and total milliseconds.
void set_launch_tag(int tag);
struct ProfScope {
  int id;
  hipStream_t s;
  bool on;
  ProfScope(int id_, hipStream_t s_);
  ~ProfScope();
};

// ---------------------------------------------------------------- device helpers
__device__ __forceinline__ int xcd_swizzle(int bid, int nwg) {
  // Blocks are dealt round-robin over the 8 XCDs; give each XCD a contiguous range of logical
  // tile ids so neighbouring tiles (shared operand panels) meet in one L2.  Bijective for any nwg.
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}

// Counter-based dropout RNG: keep(seed, site, idx) is a pure function, so the backward pass
// regenerates the mask instead of storing it.
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
// One 32-bit hash serves a PAIR of elements (idx >> 1), 16 random bits each: keep iff the element's 16-bit field is at or
// above floor(p * 65536) -- the drop probability is p to within 2^-16.  The hash was the VALU bound of the attention-stage
// kernels in train mode (two multiply-xorshift rounds per element: att_score_fwd ran at 2 TB/s against 4 TB/s in eval
// mode); vector code takes four consecutive elements from drop_scale4 (two hashes).
__device__ __forceinline__ uint32_t drop_hash(uint64_t seed, uint64_t pair) {
  const uint32_t lo = (uint32_t)pair, hi = (uint32_t)(pair >> 32);
  uint32_t h = mix32(lo ^ (uint32_t)seed);
  return mix32(h + hi * 0x9E3779B9U + (uint32_t)(seed >> 32));
}
__device__ __forceinline__ float drop_scale(uint64_t seed, uint64_t idx, float p, float inv_keep) {
  // returns 0 (dropped) or 1/(1-p) (kept)
  const uint32_t h = drop_hash(seed, idx >> 1);
  const uint32_t u = (idx & 1) ? (h >> 16) : (h & 0xffffu);
  return u >= (uint32_t)(p * 65536.0f) ? inv_keep : 0.0f;
}
// scales of elements idx .. idx + 3, idx a multiple of 4
__device__ __forceinline__ float4 drop_scale4(uint64_t seed, uint64_t idx, float p, float inv_keep) {
  const uint32_t h0 = drop_hash(seed, idx >> 1), h1 = drop_hash(seed, (idx >> 1) + 1);
  const uint32_t thr = (uint32_t)(p * 65536.0f);
  return make_float4((h0 & 0xffffu) >= thr ? inv_keep : 0.f, (h0 >> 16) >= thr ? inv_keep : 0.f,
                     (h1 & 0xffffu) >= thr ? inv_keep : 0.f, (h1 >> 16) >= thr ? inv_keep : 0.f);
}

// The 2x2 max-pool window rule of the conv + ReLU + pool kernels (include/vqa_hip.h): of the window's four pre-activations
// in the order dy*2+dx the FIRST strict maximum wins (what nn.MaxPool2d returns on ties); the bias is added to the winner
// (max(z + b) == max(z) + b); where the result is <= 0 the output is 0 and the code byte 4 (dead: no pixel gets the gradient).
// Three sites spell the same rule out themselves because this helper moves their code: pconv_kernel (conv_patch_bf16.hip;
// <4, 0, false> goes from 216 to 217 VGPRs), convk_relu_pool_kernel (conv_generic.hip; 42 to 40) and the fp32 wide-store
// path of conv0_fwd_kernel (conv0.hip; same registers, but the schedule shifts: that kernel is kept instruction-identical).
struct PoolPick { float v; uint8_t code; };
__device__ __forceinline__ PoolPick pool_pick(float z0, float z1, float z2, float z3, float bias) {
  float best = z0;
  int a = 0;
  if (z1 > best) { best = z1; a = 1; }
  if (z2 > best) { best = z2; a = 2; }
  if (z3 > best) { best = z3; a = 3; }
  best += bias;
  return {best > 0.f ? best : 0.f, best > 0.f ? (uint8_t)a : (uint8_t)4};
}

__device__ __forceinline__ uint32_t f2bf16_pair(float lo, float hi) {      // round to nearest even (v_cvt_pk_bf16_f32)
  typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
  const bf2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, v);
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// the same over a workgroup of up to 16 waves; red: 16 floats of LDS
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

}  // namespace vqa
