// Loads of an image-feature cache operand (vn, v') by the kernels that read one: the element type is fp32 or IEEE half
// (a float16 cache).  A half is widened on load, which is exact, so everything behind the load computes in
// fp32 on the same values, in the same order, as on an fp32 cache that holds them.  The fp32 overloads are the expressions
// the kernels had before they were templated on the element type: their instantiations compile to the code they were.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

namespace vqa {

// quad c of the row that starts at p (elements 4*c .. 4*c + 3) as a float4: one 16-byte load of fp32 (p 16-byte aligned), one
// 8-byte load of fp16 (p 8-byte aligned)
// That alignment, host side: a launcher takes its quad kernel for a pointer with (address & (kQuadAlign<VT> - 1)) == 0, and
// an entry point whose kernel has no scalar form requires it.
template <class VT>
constexpr uintptr_t kQuadAlign = 4 * sizeof(VT);
template <class I>
__device__ __forceinline__ float4 load_quad(const float* p, I c) { return reinterpret_cast<const float4*>(p)[c]; }
template <class I>
__device__ __forceinline__ float4 load_quad(const __half* p, I c) {
  const uint2 raw = reinterpret_cast<const uint2*>(p)[c];
  const __half2* h = reinterpret_cast<const __half2*>(&raw);
  const float2 a = __half22float2(h[0]), b = __half22float2(h[1]);
  return make_float4(a.x, a.y, b.x, b.y);
}

// element i of the row that starts at p
template <class I>
__device__ __forceinline__ float load_one(const float* p, I i) { return p[i]; }
template <class I>
__device__ __forceinline__ float load_one(const __half* p, I i) { return __half2float(p[i]); }

}  // namespace vqa
