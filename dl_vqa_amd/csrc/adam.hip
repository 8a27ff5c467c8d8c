// The optimizer's streaming kernels: Adam over one tensor, Adam over a table of segments of a flat buffer (FusedAdam's
// parameter groups), and the in-place scale of a tensor by a device scalar.
#include <math.h>
#include "common.hpp"

namespace vqa {

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

extern "C" {

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
  VQA_REQUIRE((ptr_bits(param, grad, exp_avg, exp_avg_sq) & 15) == 0,
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
