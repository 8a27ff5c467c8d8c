// Deletion and insertion curves of an attribution map from cached features (vqa_rank_desc, vqa_occl_curves):
// the logit of one answer column with only the first k positions of a ranking present (insertion) and with the first k absent
// (deletion), k = 0 .. P, in the kept form of the closed form of csrc/occlusion.hip -- sums over the positions that REMAIN, so
// nothing is ever subtracted.  The ranking is cut into chunks of CURVE_L steps: one pass sums each chunk's probs * U rows, a
// small pass turns the chunk sums into exclusive prefixes (insertion) and suffixes (deletion), and the walk gives one wave per
// (question, chunk), which steps through its rows from its prefix forward and from its suffix backward.
#include "occl_core.hpp"

namespace vqa {

constexpr int RANK_THREADS = 256;
constexpr int RANK_MAX_P = 8192;      // the row's keys in LDS: 32 KiB

constexpr int CURVE_L = 16;           // steps per chunk: part of the summation order, hence compile-time
constexpr int CURVE_THREADS = 256;    // 4 waves
constexpr int CURVE_WAVES = CURVE_THREADS / 64;
static_assert(CURVE_L + 1 <= 64, "lane j of a wave holds step j of its chunk, j = 0 .. CURVE_L");

// A total order on floats as unsigned keys, larger key = ranked earlier: -0.0 is +0.0, every NaN is the lowest key (0; -inf
// maps to 0x007fffff, above it).
__device__ __forceinline__ uint32_t rank_key(float v) {
  if (v != v) return 0u;
  uint32_t u = __float_as_uint(v);
  if ((u << 1) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One workgroup per row: rank[p] = #{s : key[s] > key[p] or (key[s] == key[p] and s < p)}, order[rank[p]] = p.  Every lane of
// a wave reads the same key[s] (an LDS broadcast); the ranks of a row are a permutation of 0 .. P-1 whatever the input.
__global__ void __launch_bounds__(RANK_THREADS) rank_desc_kernel(const float* maps, int* order, int P) {
  extern __shared__ __attribute__((aligned(16))) uint32_t keys[];
  const float* row = maps + (int64_t)blockIdx.x * P;
  int* out = order + (int64_t)blockIdx.x * P;
  for (int i = threadIdx.x; i < P; i += RANK_THREADS) keys[i] = rank_key(row[i]);
  __syncthreads();
  for (int p = threadIdx.x; p < P; p += RANK_THREADS) {
    const uint32_t kp = keys[p];
    int rank = 0;
    for (int s = 0; s < p; ++s) rank += keys[s] >= kp;
    for (int s = p + 1; s < P; ++s) rank += keys[s] > kp;
    out[rank] = p;
  }
}

__device__ __forceinline__ int lane_int(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ float lane_float(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }

// What lane j < n of the wave of (b, chunk) holds: step j's position (-1 for an entry outside [0, P), which contributes
// nothing and is never an address) and its attention weights.
template <int G>
__device__ __forceinline__ void chunk_steps(const int* order, const float* probs, int b, int k0, int n, int P, int lane, int& pos,
                                            float (&w)[G]) {
  pos = -1;
  if (lane < n) {
    const int s = order[(int64_t)b * P + k0 + lane];
    if ((unsigned)s < (unsigned)P) pos = s;
  }
#pragma unroll
  for (int g = 0; g < G; ++g) w[g] = pos >= 0 ? probs[((int64_t)b * G + g) * P + pos] : 0.f;
}

__device__ __forceinline__ void axpy4(float4& a, float w, const float4 u) {
  a.x = fmaf(w, u.x, a.x); a.y = fmaf(w, u.y, a.y); a.z = fmaf(w, u.z, a.z); a.w = fmaf(w, u.w, a.w);
}

// Pass one.  One wave per (b, chunk): sum[b][c][g][:] = sum_j probs[b][g][s_j] * U[row][s_j][g][:] over the chunk's steps j in
// ascending order from 0, lane l over the quads l, l + 64, ...; mass[b][c][g] the same sum of the weights.
template <int G>
__global__ void __launch_bounds__(CURVE_THREADS)
curve_chunk_sum_kernel(const float* U, const int* slot, int slot0, int R, const float* probs, const int* order, float* sum,
                       float* mass, int B, int nch, int P, int hid) {
  const int lane = threadIdx.x & 63;
  const int64_t task = (int64_t)blockIdx.x * CURVE_WAVES + (threadIdx.x >> 6);
  if (task >= (int64_t)B * nch) return;                               // wave-uniform; no barrier in this kernel
  const int b = (int)(task / nch), c = (int)(task - (int64_t)b * nch);
  const int row = occl_row(slot, b, slot0, R);
  if (row < 0) return;
  const int k0 = c * CURVE_L, n = min(CURVE_L, P - k0), nq = hid >> 2;
  int pos;
  float w[G];
  chunk_steps<G>(order, probs, b, k0, n, P, lane, pos, w);
  const float4* Ub = reinterpret_cast<const float4*>(U + (int64_t)row * P * G * hid);
  float4* out = reinterpret_cast<float4*>(sum) + (int64_t)task * G * nq;
  for (int q = lane; q < nq; q += 64) {
    float4 acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < CURVE_L; ++j) {
      const int s = lane_int(pos, j);
      if (j < n && s >= 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) axpy4(acc[g], lane_float(w[g], j), Ub[((int64_t)s * G + g) * nq + q]);
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) out[g * nq + q] = acc[g];
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < CURVE_L; ++j) m += lane_float(w[g], j);        // 0 for j >= n and for an entry out of range
    if (lane == 0) mass[task * G + g] = m;
  }
}

// Pass two.  Per (b, element of [G][hid] or of the masses): pre[c] = the sum of chunks 0 .. c-1 in ascending order,
// and sum[c] is REPLACED by the sum of chunks nch-1 .. c+1 in descending order.  Element e of a question: a quad of the sums
// for e < G * nq, else one mass.
__global__ void __launch_bounds__(CURVE_THREADS)
curve_scan_kernel(float* sum, float* pre, float* mass, float* mass_pre, const int* slot, int slot0, int R, int B, int nch, int G,
                  int nq) {
  const int per = G * nq + G;
  const int64_t t = (int64_t)blockIdx.x * CURVE_THREADS + threadIdx.x;
  if (t >= (int64_t)B * per) return;
  const int b = (int)(t / per), e = (int)(t - (int64_t)b * per);
  if (occl_row(slot, b, slot0, R) < 0) return;
  if (e < G * nq) {
    float4* s4 = reinterpret_cast<float4*>(sum) + (int64_t)b * nch * G * nq + e;
    float4* p4 = reinterpret_cast<float4*>(pre) + (int64_t)b * nch * G * nq + e;
    const int64_t step = (int64_t)G * nq;
    float4 run = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = 0; c < nch; ++c) {
      const float4 v = s4[c * step];
      p4[c * step] = run;
      run.x += v.x; run.y += v.y; run.z += v.z; run.w += v.w;
    }
    run = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = nch - 1; c >= 0; --c) {
      const float4 v = s4[c * step];
      s4[c * step] = run;
      run.x += v.x; run.y += v.y; run.z += v.z; run.w += v.w;
    }
  } else {
    float* s1 = mass + (int64_t)b * nch * G + (e - G * nq);
    float* p1 = mass_pre + (int64_t)b * nch * G + (e - G * nq);
    float run = 0.f;
    for (int c = 0; c < nch; ++c) {
      const float v = s1[c * G];
      p1[c * G] = run;
      run += v;
    }
    run = 0.f;
    for (int c = nch - 1; c >= 0; --c) {
      const float v = s1[c * G];
      s1[c * G] = run;
      run += v;
    }
  }
}

// alpha of a kept set with mass m that leaves `absent` positions out: each of those keeps the weight r
__device__ __forceinline__ float kept_alpha(float m, int absent, float r) { return 1.f / fmaf((float)absent, r, m); }

// this lane's part of W2[a] . relu(base + sum_g alpha[g] * acc[g]) for one quad
template <int G>
__device__ __forceinline__ float kept_dot(const float4 (&acc)[G], const float (&alpha)[G], float4 pre, const float4 w2) {
#pragma unroll
  for (int g = 0; g < G; ++g) {
    pre.x = fmaf(alpha[g], acc[g].x, pre.x); pre.y = fmaf(alpha[g], acc[g].y, pre.y);
    pre.z = fmaf(alpha[g], acc[g].z, pre.z); pre.w = fmaf(alpha[g], acc[g].w, pre.w);
  }
  return fmaf(w2.w, fmaxf(pre.w, 0.f), fmaf(w2.z, fmaxf(pre.z, 0.f), fmaf(w2.y, fmaxf(pre.y, 0.f), w2.x * fmaxf(pre.x, 0.f))));
}

// The walk.  Workgroup = (question b, CURVE_WAVES consecutive chunks); it starts with occl_head (occl_core.hpp): base and
// W2[a] into LDS and r[g]; dynamic LDS occl_lds(2, hid).  Then wave w takes chunk c: state j of the chunk, j = 0 .. n, has
// the chunk's first j steps on the insertion side (kept set order[: k0 + j]) and its steps j .. n-1 on the deletion side (kept
// set order[k0 + j :]).  Lane j holds step j's position and weights and both alphas of state j; the masses are walked by every
// lane alike.  Per quad the insertion sums start from the prefix and add the rows j = 0 .. n-1, the deletion sums start from
// the suffix and add the rows j = n-1 .. 0; each state's dot product is finished by the wave butterfly.  insertion[k0 + j] is
// written for j = 1 .. n (j = 0 by chunk 0 alone), deletion[k0 + j] for j = 0 .. n-1 (j = n by the last chunk alone): every
// element once.
template <int G>
__global__ void __launch_bounds__(CURVE_THREADS)
curve_walk_kernel(const float* base, const float* U, const int* slot, int slot0, int R, const float* probs, const float* score,
                  const float* cnull, const float* W2, int64_t w2_ld, const float* b2, const int* answers, const int* order,
                  const float* suf, const float* pre, const float* mass_suf, const float* mass_pre, float* deletion,
                  float* insertion, int ngroup, int nch, int P, int hid, int A) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int b = blockIdx.x / ngroup;
  const int cg = blockIdx.x - b * ngroup;
  const int row = occl_row(slot, b, slot0, R);
  if (row < 0) return;                                                // block-uniform
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = answers[b];
  float* del = deletion + (int64_t)b * (P + 1);
  float* ins = insertion + (int64_t)b * (P + 1);
  if ((unsigned)a >= (unsigned)A) {
    const int k = cg * CURVE_WAVES * CURVE_L + tid;
    if (tid < CURVE_WAVES * CURVE_L && k < P) del[k] = ins[k] = 0.f;
    if (cg == ngroup - 1 && tid == 0) del[P] = ins[P] = 0.f;
    return;
  }
  float* s_base = sm;                 // [hid]
  float* s_w2 = sm + hid;             // [hid]
  float* red = sm + 2 * (size_t)hid;  // [16]
  float* s_r = red + 16;              // [G]
  const int nq = hid >> 2;
  occl_head<G, CURVE_THREADS>(base, score, cnull, W2, w2_ld, b, a, P, hid, s_base, s_w2, red, s_r);
  const int c = cg * CURVE_WAVES + wave;
  if (c >= nch) return;                                               // wave-uniform; no barrier below
  const int k0 = c * CURVE_L, n = min(CURVE_L, P - k0);
  int pos;
  float w[G];
  chunk_steps<G>(order, probs, b, k0, n, P, lane, pos, w);
  // both alphas of state `lane`: the masses walked in the sums' order, by every lane alike
  float a_ins[G], a_del[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float r = s_r[g];
    a_ins[g] = a_del[g] = 0.f;
    float m = mass_pre[((int64_t)b * nch + c) * G + g];
#pragma unroll
    for (int j = 0; j <= CURVE_L; ++j) {
      if (lane == j) a_ins[g] = kept_alpha(m, P - (k0 + j), r);
      if (j < CURVE_L) m += lane_float(w[g], j);                       // +0 beyond n: those states are never read
    }
    m = mass_suf[((int64_t)b * nch + c) * G + g];
#pragma unroll
    for (int j = CURVE_L; j >= 0; --j) {
      if (j < CURVE_L && j < n) m += lane_float(w[g], j);
      if (j <= n && lane == j) a_del[g] = kept_alpha(m, k0 + j, r);
    }
  }
  const float4* Ub = reinterpret_cast<const float4*>(U + (int64_t)row * P * G * hid);
  const float4* pre4 = reinterpret_cast<const float4*>(pre) + ((int64_t)b * nch + c) * G * nq;
  const float4* suf4 = reinterpret_cast<const float4*>(suf) + ((int64_t)b * nch + c) * G * nq;
  float d_ins[CURVE_L + 1], d_del[CURVE_L + 1];
#pragma unroll
  for (int j = 0; j <= CURVE_L; ++j) d_ins[j] = d_del[j] = 0.f;
  for (int q = lane; q < nq; q += 64) {
    const float4 bq = reinterpret_cast<const float4*>(s_base)[q];
    const float4 w2 = reinterpret_cast<const float4*>(s_w2)[q];
    float4 acc[G];
    float al[G];
    // insertion: from the prefix, forward
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = pre4[g * nq + q];
#pragma unroll
    for (int j = 0; j <= CURVE_L; ++j) {
      if (j <= n) {
#pragma unroll
        for (int g = 0; g < G; ++g) al[g] = lane_float(a_ins[g], j);
        d_ins[j] += kept_dot<G>(acc, al, bq, w2);
      }
      if (j < CURVE_L) {
        const int s = lane_int(pos, j);
        if (j < n && s >= 0) {
#pragma unroll
          for (int g = 0; g < G; ++g) axpy4(acc[g], lane_float(w[g], j), Ub[((int64_t)s * G + g) * nq + q]);
        }
      }
    }
    // deletion: from the suffix, backward
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = suf4[g * nq + q];
#pragma unroll
    for (int j = CURVE_L; j >= 0; --j) {
      if (j < CURVE_L) {
        const int s = lane_int(pos, j);
        if (j < n && s >= 0) {
#pragma unroll
          for (int g = 0; g < G; ++g) axpy4(acc[g], lane_float(w[g], j), Ub[((int64_t)s * G + g) * nq + q]);
        }
      }
      if (j <= n) {
#pragma unroll
        for (int g = 0; g < G; ++g) al[g] = lane_float(a_del[g], j);
        d_del[j] += kept_dot<G>(acc, al, bq, w2);
      }
    }
  }
  const float bias = b2[a];
#pragma unroll
  for (int j = 0; j <= CURVE_L; ++j) {
    if (j <= n) {                                                     // wave-uniform
      const float vi = wave_sum(d_ins[j]) + bias, vd = wave_sum(d_del[j]) + bias;
      if (lane == 0) {
        if (j > 0 || c == 0) ins[k0 + j] = vi;
        if (j < n || c == nch - 1) del[k0 + j] = vd;
      }
    }
  }
}

static int curve_chunks(int P) { return (P + CURVE_L - 1) / CURVE_L; }

}  // namespace vqa

using namespace vqa;

extern "C" {

int vqa_rank_desc(const float* maps, int32_t* order, int B, int P, vqa_stream_t stream) {
  set_launch_tag(-1);
  const char* who = "vqa_rank_desc";
  VQA_REQUIRE(maps && order, "%s: null pointer", who);
  VQA_REQUIRE(B >= 0 && P >= 1 && P <= RANK_MAX_P, "%s: B=%d, P=%d out of range (P in 1..%d)", who, B, P, RANK_MAX_P);
  if (B == 0) return VQA_OK;
  hipLaunchKernelGGL(rank_desc_kernel, dim3(B), dim3(RANK_THREADS), (size_t)P * 4, (hipStream_t)stream, maps, order, P);
  return check_hip(hipGetLastError(), "rank_desc launch");
}

int vqa_occl_curves_chunk(void) { return CURVE_L; }

int64_t vqa_occl_curves_workspace_bytes(int B, int P, int G, int hid) {
  if (B < 1 || P < 1 || G < 1 || hid < 1) return 0;
  return 2 * (int64_t)B * curve_chunks(P) * G * ((int64_t)hid + 1) * 4;
}

int vqa_occl_curves(const float* base, const float* U, const int32_t* slot, int slot0, const float* probs, const float* score,
                    const float* cnull, const float* W2, int64_t w2_ld, const float* b2, const int32_t* answers,
                    const int32_t* order, float* workspace, int64_t workspace_bytes, float* deletion, float* insertion, int R,
                    int B, int P, int hid, int G, int A, vqa_stream_t stream) {
  set_launch_tag(-1);
  const char* who = "vqa_occl_curves";
  const bool pointers = base && U && slot && probs && score && cnull && W2 && b2 && answers && order && deletion && insertion;
  // without questions nothing is read, so no alignment is asked for (and no workspace, below)
  if (const int rc = occl_check(who, G, pointers, hid, w2_ld, 2, "2", B ? ptr_bits(base, U, W2, workspace) : 0,
                                "base, U, W2 and the workspace", R >= 1 && B >= 0 && P >= 1 && P <= (1 << 20) && A >= 1,
                                "%s: R=%d, B=%d, P=%d, A=%d out of range", R, B, P, A))
    return rc;
  if (B == 0) return VQA_OK;
  const int64_t need = vqa_occl_curves_workspace_bytes(B, P, G, hid);
  VQA_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
              (long long)need);
  const int nch = curve_chunks(P), nq = hid >> 2;
  const int ngroup = (nch + CURVE_WAVES - 1) / CURVE_WAVES;
  const int64_t tasks = (int64_t)B * nch, scan = (int64_t)B * (G * nq + G);
  VQA_REQUIRE((int64_t)B * ngroup < (1LL << 31) && (scan + CURVE_THREADS - 1) / CURVE_THREADS < (1LL << 31),
              "%s: B=%d x %d chunks exceed the grid", who, B, nch);
  // workspace: chunk sums / suffixes [B][nch][G][hid], prefixes [B][nch][G][hid], then the same two of the masses [B][nch][G]
  float* sum = workspace;
  float* pre = sum + tasks * G * hid;
  float* mass = pre + tasks * G * hid;
  float* mass_pre = mass + tasks * G;
  hipStream_t s = (hipStream_t)stream;
  return with_int14(G, [&](auto g) {
    constexpr int GG = decltype(g)::value;
    hipLaunchKernelGGL(curve_chunk_sum_kernel<GG>, dim3((unsigned)((tasks + CURVE_WAVES - 1) / CURVE_WAVES)), dim3(CURVE_THREADS),
                       0, s, U, slot, slot0, R, probs, order, sum, mass, B, nch, P, hid);
    int rc = check_hip(hipGetLastError(), "occl_curves chunk-sum launch");
    if (rc) return rc;
    hipLaunchKernelGGL(curve_scan_kernel, dim3((unsigned)((scan + CURVE_THREADS - 1) / CURVE_THREADS)), dim3(CURVE_THREADS), 0, s,
                       sum, pre, mass, mass_pre, slot, slot0, R, B, nch, G, nq);
    rc = check_hip(hipGetLastError(), "occl_curves scan launch");
    if (rc) return rc;
    // the attribute is set once per kernel, so for the largest LDS size the check above admits
    rc = set_smem(curve_walk_kernel<GG>, 64 * 1024, "attr(occl_curves)");
    if (rc) return rc;
    hipLaunchKernelGGL(curve_walk_kernel<GG>, dim3(B * ngroup), dim3(CURVE_THREADS), occl_lds(2, hid), s, base, U, slot, slot0, R,
                       probs, score, cnull, W2, w2_ld, b2, answers, order, sum, pre, mass, mass_pre, deletion, insertion, ngroup,
                       nch, P, hid, A);
    return check_hip(hipGetLastError(), "occl_curves walk launch");
  });
}

}  // extern "C"
