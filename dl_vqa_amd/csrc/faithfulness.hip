// Deletion and insertion curves of an attribution map from cached features (vqa_rank_desc, vqa_occl_curves):
// the logit of one answer column with only the first k positions of a ranking present (insertion) and with the first k absent
// (deletion), k = 0 .. P, in the kept form of the closed form of csrc/occlusion.hip -- sums over the positions that REMAIN, so
// nothing is ever subtracted.  The ranking is cut into chunks of CURVE_L steps: one pass sums each chunk's probs * U rows, a
// small pass turns the chunk sums into exclusive prefixes (insertion) and suffixes (deletion), and the walk gives one wave per
// (question, chunk), which steps through its rows from its prefix forward and from its suffix backward.
// Sampled Shapley maps (vqa_occl_curves_orders, vqa_shapley_accumulate) walk the same three kernels over
// (question, order) pairs from one table of orders that every question shares -- curve_task is the one place that says which
// question and which order row a task reads -- and one more kernel folds the curves' steps into maps and error bars.
// Probability curves (vqa_occl_curves_hidden) run the same three kernels with the walk under a compile-time
// flag: it keeps every state's hidden row, from which one GEMM with W2 gives every answer column.
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

// A curve task t: the question it walks and the row of the order table it walks along.  t itself is the task's row of the
// workspace and of both outputs.  M == 0 (vqa_occl_curves): one order per question, task t is question t with order row t.
// M >= 1 (vqa_occl_curves_orders): task t = b * M + m is question b along row m of a table of M orders.
struct CurveTask { int b, o; };
__device__ __forceinline__ CurveTask curve_task(int t, int M) {
  if (M == 0) return {t, t};
  const int b = t / M;
  return {b, t - b * M};
}

// What lane j < n of the wave of (task, chunk) holds: step j's position (-1 for an entry outside [0, P), which contributes
// nothing and is never an address) and its attention weights.
template <int G>
__device__ __forceinline__ void chunk_steps(const int* order, const float* probs, CurveTask task, int k0, int n, int P, int lane,
                                            int& pos, float (&w)[G]) {
  const int b = task.b;
  pos = -1;
  if (lane < n) {
    const int s = order[(int64_t)task.o * P + k0 + lane];
    if ((unsigned)s < (unsigned)P) pos = s;
  }
#pragma unroll
  for (int g = 0; g < G; ++g) w[g] = pos >= 0 ? probs[((int64_t)b * G + g) * P + pos] : 0.f;
}

__device__ __forceinline__ void axpy4(float4& a, float w, const float4 u) {
  a.x = fmaf(w, u.x, a.x); a.y = fmaf(w, u.y, a.y); a.z = fmaf(w, u.z, a.z); a.w = fmaf(w, u.w, a.w);
}

// Pass one.  One wave per (task t, chunk), b the task's question: sum[t][c][g][:] = sum_j probs[b][g][s_j] * U[row][s_j][g][:]
// over the chunk's steps j in ascending order from 0, lane l over the quads l, l + 64, ...; mass[t][c][g] the same sum of the
// weights.
template <int G>
__global__ void __launch_bounds__(CURVE_THREADS)
curve_chunk_sum_kernel(const float* U, const int* slot, int slot0, int R, const float* probs, const int* order, float* sum,
                       float* mass, int T, int M, int nch, int P, int hid) {
  const int lane = threadIdx.x & 63;
  const int64_t task = (int64_t)blockIdx.x * CURVE_WAVES + (threadIdx.x >> 6);
  if (task >= (int64_t)T * nch) return;                               // wave-uniform; no barrier in this kernel
  const int t = (int)(task / nch), c = (int)(task - (int64_t)t * nch);
  const CurveTask ct = curve_task(t, M);
  const int row = occl_row(slot, ct.b, slot0, R);
  if (row < 0) return;
  const int k0 = c * CURVE_L, n = min(CURVE_L, P - k0), nq = hid >> 2;
  int pos;
  float w[G];
  chunk_steps<G>(order, probs, ct, k0, n, P, lane, pos, w);
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

// Pass two.  Per (task, element of [G][hid] or of the masses): pre[c] = the sum of chunks 0 .. c-1 in ascending order,
// and sum[c] is REPLACED by the sum of chunks nch-1 .. c+1 in descending order.  Element e of a question: a quad of the sums
// for e < G * nq, else one mass.
__global__ void __launch_bounds__(CURVE_THREADS)
curve_scan_kernel(float* sum, float* pre, float* mass, float* mass_pre, const int* slot, int slot0, int R, int T, int M, int nch,
                  int G, int nq) {
  const int per = G * nq + G;
  const int64_t i = (int64_t)blockIdx.x * CURVE_THREADS + threadIdx.x;
  if (i >= (int64_t)T * per) return;
  const int t = (int)(i / per), e = (int)(i - (int64_t)t * per);
  if (occl_row(slot, curve_task(t, M).b, slot0, R) < 0) return;
  if (e < G * nq) {
    float4* s4 = reinterpret_cast<float4*>(sum) + (int64_t)t * nch * G * nq + e;
    float4* p4 = reinterpret_cast<float4*>(pre) + (int64_t)t * nch * G * nq + e;
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
    float* s1 = mass + (int64_t)t * nch * G + (e - G * nq);
    float* p1 = mass_pre + (int64_t)t * nch * G + (e - G * nq);
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

// one quad of base + sum_g alpha[g] * acc[g], g ascending: the hidden row of a kept set before its relu
template <int G>
__device__ __forceinline__ float4 kept_pre(const float4 (&acc)[G], const float (&alpha)[G], float4 pre) {
#pragma unroll
  for (int g = 0; g < G; ++g) {
    pre.x = fmaf(alpha[g], acc[g].x, pre.x); pre.y = fmaf(alpha[g], acc[g].y, pre.y);
    pre.z = fmaf(alpha[g], acc[g].z, pre.z); pre.w = fmaf(alpha[g], acc[g].w, pre.w);
  }
  return pre;
}

// this lane's part of W2[a] . relu(base + sum_g alpha[g] * acc[g]) for one quad
template <int G>
__device__ __forceinline__ float kept_dot(const float4 (&acc)[G], const float (&alpha)[G], float4 base, const float4 w2) {
  const float4 pre = kept_pre<G>(acc, alpha, base);
  return fmaf(w2.w, fmaxf(pre.w, 0.f), fmaf(w2.z, fmaxf(pre.z, 0.f), fmaf(w2.y, fmaxf(pre.y, 0.f), w2.x * fmaxf(pre.x, 0.f))));
}

// the same quad as the hidden row itself: relu(base + sum_g alpha[g] * acc[g])
template <int G>
__device__ __forceinline__ float4 kept_hidden(const float4 (&acc)[G], const float (&alpha)[G], float4 base) {
  const float4 pre = kept_pre<G>(acc, alpha, base);
  return make_float4(fmaxf(pre.x, 0.f), fmaxf(pre.y, 0.f), fmaxf(pre.z, 0.f), fmaxf(pre.w, 0.f));
}

// The walk.  Workgroup = (task t, CURVE_WAVES consecutive chunks); it starts with occl_head (occl_core.hpp) for the task's
// question b: base and W2[a] into LDS and r[g]; dynamic LDS occl_lds(2, hid).  Then wave w takes chunk c: state j, j = 0 .. n, has
// the chunk's first j steps on the insertion side (kept set order[: k0 + j]) and its steps j .. n-1 on the deletion side (kept
// set order[k0 + j :]).  Lane j holds step j's position and weights and both alphas of state j; the masses are walked by every
// lane alike.  Per quad the insertion sums start from the prefix and add the rows j = 0 .. n-1, the deletion sums start from
// the suffix and add the rows j = n-1 .. 0; each state's dot product is finished by the wave butterfly.  insertion[k0 + j] is
// written for j = 1 .. n (j = 0 by chunk 0 alone), deletion[k0 + j] for j = 0 .. n-1 (j = n by the last chunk alone): every
// element once.
// HIDDEN (vqa_occl_curves_hidden): the same walk -- the same chunk_steps, alphas, accumulation order and CURVE_L -- that keeps
// each state's hidden row relu(base + sum_g alpha_g * acc_g) instead of collapsing it onto one W2 row.  No column is explained:
// W2, b2, answers and A are not looked at, the head loads no W2 (dynamic LDS occl_lds(1, hid)) and there is no butterfly.  Lane l
// stores its quad of state j as one float4, 64 lanes 1 KiB contiguous, into hidden [T][2][P + 1][hid]: [t][1][k0 + j] for the
// insertion states, [t][0][k0 + j] for the deletion states, under the same once-only rule (deletion / insertion unused).
template <int G, bool HIDDEN = false>
__global__ void __launch_bounds__(CURVE_THREADS)
curve_walk_kernel(const float* base, const float* U, const int* slot, int slot0, int R, const float* probs, const float* score,
                  const float* cnull, const float* W2, int64_t w2_ld, const float* b2, const int* answers, const int* order,
                  const float* suf, const float* pre, const float* mass_suf, const float* mass_pre, float* deletion,
                  float* insertion, int M, int ngroup, int nch, int P, int hid, int A, float* hidden) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int t = blockIdx.x / ngroup;
  const int cg = blockIdx.x - t * ngroup;
  const CurveTask ct = curve_task(t, M);
  const int b = ct.b;
  const int row = occl_row(slot, b, slot0, R);
  if (row < 0) return;                                                // block-uniform
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int a = 0;
  float *del = nullptr, *ins = nullptr;
  if constexpr (!HIDDEN) {
    a = answers[b];
    del = deletion + (int64_t)t * (P + 1);
    ins = insertion + (int64_t)t * (P + 1);
    if ((unsigned)a >= (unsigned)A) {
      const int k = cg * CURVE_WAVES * CURVE_L + tid;
      if (tid < CURVE_WAVES * CURVE_L && k < P) del[k] = ins[k] = 0.f;
      if (cg == ngroup - 1 && tid == 0) del[P] = ins[P] = 0.f;
      return;
    }
  }
  float* s_base = sm;                                   // [hid]
  float* s_w2 = sm + hid;                               // [hid]; HIDDEN: not there
  float* red = sm + (HIDDEN ? 1 : 2) * (size_t)hid;     // [16]
  float* s_r = red + 16;                                // [G]
  const int nq = hid >> 2;
  occl_head<G, CURVE_THREADS, !HIDDEN>(base, score, cnull, W2, w2_ld, b, a, P, hid, s_base, s_w2, red, s_r);
  const int c = cg * CURVE_WAVES + wave;
  if (c >= nch) return;                                               // wave-uniform; no barrier below
  const int k0 = c * CURVE_L, n = min(CURVE_L, P - k0);
  int pos;
  float w[G];
  chunk_steps<G>(order, probs, ct, k0, n, P, lane, pos, w);
  // both alphas of state `lane`: the masses walked in the sums' order, by every lane alike
  float a_ins[G], a_del[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float r = s_r[g];
    a_ins[g] = a_del[g] = 0.f;
    float m = mass_pre[((int64_t)t * nch + c) * G + g];
#pragma unroll
    for (int j = 0; j <= CURVE_L; ++j) {
      if (lane == j) a_ins[g] = kept_alpha(m, P - (k0 + j), r);
      if (j < CURVE_L) m += lane_float(w[g], j);                       // +0 beyond n: those states are never read
    }
    m = mass_suf[((int64_t)t * nch + c) * G + g];
#pragma unroll
    for (int j = CURVE_L; j >= 0; --j) {
      if (j < CURVE_L && j < n) m += lane_float(w[g], j);
      if (j <= n && lane == j) a_del[g] = kept_alpha(m, k0 + j, r);
    }
  }
  const float4* Ub = reinterpret_cast<const float4*>(U + (int64_t)row * P * G * hid);
  const float4* pre4 = reinterpret_cast<const float4*>(pre) + ((int64_t)t * nch + c) * G * nq;
  const float4* suf4 = reinterpret_cast<const float4*>(suf) + ((int64_t)t * nch + c) * G * nq;
  // HIDDEN: the rows [t][0][k0] (deletion) and [t][1][k0] (insertion) of the output, as quads
  float4* h_del = HIDDEN ? reinterpret_cast<float4*>(hidden) + (((int64_t)t * 2) * (P + 1) + k0) * nq : nullptr;
  float4* h_ins = HIDDEN ? h_del + (int64_t)(P + 1) * nq : nullptr;
  float d_ins[HIDDEN ? 1 : CURVE_L + 1], d_del[HIDDEN ? 1 : CURVE_L + 1];
  if constexpr (!HIDDEN) {
#pragma unroll
    for (int j = 0; j <= CURVE_L; ++j) d_ins[j] = d_del[j] = 0.f;
  }
  for (int q = lane; q < nq; q += 64) {
    const float4 bq = reinterpret_cast<const float4*>(s_base)[q];
    float4 w2 = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (!HIDDEN) w2 = reinterpret_cast<const float4*>(s_w2)[q];
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
        if constexpr (HIDDEN) {
          if (j > 0 || c == 0) h_ins[(int64_t)j * nq + q] = kept_hidden<G>(acc, al, bq);
        } else {
          d_ins[j] += kept_dot<G>(acc, al, bq, w2);
        }
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
        if constexpr (HIDDEN) {
          if (j < n || c == nch - 1) h_del[(int64_t)j * nq + q] = kept_hidden<G>(acc, al, bq);
        } else {
          d_del[j] += kept_dot<G>(acc, al, bq, w2);
        }
      }
    }
  }
  if constexpr (!HIDDEN) {
    const float bias = b2[a];
#pragma unroll
    for (int j = 0; j <= CURVE_L; ++j) {
      if (j <= n) {                                                   // wave-uniform
        const float vi = wave_sum(d_ins[j]) + bias, vd = wave_sum(d_del[j]) + bias;
        if (lane == 0) {
          if (j > 0 || c == 0) ins[k0 + j] = vi;
          if (j < n || c == nch - 1) del[k0 + j] = vd;
        }
      }
    }
  }
}


constexpr int SHAPLEY_THREADS = 256;

// Curves into Shapley estimates.  One thread owns (b, p) and folds the Mg orders of this launch into its running mean and M2
// (Welford) in ascending m, the orders before them counted by m0: with k = rank[m][p] the step at which order m reaches p,
//   e = 0.5 * ((ins[k + 1] - ins[k]) + (del[k] - del[k + 1]))        of the curves of (b, m)
//   d = e - mean;  mean += d / (m0 + m + 1);  M2 = fma(d, e - mean, M2)
// One fixed sequence of roundings per (b, p) whatever the grouping: the state crosses launches as the fp32 it is in registers.
// total > 0 (the last group): maps = mean, err = sqrt(M2 / (total * (total - 1))), NaN for total == 1.  A rank entry outside
// [0, P) is no address and gives e = 0.  m0 == 0 with `empty`: the thread of p == 0 also writes empty[b] = ins[0] of the
// group's first order, the logit of the empty image.  A question outside the slot window is left alone; a column outside
// [0, A): +0.0 everywhere.
__global__ void __launch_bounds__(SHAPLEY_THREADS)
shapley_accumulate_kernel(const float* deletion, const float* insertion, const int* rank, const int* slot, int slot0, int R,
                          const int* answers, int A, float* mean, float* m2, float* maps, float* err, float* empty, int B, int P,
                          int Mg, int m0, int total) {
  const int64_t i = (int64_t)blockIdx.x * SHAPLEY_THREADS + threadIdx.x;
  if (i >= (int64_t)B * P) return;
  const int b = (int)(i / P), p = (int)(i - (int64_t)b * P);
  if (occl_row(slot, b, slot0, R) < 0) return;
  if ((unsigned)answers[b] >= (unsigned)A) {
    mean[i] = m2[i] = 0.f;
    if (total > 0) maps[i] = err[i] = 0.f;
    if (empty && m0 == 0 && p == 0) empty[b] = 0.f;
    return;
  }
  if (empty && m0 == 0 && p == 0) empty[b] = insertion[(int64_t)b * Mg * (P + 1)];
  float mu = m0 ? mean[i] : 0.f, s2 = m0 ? m2[i] : 0.f;
  for (int m = 0; m < Mg; ++m) {
    const int k = rank[(int64_t)m * P + p];
    float e = 0.f;
    if ((unsigned)k < (unsigned)P) {
      const int64_t at = ((int64_t)b * Mg + m) * (P + 1) + k;
      e = 0.5f * ((insertion[at + 1] - insertion[at]) + (deletion[at] - deletion[at + 1]));
    }
    const float d = e - mu;
    mu += d / (float)(m0 + m + 1);
    s2 = fmaf(d, e - mu, s2);
  }
  mean[i] = mu;
  m2[i] = s2;
  if (total > 0) {
    maps[i] = mu;
    err[i] = total > 1 ? sqrtf(fmaxf(s2, 0.f) / ((float)total * (float)(total - 1))) : __int_as_float(0x7fc00000);
  }
}

static int curve_chunks(int P) { return (P + CURVE_L - 1) / CURVE_L; }

// bytes of the workspace of T curve tasks
static int64_t curve_workspace_bytes(int64_t T, int P, int G, int hid) {
  return 2 * T * curve_chunks(P) * G * ((int64_t)hid + 1) * 4;
}

// What vqa_occl_curves (M == 0: B tasks, order [B][P]) and vqa_occl_curves_orders (M >= 1: B * M tasks, order [M][P]) do
// alike: the checks, the workspace layout and the three launches over the tasks (curve_task).  vqa_occl_curves_hidden (M == 0)
// too: `hidden` [B][2][P + 1][hid] in place of W2, b2, answers, deletion and insertion (all null, w2_ld = hid, A = 1), the
// third launch being the walk that keeps its hidden rows.
static int curves_launch(const char* who, const float* base, const float* U, const int32_t* slot, int slot0, const float* probs,
                         const float* score, const float* cnull, const float* W2, int64_t w2_ld, const float* b2,
                         const int32_t* answers, const int32_t* order, float* workspace, int64_t workspace_bytes, float* deletion,
                         float* insertion, float* hidden, int R, int B, int M, int P, int hid, int G, int A, hipStream_t s) {
  const bool pointers = base && U && slot && probs && score && cnull && order &&
                        (hidden ? true : W2 && b2 && answers && deletion && insertion);
  // without questions nothing is read, so no alignment is asked for (and no workspace, below)
  if (const int rc = occl_check(who, G, pointers, hid, w2_ld, hidden ? 1 : 2, hidden ? "1" : "2",
                                B ? ptr_bits(base, U, W2, workspace, hidden) : 0,
                                hidden ? "base, U, the workspace and the hidden rows" : "base, U, W2 and the workspace",
                                R >= 1 && B >= 0 && P >= 1 && P <= (1 << 20) && A >= 1, "%s: R=%d, B=%d, P=%d, A=%d out of range", R,
                                B, P, A))
    return rc;
  if (B == 0) return VQA_OK;
  const int64_t T = (int64_t)B * (M ? M : 1);
  const int64_t need = curve_workspace_bytes(T, P, G, hid);
  VQA_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
              (long long)need);
  const int nch = curve_chunks(P), nq = hid >> 2;
  const int ngroup = (nch + CURVE_WAVES - 1) / CURVE_WAVES;
  const int64_t tasks = T * nch, scan = T * (G * nq + G);
  VQA_REQUIRE(T * ngroup < (1LL << 31) && (scan + CURVE_THREADS - 1) / CURVE_THREADS < (1LL << 31),
              "%s: B=%d x %d orders x %d chunks exceed the grid", who, B, M ? M : 1, nch);
  // workspace: chunk sums / suffixes [T][nch][G][hid], prefixes [T][nch][G][hid], then the same two of the masses [T][nch][G]
  float* sum = workspace;
  float* pre = sum + tasks * G * hid;
  float* mass = pre + tasks * G * hid;
  float* mass_pre = mass + tasks * G;
  return with_int14(G, [&](auto g) {
    constexpr int GG = decltype(g)::value;
    hipLaunchKernelGGL(curve_chunk_sum_kernel<GG>, dim3((unsigned)((tasks + CURVE_WAVES - 1) / CURVE_WAVES)), dim3(CURVE_THREADS),
                       0, s, U, slot, slot0, R, probs, order, sum, mass, (int)T, M, nch, P, hid);
    int rc = check_hip(hipGetLastError(), "occl_curves chunk-sum launch");
    if (rc) return rc;
    hipLaunchKernelGGL(curve_scan_kernel, dim3((unsigned)((scan + CURVE_THREADS - 1) / CURVE_THREADS)), dim3(CURVE_THREADS), 0, s,
                       sum, pre, mass, mass_pre, slot, slot0, R, (int)T, M, nch, G, nq);
    rc = check_hip(hipGetLastError(), "occl_curves scan launch");
    if (rc) return rc;
    // the attribute is set once per kernel, so for the largest LDS size the check above admits
    auto walk = hidden ? curve_walk_kernel<GG, true> : curve_walk_kernel<GG, false>;
    rc = set_smem(walk, 64 * 1024, hidden ? "attr(occl_curves_hidden)" : "attr(occl_curves)");
    if (rc) return rc;
    hipLaunchKernelGGL(walk, dim3((unsigned)(T * ngroup)), dim3(CURVE_THREADS), occl_lds(hidden ? 1 : 2, hid), s, base, U, slot,
                       slot0, R, probs, score, cnull, W2, w2_ld, b2, answers, order, sum, pre, mass, mass_pre, deletion, insertion,
                       M, ngroup, nch, P, hid, A, hidden);
    return check_hip(hipGetLastError(), hidden ? "occl_curves_hidden walk launch" : "occl_curves walk launch");
  });
}

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
  return curve_workspace_bytes(B, P, G, hid);
}

int vqa_occl_curves(const float* base, const float* U, const int32_t* slot, int slot0, const float* probs, const float* score,
                    const float* cnull, const float* W2, int64_t w2_ld, const float* b2, const int32_t* answers,
                    const int32_t* order, float* workspace, int64_t workspace_bytes, float* deletion, float* insertion, int R,
                    int B, int P, int hid, int G, int A, vqa_stream_t stream) {
  set_launch_tag(-1);
  return curves_launch("vqa_occl_curves", base, U, slot, slot0, probs, score, cnull, W2, w2_ld, b2, answers, order, workspace,
                       workspace_bytes, deletion, insertion, nullptr, R, B, 0, P, hid, G, A, (hipStream_t)stream);
}

int vqa_occl_curves_hidden(const float* base, const float* U, const int32_t* slot, int slot0, const float* probs,
                           const float* score, const float* cnull, const int32_t* order, float* workspace, int64_t workspace_bytes,
                           float* hidden, int R, int B, int P, int hid, int G, vqa_stream_t stream) {
  set_launch_tag(-1);
  const char* who = "vqa_occl_curves_hidden";
  // a null `hidden` reads as the column form without its operands: curves_launch's own "null pointer"
  return curves_launch(who, base, U, slot, slot0, probs, score, cnull, nullptr, hid, nullptr, nullptr, order, workspace,
                       workspace_bytes, nullptr, nullptr, hidden, R, B, 0, P, hid, G, 1, (hipStream_t)stream);
}

int64_t vqa_occl_curves_orders_workspace_bytes(int B, int M, int P, int G, int hid) {
  if (B < 1 || M < 1 || P < 1 || G < 1 || hid < 1) return 0;
  return curve_workspace_bytes((int64_t)B * M, P, G, hid);
}

int vqa_occl_curves_orders(const float* base, const float* U, const int32_t* slot, int slot0, const float* probs,
                           const float* score, const float* cnull, const float* W2, int64_t w2_ld, const float* b2,
                           const int32_t* answers, const int32_t* orders, float* workspace, int64_t workspace_bytes,
                           float* deletion, float* insertion, int R, int B, int M, int P, int hid, int G, int A,
                           vqa_stream_t stream) {
  set_launch_tag(-1);
  const char* who = "vqa_occl_curves_orders";
  VQA_REQUIRE(M >= 1 && (int64_t)(B > 0 ? B : 0) * M < (1LL << 31), "%s: M=%d orders for B=%d questions out of range", who, M, B);
  return curves_launch(who, base, U, slot, slot0, probs, score, cnull, W2, w2_ld, b2, answers, orders, workspace, workspace_bytes,
                       deletion, insertion, nullptr, R, B, M, P, hid, G, A, (hipStream_t)stream);
}

int vqa_shapley_accumulate(const float* deletion, const float* insertion, const int32_t* rank, const int32_t* slot, int slot0,
                           const int32_t* answers, float* mean, float* m2, float* maps, float* err, float* empty, int R, int B,
                           int P, int Mg, int m0, int total, int A, vqa_stream_t stream) {
  set_launch_tag(-1);
  const char* who = "vqa_shapley_accumulate";
  VQA_REQUIRE(deletion && insertion && rank && slot && answers && mean && m2 && (total == 0 || (maps && err)), "%s: null pointer",
              who);
  VQA_REQUIRE(R >= 1 && B >= 0 && P >= 1 && P <= (1 << 20) && A >= 1, "%s: R=%d, B=%d, P=%d, A=%d out of range", who, R, B, P, A);
  VQA_REQUIRE(Mg >= 1 && m0 >= 0 && m0 <= (1 << 20) && Mg <= (1 << 20) && (total == 0 || total == m0 + Mg),
              "%s: Mg=%d orders after m0=%d, total=%d (0, or m0 + Mg on the last group)", who, Mg, m0, total);
  if (B == 0) return VQA_OK;
  const int64_t blocks = ((int64_t)B * P + SHAPLEY_THREADS - 1) / SHAPLEY_THREADS;
  VQA_REQUIRE(blocks < (1LL << 31), "%s: B=%d x P=%d exceed the grid", who, B, P);
  hipLaunchKernelGGL(shapley_accumulate_kernel, dim3((unsigned)blocks), dim3(SHAPLEY_THREADS), 0, (hipStream_t)stream, deletion,
                     insertion, rank, slot, slot0, R, answers, A, mean, m2, maps, err, empty, B, P, Mg, m0, total);
  return check_hip(hipGetLastError(), "shapley_accumulate launch");
}

}  // extern "C"
