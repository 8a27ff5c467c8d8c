// Host side that the three GEMM entry points share (vqa_gemm in gemm.hip, vqa_gemm_x3 in gemm_x3.hip, vqa_gemm_bf16 in
// bf16.hip): the plan, the argument check, the epilogue parameters, the split-K slab rule and its workspace claim, the
// operand-layout dispatch and the run tail.  Each rule is written here once.
#pragma once
#include "gemm_epilogue.hpp"

namespace vqa {

// Tile / split-K plan of a plain GEMM; bk = K-step depth in elements (32 fp32, 64 bf16).  big: 0 = 64 x 64 tiles, 1 = 128 x 128,
// 2 = 256 x 128; order: tile_coord's.  The x3 engine has one tile shape and one order and leaves both 0.
struct GemmPlan { int big; int tiles_m, tiles_n, nk, splits, ks_per_split, order; };
// splits as asked for, then as few as still cover the K-steps at that depth
inline void split_k(GemmPlan& p, int splits) { p.ks_per_split = (p.nk + splits - 1) / splits; p.splits = (p.nk + p.ks_per_split - 1) / p.ks_per_split; }
GemmPlan plan_gemm(int M, int N, int K, int bk = BK);
// vqa_gemm_bf16 only: replaces p by the 128 x 256 plan of a long-K weight gradient and returns true where that plan is admitted
bool plan_gemm_wide(GemmPlan& p, int M, int N, int K, int transA, int transB, bool has_workspace, int64_t workspace_bytes);
// vqa_gemm_x3's plan (gemm_x3.hip): one tile shape, X3_BM x X3_BN
constexpr int X3_BM = 192, X3_BN = 128;
GemmPlan plan_gemm_x3(int M, int N, int K);

// Whether a plan runs on the persistent kernel: asked by the launcher and by vqa_gemm_plan.
// vqa_gemm: tiles above 64 x 64 only, unsplit, K short (<= 16 K-steps) unless VQA_PERSISTENT=0/1 forces the choice
inline bool gemm_runs_persistent(const GemmPlan& p) {
  const int pt = knobs().persistent;
  return p.big != 0 && p.splits == 1 && (pt >= 0 ? pt == 1 : p.nk <= 16);
}
// vqa_gemm_x3: unsplit with more tiles than the 256 workgroups of its grid, unless VQA_PERSISTENT=0
inline bool gemm_x3_runs_persistent(const GemmPlan& p) {
  return p.splits == 1 && p.tiles_m * p.tiles_n > 256 && knobs().persistent != 0;
}

// Split-K partials [splits][M][N] in fp32: what *_workspace_bytes report and what the entry points claim.
inline int64_t slab_bytes(const GemmPlan& p, int M, int N) { return p.splits > 1 ? (int64_t)p.splits * M * N * 4 : 0; }

// Points pe.slab at the workspace when the plan splits K (nullptr otherwise); a workspace that is missing or too small is an error.
inline int claim_slab(const char* name, const GemmPlan& p, EpiParams& pe, float* workspace, int64_t workspace_bytes) {
  const int64_t need = slab_bytes(p, pe.M, pe.N);
  if (need && (!workspace || workspace_bytes < need)) {
    set_error("%s: workspace %lld bytes < %lld needed", name, (long long)workspace_bytes, (long long)need);
    return VQA_ERR_WORKSPACE;
  }
  pe.slab = need ? workspace : nullptr;
  return VQA_OK;
}

// What every engine asks of its operands; quantum = elements per 16 bytes (4 fp32, 8 bf16).
inline int check_gemm_args(const char* name, int quantum, const void* A, int64_t lda, const void* B, int64_t ldb, const void* C,
                           int64_t ldc, int M, int N, int K, const float* rowgroup, int rg_div) {
  VQA_REQUIRE(A && B && C, "%s: null operand", name);
  VQA_REQUIRE(M > 0 && N > 0 && K > 0, "%s: bad shape M=%d N=%d K=%d", name, M, N, K);
  VQA_REQUIRE(((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0 && lda % quantum == 0 && ldb % quantum == 0,
              "%s: A/B must be 16-byte aligned with leading dimensions multiple of %d (lda=%lld ldb=%lld)", name, quantum,
              (long long)lda, (long long)ldb);
  VQA_REQUIRE(lda < (1 << 21) && ldb < (1 << 21) && ldc < (1 << 21),
              "%s: leading dimensions must be below 2^21 (lda=%lld ldb=%lld ldc=%lld)", name, (long long)lda, (long long)ldb,
              (long long)ldc);
  VQA_REQUIRE(!rowgroup || rg_div > 0, "%s: rg_div must be positive", name);
  return VQA_OK;
}

// C: fp32 result, Cb: bf16 result (one of the two); slab is claim_slab's.
inline EpiParams epi_params(float* C, uint16_t* Cb, int64_t ldc, int M, int N, const float* bias1, const float* bias2,
                            const float* rowgroup, int64_t rg_ld, int rg_div, int rg_op, int relu, int accumulate, float* aux) {
  return EpiParams{C, ldc, M, N, bias1, bias2, rowgroup, rg_ld, rg_div, rg_op, relu, accumulate, aux, nullptr, Cb};
}

// Operand layouts: transA = 0 -> A is [M][K] (loader AR), 1 -> [K][M] (AC);  transB = 1 -> B is [N][K] (BR), 0 -> [K][N] (BC).
// f(Loader<A loader>{}, Loader<B loader>{}) launches with the pair.
template <class L> struct Loader { using type = L; };
template <class AR, class AC, class BR, class BC, class F>
int with_layout(int transA, int transB, F&& f) {
  return with_flags(transA != 0, transB != 0, [&](auto ta, auto tb) {
    return f(Loader<std::conditional_t<decltype(ta)::value, AC, AR>>{}, Loader<std::conditional_t<decltype(tb)::value, BR, BC>>{});
  });
}

// Reduction of the split-K slabs (pe.slab [splits][M][N]) with the epilogue applied (runtime.hip).
int launch_splitk_reduce(const EpiParams& pe, int splits, hipStream_t s);

// The tail of every entry point: launch() is the engine's kernel launch for plan p.
template <class F>
int run_gemm(const GemmPlan& p, const EpiParams& pe, int tag, hipStream_t s, F&& launch) {
  set_launch_tag(tag);
  ProfScope prof(VQA_K_GEMM, s);
  int rc = launch();
  if (rc == 0 && p.splits > 1) rc = launch_splitk_reduce(pe, p.splits, s);
  return rc;
}

}  // namespace vqa
