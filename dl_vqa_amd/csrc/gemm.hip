// Generic fp32 MFMA GEMM (vqa_gemm): the planner, the two kernel templates and the C entry point.  The host rules it shares
// with vqa_gemm_x3 and vqa_gemm_bf16 are in gemm_host.hpp; the library's error / knob / profiling plumbing is in runtime.hip.
#include <stdlib.h>

#include "gemm_host.hpp"

// This file is compiled six times (dl_vqa_amd/build.py): VQA_GEMM_PART = 0 is the planner + the C ABI, parts 1-5 hold the
// kernels (1: 64x64 tiles; 2, 3: 128x128 tiles with A stored [M][K] / [K][M]; 4, 5: the same for 256x128) -- the fused
// epilogue's straight-line variants make a single translation unit with all of them take seven minutes to compile.
#ifndef VQA_GEMM_PART
#define VQA_GEMM_PART 0
#endif

namespace vqa {

using Cfg128 = TileCfg<128, 128, 2, 2>;
using Cfg256 = TileCfg<256, 128, 4, 2>;
using Cfg64 = TileCfg<64, 64, 2, 2>;

// Part 0 sees this declaration only; the definition and its kernels are compiled by the part that owns (Cfg, AL, BL).
template <class Cfg, class AL, class BL>
int launch_gemm(const typename AL::Params& pa, const typename BL::Params& pb, const EpiParams& pe, const GemmPlan& p, int K,
                hipStream_t s);

#if VQA_GEMM_PART != 0
// gemm_kernel, gemm_bf16_kernel (bf16.hip) and gemm_x3_kernel (gemm_x3.hip) open and close alike (tile coordinate, K range,
// slab store or epilogue) around different main loops.  The three bodies stay spelled out: sharing the preamble would have
// to leave every instantiation's registers and instruction mix as they are, which this host-side change does not take on.
// Persistent variant (no split-K, single Raw set): min(tiles, resident slots) workgroups walk the tiles.
template <class Cfg, class AL, class BL>
__global__ __launch_bounds__(Cfg::THREADS, Cfg::MIN_WAVES) void gemm_persistent_kernel(
    typename AL::Params pa, typename BL::Params pb, EpiParams pe, int tiles_m, int tiles_n, int nk, int Ktot,
    int order) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / Cfg::WAVES_N, wn = wave % Cfg::WAVES_N;
  auto origin = [&](int t, int& m0, int& n0) {
    int mt, nt;
    if (order == 1) { nt = t / tiles_m; mt = t - nt * tiles_m; } else { mt = t / tiles_n; nt = t - mt * tiles_n; }
    m0 = mt * Cfg::BM; n0 = nt * Cfg::BN;
  };
  gemm_persistent<Cfg, AL, BL, false>(
      xcd_swizzle(blockIdx.x, gridDim.x), gridDim.x, tiles_m * tiles_n, nk, Ktot, smem,
      [&](int t, AL& al, BL& bl) {
        int m0, n0;
        origin(t, m0, n0);
        al.init(pa, m0, loader_tid<Cfg>(), 0);
        bl.init(pb, n0, loader_tid<Cfg>(), 0);
      },
      [&](int t, f32x16 (&acc)[Cfg::TM][Cfg::TN]) {
        int m0, n0;
        origin(t, m0, n0);
        gemm_epilogue<Cfg>(pe, acc, m0, n0, wm, wn, lane);
      }
#ifdef VQA_DIAG
      , pe.bar_dbg
#endif
      );
}

template <class Cfg, class AL, class BL>
__global__ __launch_bounds__(Cfg::THREADS, Cfg::MIN_WAVES) void gemm_kernel(typename AL::Params pa, typename BL::Params pb,
                                                   EpiParams pe, int tiles_m, int tiles_n, int nk,
                                                   int ks_per_split, int Ktot, int order, int splits) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / Cfg::WAVES_N, wn = wave % Cfg::WAVES_N;
  const TileCoord tc = tile_coord(tiles_m, tiles_n, order, splits);
  const int m0 = tc.mt * Cfg::BM, n0 = tc.nt * Cfg::BN;
  const int split = tc.split;
  const int ks0 = split * ks_per_split;
  const int ks1 = min(nk, ks0 + ks_per_split);
  f32x16 acc[Cfg::TM][Cfg::TN];
  acc_zero<Cfg>(acc);
  if (!gemm_mainloop<Cfg, AL, BL>(
          [&](AL& al, BL& bl) {
            al.init(pa, m0, loader_tid<Cfg>(), ks0);
            bl.init(pb, n0, loader_tid<Cfg>(), ks0);
          },
          [](AL&, BL&) {}, acc, ks0, ks1, Ktot, smem))
    return;

  float* slab = pe.slab ? pe.slab + (int64_t)split * pe.M * pe.N : nullptr;
  if (slab) {
    store_acc_tiles<Cfg>(acc, slab, pe.N, pe.M, pe.N, m0, n0, wm, wn, lane);
    return;
  }
  gemm_epilogue<Cfg>(pe, acc, m0, n0, wm, wn, lane);
}

template <class Cfg, class AL, class BL>
int launch_gemm(const typename AL::Params& pa, const typename BL::Params& pb, const EpiParams& pe, const GemmPlan& p, int K,
                hipStream_t s) {
  using SL = SmemLayout<Cfg, AL::kTypeR, BL::kTypeR>;
  if constexpr (Cfg::BM * Cfg::BN > 64 * 64) {
    // Persistent tiles pay when K is short (<= 16 K-steps: dispatch + prologue + epilogue are then a large
    // share of a tile's life: v_conv forward 1.13 -> 1.04 ms, LSTM input GEMM 0.116 -> 0.105 ms); with long K
    // the static tile striding loses more to imbalance than it saves (v_conv dgrad 0.82 -> 0.88 ms), so those
    // keep one workgroup per tile and the hardware's dynamic dispatch.  VQA_PERSISTENT=0/1 forces the choice.
    if (gemm_runs_persistent(p)) {
      auto pk = gemm_persistent_kernel<Cfg, AL, BL>;
      int rc = ensure_dyn_smem(reinterpret_cast<const void*>(pk), SL::BYTES, "hipFuncSetAttribute(gemm_persistent)");
      if (rc) return rc;
      // resident slots from the occupancy the runtime reports for THIS kernel (registers, scratch and LDS as compiled), not
      // from the LDS layout alone: a variant that needs more registers than planned then gets a smaller grid instead of a
      // second, queued round of workgroups.  (No workgroup ever waits for another one, so co-residency is a matter of
      // speed here, never of progress.)
      const int slots = persistent_slots(reinterpret_cast<const void*>(pk), Cfg::THREADS, SL::BYTES, SL::WG_PER_CU);
      if (slots <= 0) return VQA_ERR_HIP;
      const int tiles = p.tiles_m * p.tiles_n;
      hipLaunchKernelGGL(pk, dim3(tiles < slots ? tiles : slots), dim3(Cfg::THREADS), SL::BYTES, s, pa, pb, pe,
                         p.tiles_m, p.tiles_n, p.nk, K, p.order);
      return check_hip(hipGetLastError(), "gemm_persistent_kernel launch");
    }
  }
  auto kern = gemm_kernel<Cfg, AL, BL>;
  {
    int rc = ensure_dyn_smem(reinterpret_cast<const void*>(kern), SL::BYTES, "hipFuncSetAttribute(gemm)");
    if (rc) return rc;
  }
  dim3 grid(p.tiles_m * p.tiles_n * p.splits);
  hipLaunchKernelGGL(kern, grid, dim3(Cfg::THREADS), SL::BYTES, s, pa, pb, pe, p.tiles_m, p.tiles_n, p.nk,
                     p.ks_per_split, K, p.order, p.splits);
  return check_hip(hipGetLastError(), "gemm_kernel launch");
}

#define VQA_GEMM_OWN(CFG, AL, BL)                                                                                     \
  template int launch_gemm<CFG, AL<CFG::NVA, CFG::LT>, BL<CFG::NVB, CFG::LT>>(                                         \
      const typename AL<CFG::NVA, CFG::LT>::Params&, const typename BL<CFG::NVB, CFG::LT>::Params&, const EpiParams&, \
      const GemmPlan&, int, hipStream_t);
#if VQA_GEMM_PART == 1
VQA_GEMM_OWN(Cfg64, PlainR, PlainR) VQA_GEMM_OWN(Cfg64, PlainR, PlainC) VQA_GEMM_OWN(Cfg64, PlainC, PlainR) VQA_GEMM_OWN(Cfg64, PlainC, PlainC)
#elif VQA_GEMM_PART == 2
VQA_GEMM_OWN(Cfg128, PlainR, PlainR) VQA_GEMM_OWN(Cfg128, PlainR, PlainC)
#elif VQA_GEMM_PART == 3
VQA_GEMM_OWN(Cfg128, PlainC, PlainR) VQA_GEMM_OWN(Cfg128, PlainC, PlainC)
#elif VQA_GEMM_PART == 4
VQA_GEMM_OWN(Cfg256, PlainR, PlainR) VQA_GEMM_OWN(Cfg256, PlainR, PlainC)
#elif VQA_GEMM_PART == 5
VQA_GEMM_OWN(Cfg256, PlainC, PlainR) VQA_GEMM_OWN(Cfg256, PlainC, PlainC)
#endif

}  // namespace vqa

#else  // VQA_GEMM_PART == 0: the planner and the C entry point
GemmPlan plan_gemm(int M, int N, int K, int bk) {
  GemmPlan p;
  const int nk = (K + bk - 1) / bk;
  const int t128 = ((M + 127) / 128) * ((N + 127) / 128);
  const int t64 = ((M + 63) / 64) * ((N + 63) / 64);
  int splits = 1;
  // Two workgroups fit a CU: 512 resident slots.  A launch that fills them exactly keeps two MFMA waves on
  // every SIMD (one covers the other's barriers); 384 workgroups left a quarter of the slots empty
  // (v_conv dW 0.90 -> 0.72 ms with 24 -> 32 splits), more than 512 would run a second, nearly empty round.
  const Knobs& kn = knobs();
  const int target = kn.split_target > 0 ? kn.split_target : 512;
  if (t128 >= 200) {
    p.big = 1;
    // 200..511 big tiles with a long K: two splits double the resident workgroups (LSTM dW_hh: 256 tiles)
    if (t128 * 2 <= target && nk >= 64) splits = target / t128;
  } else if (t64 >= 200) p.big = 0;
  else {
    // few big tiles + many splits = short K loops dominated by prologue/epilogue (LSTM dh GEMM, M = 256:
    // 16 tiles x 24 splits of 6 K-steps ran at 21 % of peak): below 64 big tiles use 64x64 tiles, whose
    // 4x larger tile count needs 4x fewer splits
    // ... unless K is long enough that every split of the big tiling still runs >= 16 K-steps
    // (v_conv dW: K = B*P = 173k -> 16 tiles x 32 splits x 169 K-steps)
    const int big_splits = target / t128 > 1 ? target / t128 : 1;
    p.big = (M >= 128 && N >= 128 && (t128 >= 64 || nk / big_splits >= 16)) ? 1 : 0;
    const int tiles = p.big ? t128 : t64;
    const int max_splits = nk / 4 > 1 ? nk / 4 : 1;
    splits = target / tiles > 1 ? target / tiles : 1;
    if (splits > max_splits) splits = max_splits;
    if (splits > 64) splits = 64;
  }
  // 256x128 tiles (8 MFMA waves, as the conv forward) measured 4-8 % SLOWER on the tall plain GEMMs
  // (v_conv fwd 1.29 vs 1.24 ms, dgrad 0.94 vs 0.87 ms): opt-in only (VQA_BIG_TILES=2)
  if (p.big && splits == 1 && kn.big_tiles == 2) p.big = 2;
  const int bm = p.big == 2 ? 256 : (p.big ? 128 : 64), bn = p.big ? 128 : 64;
  p.tiles_m = (M + bm - 1) / bm;
  p.tiles_n = (N + bn - 1) / bn;
  p.nk = nk;
  split_k(p, splits);
  // skinny GEMM with a big B operand: keep each XCD on its own column slice of B (tile_coord order 1)
  p.order = (p.tiles_m <= 8 && p.tiles_n >= 16 && kn.weight_stationary != 0) ? 1 : 0;
  return p;
}

// vqa_gemm_bf16's long-K weight gradient with a 256-column output (v_conv dW): 128 x 256 tiles, one workgroup per CU, split-K
// over the 256 slots.  The caller sizes its workspace by vqa_gemm_bf16_workspace_bytes, which reports the ORDINARY plan's
// slabs; this plan is admitted only where that workspace happens to hold its slabs as well (it does for the shapes of the
// train step, a coincidence of the two split counts), else the ordinary plan runs.  VQA_GEMM_WIDE=0 switches it off.
bool plan_gemm_wide(GemmPlan& p, int M, int N, int K, int transA, int transB, bool has_workspace, int64_t workspace_bytes) {
  static const int wide_ok = [] { const char* e = getenv("VQA_GEMM_WIDE"); return e && atoi(e) == 0 ? 0 : 1; }();
  if (!(wide_ok && transA && !transB && N == 256 && M % 128 == 0 && K >= (1 << 16) && has_workspace)) return false;
  GemmPlan q{1, M / 128, 1, p.nk, 0, 0, 0};
  const int splits = 256 / q.tiles_m;
  split_k(q, splits < 1 ? 1 : splits > 64 ? 64 : splits);
  if (workspace_bytes < (int64_t)q.splits * M * N * 4) return false;
  p = q;
  return true;
}

template <class Cfg>
int dispatch_gemm(const float* A, int64_t lda, int transA, const float* B, int64_t ldb, int transB,
                  const EpiParams& pe, const GemmPlan& p, int M, int N, int K, hipStream_t s) {
  return with_layout<PlainR<Cfg::NVA, Cfg::LT>, PlainC<Cfg::NVA, Cfg::LT>, PlainR<Cfg::NVB, Cfg::LT>, PlainC<Cfg::NVB, Cfg::LT>>(
      transA, transB, [&](auto al, auto bl) {
        return launch_gemm<Cfg, typename decltype(al)::type, typename decltype(bl)::type>({A, lda, M, K}, {B, ldb, N, K}, pe, p, K, s);
      });
}

#ifdef VQA_DIAG
extern unsigned long long* g_bar_dbg;   // runtime.hip: vqa_diag_barrier_buffer
#endif

}  // namespace vqa

using namespace vqa;

extern "C" {

int64_t vqa_gemm_workspace_bytes(int M, int N, int K) { return slab_bytes(plan_gemm(M, N, K), M, N); }

int vqa_gemm(const float* A, int64_t lda, int transA, const float* B, int64_t ldb, int transB, float* C,
             int64_t ldc, int M, int N, int K, const float* bias1, const float* bias2,
             const float* rowgroup, int64_t rg_ld, int rg_div, int rg_op, int relu, int accumulate,
             float* aux, float* workspace, int64_t workspace_bytes, int tag, vqa_stream_t stream) {
  if (int rc = check_gemm_args("vqa_gemm", 4, A, lda, B, ldb, C, ldc, M, N, K, rowgroup, rg_div)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const GemmPlan p = plan_gemm(M, N, K);
  EpiParams pe = epi_params(C, nullptr, ldc, M, N, bias1, bias2, rowgroup, rg_ld, rg_div, rg_op, relu, accumulate, aux);
#ifdef VQA_DIAG
  pe.bar_dbg = g_bar_dbg;
#endif
#ifdef VQA_EXP_EPI_DROPOUT
  {   // reconstruction of the withdrawn experiment: every row-group GEMM with ReLU drops 30 % in its epilogue
    const bool on = rowgroup != nullptr && relu;
    pe.drop_p = on ? 0.3f : 0.f; pe.drop_inv = 1.0f / 0.7f; pe.drop_seed = 0x1234567887654321ull;
  }
#endif
  if (int rc = claim_slab("vqa_gemm", p, pe, workspace, workspace_bytes)) return rc;
  return run_gemm(p, pe, tag, s, [&] {
    return p.big == 2 ? dispatch_gemm<Cfg256>(A, lda, transA, B, ldb, transB, pe, p, M, N, K, s)
           : p.big  ? dispatch_gemm<Cfg128>(A, lda, transA, B, ldb, transB, pe, p, M, N, K, s)
                    : dispatch_gemm<Cfg64>(A, lda, transA, B, ldb, transB, pe, p, M, N, K, s);
  });
}

}  // extern "C"
#endif  // VQA_GEMM_PART
