// Image encoder kernels: Conv2d(3x3, stride, pad 0) + ReLU + MaxPool2d(2,2), forward / dgrad / wgrad,
// as implicit GEMMs on the fp32 MFMA engine (gemm_core.hpp).
//
// Reference: models/model.py:72-84 (ImageNet2).  Layout: NHWC, channels padded to a multiple of 4.
//
// forward   M = 4 * (#pool windows): row m = 4*w + j is conv-output pixel j = dy*2+dx of pool window
//           w = (b, py, px).  In the MFMA C layout a lane holds rows (r&3) + 8*(r>>2) + 4*(lane>>5)
//           of one column, i.e. the four pixels of a window sit in four consecutive accumulator
//           registers of ONE lane: bias + ReLU + 2x2 max + arg-max are register-only, and the
//           pre-pool activation (3.2 GB for conv0 at B = 256) never exists in memory.
//           K = 9*CiP ordered (ky, kx, ci): the A "row" of a pixel for one tap is CiP contiguous floats.
// dgrad     rows = conv-INPUT pixels, K = (ky, kx, co); the A loader rebuilds dY on the fly from the
//           pooled gradient and the stored arg-max byte (one non-zero per 2x2 window).
// wgrad     out[(ky,kx,ci)][co] = sum over conv-output pixels; split along that (huge) reduction over
//           workgroups into slabs, then reduced and transposed to the torch layout [Co][Ci][3][3].
#include "bf16_core.hpp"

namespace vqa {

#include "conv_device.inc"
#include "conv_host.inc"

using Cfg128 = TileCfg<128, 128, 2, 2>;
using Cfg128x64 = TileCfg<128, 64, 2, 2>;
// 256-row tiles for the pixel-major GEMMs (forward / dgrad: M = millions of pixels): 25 % fewer bytes
// staged per MFMA than 128x128 (tools/mfma_ws.hip: 83 % -> 88 % of the MFMA rate in the same skeleton).
#ifndef VQA_BIG_PF
#define VQA_BIG_PF 0
#endif
using Cfg256x128 = TileCfg<256, 128, 4, 2, 4, VQA_BIG_PF>;   // 8 MFMA waves (64x64 each) + 4 loader waves, one workgroup per CU
using Cfg256x64 = TileCfg<256, 64, 4, 2, 4, VQA_BIG_PF>;     // 8 MFMA waves (64x32 each)
using Cfg64 = TileCfg<64, 64, 2, 2>;
// wgrad rows are (tap, ci): 9*CiP = 576 for CiP = 64 is 4.5 x 128 but 6 x 96 (1 x 4 MFMA waves of 96x32)
#ifndef VQA_WGRAD_PF
#define VQA_WGRAD_PF 3
#endif
using Cfg96x128 = TileCfg<96, 128, 1, 4, 4, VQA_WGRAD_PF>;
// wgrad streams new pixels from HBM every K-step: three K-steps of loads in flight (75 -> 78 % on conv1 in spite
// of ~55 spilled loader registers; four spill 100+ and lose 15 points; dgrad's 128x64 tile loses 9 points at three)
using Cfg128W = TileCfg<128, 128, 2, 2, 4, VQA_WGRAD_PF>;
#ifndef VQA_W192_PF
#define VQA_W192_PF 3
#endif
// 192 rows, 8 MFMA waves (2 x 4, 96x32 each) + 4 loader waves, one workgroup per CU (84 KB LDS, 164 VGPRs): the routed
// B operand is reloaded by 3 (conv1) / 6 (conv2) row tiles instead of 6 / 9 (see plan_wgrad for when it is used)
using Cfg192x128W = TileCfg<192, 128, 2, 4, 4, VQA_W192_PF>;
using Cfg384x128W = TileCfg<384, 128, 4, 2, 4, 2>;   // 9*CiP = 1152 as three row tiles (see plan_wgrad)
// the same tiles with 8 loader waves (1024 threads): two loader waves per SIMD for loader-bound K loops
using Cfg256x128L8 = TileCfg<256, 128, 4, 2, 8>;
using Cfg256x64L8 = TileCfg<256, 64, 4, 2, 8>;
// dgrad with CiP <= 64 (conv1): a K-step is only 32 MFMAs per wave, so the loaders are the long pole; with 8
// loader waves (768 threads, 74 VGPRs: two workgroups = 6 waves per SIMD) 70.6 -> 73.0 % on the same box
#ifndef VQA_DGRAD_PF
#define VQA_DGRAD_PF 2
#endif
using Cfg128x64L8 = TileCfg<128, 64, 2, 2, 8, VQA_DGRAD_PF>;

template <class Cfg, bool U>
static int launch_fwd(const float* x, const float* wf, const float* bias, float* pooled, uint8_t* amax,
                      const ConvGeom& g, hipStream_t s) {
  using SL = SmemLayout<Cfg, true, false>;
  const int nWin = g.B * g.Hp * g.Wp, K = 9 * g.CiP;
  typename ConvFwdA<Cfg::NVA, Cfg::LT, U>::Params pa{x, g.H, g.W, g.CiP, g.Hp, g.Wp, g.stride, nWin, K};
  typename PlainC<Cfg::NVB, Cfg::LT>::Params pb{wf, g.Co, g.Co, K};
  const int tiles_m = (4 * nWin + Cfg::BM - 1) / Cfg::BM, tiles_n = (g.Co + Cfg::BN - 1) / Cfg::BN;
  const int slots = 256 * SL::WG_PER_CU, tiles = tiles_m * tiles_n;
  // Persistent tiles measured neutral to slower on the conv kernels (conv1 fwd 3.83 -> 3.81 ms, conv2 dgrad
  // 3.65 -> 3.93 ms: their K loops are long and the second workgroup / MFMA wave of the SIMD already covers a
  // tile's prologue and epilogue), so they are opt-in (VQA_PERSISTENT=1) and parity-tested that way.
  return launch_tiles(knobs().persistent == 1, conv_fwd_persistent_kernel<Cfg, U>,
                      {"attr(conv_fwd_p)", "conv_fwd_persistent launch"}, tiles < slots ? tiles : slots,
                      conv_fwd_kernel<Cfg, U>, {"attr(conv_fwd)", "conv_fwd launch"}, tiles, Cfg::THREADS, SL::BYTES, s, pa,
                      pb, bias, pooled, amax, g.Co, tiles_m, tiles_n, (K + BK - 1) / BK);
}

template <class Cfg, bool U>
static int launch_dgrad(const float* dp, const uint8_t* am, const float* wd, float* dx, const ConvGeom& g,
                        hipStream_t s) {
  using SL = SmemLayout<Cfg, true, false>;
  const int rows = g.B * g.H * g.W, K = 9 * g.Co;
  typename ConvDgradA<Cfg::NVA, Cfg::LT, U>::Params pa{dp, am, g.H, g.W, g.Hp, g.Wp, g.Co, g.stride, rows, K};
  typename PlainC<Cfg::NVB, Cfg::LT>::Params pb{wd, g.CiP, g.CiP, K};
  const int tiles_m = (rows + Cfg::BM - 1) / Cfg::BM, tiles_n = (g.CiP + Cfg::BN - 1) / Cfg::BN;
  const int slots = 256 * SL::WG_PER_CU, tiles = tiles_m * tiles_n;
  return launch_tiles(knobs().persistent == 1 /* see launch_fwd */, conv_dgrad_persistent_kernel<Cfg, U>,
                      {"attr(conv_dgrad_p)", "conv_dgrad_persistent launch"}, tiles < slots ? tiles : slots,
                      conv_dgrad_kernel<Cfg, U>, {"attr(conv_dgrad)", "conv_dgrad launch"}, tiles, Cfg::THREADS, SL::BYTES,
                      s, pa, pb, dx, g.CiP, tiles_m, tiles_n, (K + BK - 1) / BK);
}

struct WgradPlanF : WgradPlan { int big, bm; };
static WgradPlanF plan_wgrad(const ConvGeom& g) {
  const int KI = 9 * g.CiP;
  const int big = (KI >= 128 && g.Co >= 128) ? 1 : 0;
  // 96-row tiles when they waste fewer rows than 128-row tiles (KI = 576: 576 vs 640 rows of MFMA work)
  int bm = !big ? 64 : ((KI + 95) / 96 * 96 < (KI + 127) / 128 * 128 ? 96 : 128);
  // 9*CiP = 576 (CiP = 64): three 192-row tiles (8 MFMA waves, one workgroup per CU) instead of six 96-row tiles halve
  // the reloads of the routed B operand: 76.6 -> 80.3 % with the early K-step barrier (before it: +1 point); where
  // 128-row tiles fit exactly (9*CiP = 1152) two 128x128 workgroups per CU stay ahead (83.0 vs 79.4 %).
  // VQA_WGRAD_192=0 / 1 disables / forces it wherever 9*CiP % 192 == 0.
  {
    const int w192 = knobs().wgrad_192, w384 = knobs().wgrad_384;
    const bool can = big && KI % 192 == 0 && g.CiP % BK == 0 && g.Co % BK == 0 && 2 * g.Wp >= BK;
    if (can && (w192 >= 0 ? w192 == 1 : bm == 96)) bm = 192;
    // 9*CiP = 1152 (CiP = 128): three 384-row tiles (8 MFMA waves of 96x64, one workgroup per CU, 133 KB LDS) reload
    // the routed B operand 3x instead of 9x: 82.4 -> 86.6 % (same box).  VQA_WGRAD_384=0 / 1 disables / forces it.
    if (can && KI % 384 == 0 && w192 != 1 && (w384 >= 0 ? w384 == 1 : true)) bm = 384;
  }
  // 2 workgroups fit a CU (LDS): tiles * splits must not exceed the 512 resident slots, or the few
  // workgroups left over run alone in a second round and double the kernel's time.
  WgradPlanF p{plan_splits(g, bm, big ? 128 : 64, BK, bm >= 192 ? 256 : 512), big, bm};
  p.bias_parts = p.splits;      // the MFMA waves sum the bias: one partial row per split
  return p;
}

template <class Cfg, bool U>
static int launch_wgrad(const float* x, const float* dp, const uint8_t* am, float* slab, float* bias_slab,
                        const ConvGeom& g, const WgradPlan& p, hipStream_t s) {
  using SL = SmemLayout<Cfg, false, false>;
  WgradGeom wg{g.H, g.W, g.CiP, g.Hp, g.Wp, g.Co, g.stride, p.Mtot};
  typename WgradA<Cfg::NVA, Cfg::LT, U>::Params pa{x, wg, p.KI};
  typename WgradB<Cfg::NVB, Cfg::LT, U>::Params pb{dp, am, wg};
  return launch_kernel(conv_wgrad_kernel<Cfg, U>, {"attr(conv_wgrad)", "conv_wgrad launch"},
                       p.tiles_m * p.tiles_n * p.splits, Cfg::THREADS, SL::BYTES, s, pa, pb, slab, bias_slab, p.tiles_m,
                       p.tiles_n, p.nk, p.ks_per_split);
}

}  // namespace vqa

using namespace vqa;

extern "C" {

int vqa_nchw_to_nhwc4(const float* x, float* y, int B, int C, int H, int W, vqa_stream_t stream) {
  VQA_REQUIRE(x && y && C >= 1 && C <= 4, "vqa_nchw_to_nhwc4: C=%d must be 1..4", C);
  const int64_t HW = (int64_t)H * W, total = (int64_t)B * HW;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(nchw_to_nhwc4_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, C, HW, total);
  return check_hip(hipGetLastError(), "nchw_to_nhwc4 launch");
}

int vqa_conv_pack_weights(const float* w, float* wf, float* wd, int Co, int Ci, int CiP, vqa_stream_t stream) {
  VQA_REQUIRE(w && wf && Ci <= CiP && CiP % 4 == 0, "vqa_conv_pack_weights: bad args Ci=%d CiP=%d", Ci, CiP);
  const int total = 9 * CiP * Co;
  hipLaunchKernelGGL(pack_weights_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, wf, wd,
                     Co, Ci, CiP);
  return check_hip(hipGetLastError(), "pack_weights launch");
}

int vqa_conv3x3_relu_pool_fwd(const float* x, const float* wf, const float* bias, float* pooled, uint8_t* argmax,
                              int B, int H, int W, int CiP, int Co, int stride, int tag, vqa_stream_t stream) {
  VQA_REQUIRE(x && wf && bias && pooled && argmax && B > 0, "vqa_conv3x3_relu_pool_fwd: null pointer");
  const ConvWalk w{"vqa_conv3x3_relu_pool_fwd", B, H, W, CiP, Co, stride, batch_chunk(B, H, W, CiP, Co, stride)};
  hipStream_t s = (hipStream_t)stream;
  return for_each_chunk(w, VQA_K_CONV_FWD, tag, s, [&](const ConvChunk& c) {
    auto go = [&](auto cfg, auto uni) {
      return launch_fwd<decltype(cfg), decltype(uni)::value>(x + c.xo, wf, bias, pooled + c.po, argmax + c.po, c.g, s);
    };
    // Two 128x128 workgroups per CU beat one 256x128 workgroup (8 MFMA + 4 or 8 loader waves) since the loaders
    // left the VALU: conv1 / conv2 forward 84.4 / 88.3 % against 82.7 / 84.7 % (4 loader waves) and 83.6 / 85.2 %
    // (8); on dgrad the gap is wider (72 / 81 % against 56 / 70 % and 66 / 75 %).  The 256-row kernels stay
    // selectable with VQA_BIG_TILES=1 (4 loader waves) / 3 (8) and are parity-tested that way.
    const int bt = knobs().big_tiles;
    // channel counts that are not multiples of BK take the general per-lane-tap loaders (one tile shape)
    if (CiP % BK != 0) return go(Cfg128x64{}, Flag<false>{});
    if (bt == 3 && Co > 64) return go(Cfg256x128L8{}, Flag<true>{});
    if (Co > 64) return bt == 1 ? go(Cfg256x128{}, Flag<true>{}) : go(Cfg128{}, Flag<true>{});
    return go(Cfg128x64{}, Flag<true>{});
  });
}

int vqa_conv3x3_dgrad(const float* dpooled, const uint8_t* argmax, const float* wd, float* dx, int B, int H, int W,
                      int CiP, int Co, int stride, int tag, vqa_stream_t stream) {
  VQA_REQUIRE(dpooled && argmax && wd && dx && B > 0, "vqa_conv3x3_dgrad: null pointer");
  const ConvWalk w{"vqa_conv3x3_dgrad", B, H, W, CiP, Co, stride, batch_chunk(B, H, W, CiP, Co, stride)};
  hipStream_t s = (hipStream_t)stream;
  return for_each_chunk(w, VQA_K_CONV_DGRAD, tag, s, [&](const ConvChunk& c) {
    auto go = [&](auto cfg, auto uni) {
      return launch_dgrad<decltype(cfg), decltype(uni)::value>(dpooled + c.po, argmax + c.po, wd, dx + c.xo, c.g, s);
    };
    const int bt = knobs().big_tiles;      // 256-row tiles are opt-in only, see vqa_conv3x3_relu_pool_fwd
    if (Co % BK != 0) return go(Cfg128x64{}, Flag<false>{});
    if (bt == 3) return CiP > 64 ? go(Cfg256x128L8{}, Flag<true>{}) : go(Cfg256x64L8{}, Flag<true>{});
    if (CiP > 64) return bt == 1 ? go(Cfg256x128{}, Flag<true>{}) : go(Cfg128{}, Flag<true>{});
    if (bt == 0) return go(Cfg128x64{}, Flag<true>{});
    return bt == 1 ? go(Cfg256x64{}, Flag<true>{}) : go(Cfg128x64L8{}, Flag<true>{});
  });
}

int64_t vqa_conv3x3_wgrad_workspace_bytes(int B, int H, int W, int CiP, int Co, int stride) {
  if (no_windows(B, H, W, stride)) return 0;
  const ConvWalk w{"vqa_conv3x3_wgrad", B, H, W, CiP, Co, stride, batch_chunk(B, H, W, CiP, Co, stride)};
  // one [9*CiP][Co] slab and one partial bias row per split of every chunk
  return slab_bytes(w, count_slabs(w, plan_wgrad));
}

int vqa_conv3x3_wgrad(const float* x, const float* dpooled, const uint8_t* argmax, float* dw, float* dbias, int B,
                      int H, int W, int CiP, int Ci, int Co, int stride, float* workspace, int64_t workspace_bytes,
                      int tag, vqa_stream_t stream) {
  VQA_REQUIRE(x && dpooled && argmax && dw && dbias && workspace && B > 0, "vqa_conv3x3_wgrad: null pointer");
  VQA_REQUIRE(Ci >= 1 && Ci <= CiP, "vqa_conv3x3_wgrad: Ci=%d CiP=%d", Ci, CiP);
  const ConvWalk w{"vqa_conv3x3_wgrad", B, H, W, CiP, Co, stride, batch_chunk(B, H, W, CiP, Co, stride)};
  hipStream_t s = (hipStream_t)stream;
  return wgrad_walk(
      w, plan_wgrad, 0, workspace, workspace_bytes, dw, Ci, tag, s,
      [&](const ConvChunk& c, const WgradPlanF& p, float* slab, float* bias_slab) {
        auto go = [&](auto cfg, auto uni) {
          return launch_wgrad<decltype(cfg), decltype(uni)::value>(x + c.xo, dpooled + c.po, argmax + c.po, slab, bias_slab,
                                                                   c.g, p, s);
        };
        auto go_uni = [&](auto cfg) {
          return with_flag(CiP % BK == 0 && Co % BK == 0 && 2 * c.g.Wp >= BK, [&](auto uni) { return go(cfg, uni); });
        };
        // (8 loader waves on the 192-row tile: +0.5 %, with 3 or 4 K-steps in flight alike; not worth the kernels)
        return p.bm == 384   ? go(Cfg384x128W{}, Flag<true>{})
               : p.bm == 192 ? go(Cfg192x128W{}, Flag<true>{})
               : p.bm == 96  ? go_uni(Cfg96x128{})
               : p.big       ? go_uni(Cfg128W{})
                             : go_uni(Cfg64{});
      },
      [&](const float* bias_rows, int n) { return reduce_bias_rows(bias_rows, dbias, n, Co, s); });
}

}  // extern "C"

#ifdef VQA_DIAG
// diagnostic build only: read-and-reset the s_memtime sums of the conv kernels (this translation unit)
extern "C" int vqa_diag_read(unsigned long long* out8) {
  unsigned long long z[4] = {0, 0, 0, 0};
  hipDeviceSynchronize();
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(vqa::vqa_diag_buf), sizeof(z)) != hipSuccess) return 1;
  if (hipMemcpyFromSymbol(out8 + 4, HIP_SYMBOL(vqa::vqa_diag_ld), sizeof(z)) != hipSuccess) return 1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(vqa::vqa_diag_ld), z, sizeof(z)) != hipSuccess) return 1;
  return hipMemcpyToSymbol(HIP_SYMBOL(vqa::vqa_diag_buf), z, sizeof(z)) == hipSuccess ? 0 : 1;
}
#endif
