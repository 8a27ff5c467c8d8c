// bf16 convolution entry points (BASELINE configs[3]); kernels in conv_bf16.inc, shared device code in conv_device.inc.
#include "bf16_core.hpp"

namespace vqa {

#include "conv_device.inc"
#include "conv_host.inc"
#include "conv_bf16.inc"

using Cfg128 = TileCfg<128, 128, 2, 2>;
using Cfg128x64 = TileCfg<128, 64, 2, 2>;
// 256-row tiles (8 MFMA waves + 4 loader waves, one workgroup per CU): a third fewer staged bytes per MFMA than two
// 128x128 workgroups -- on bf16 MFMA the kernels are bound by exactly those bytes (VQA_BIG_TILES=1 selects them)
using Cfg256x128 = TileCfg<256, 128, 4, 2, 4, 2>;
using Cfg256x64 = TileCfg<256, 64, 4, 2, 4, 2>;
#ifndef VQA_BF16_FWD_PF
#define VQA_BF16_FWD_PF 2
#endif
using Cfg128x64L8 = TileCfg<128, 64, 2, 2, 8, 2>;   // 8 loader waves: the bf16 routing (2.5 VALU per element) is the long pole of dgrad
using Cfg128F = TileCfg<128, 128, 2, 2, 4, VQA_BF16_FWD_PF>;     // forward: plain copies, a third ring slot fits the registers

// ------------------------------------------------------------------ bf16 path launchers (conv_bf16.inc)
using CfgWb = TileCfg<128, 128, 2, 2, 4, 2>;      // bf16 wgrad: both operands through the transpose-read image

template <class Cfg, bool OB>
static int launch_fwd_bf16(const void* x, const void* wfT, const float* bias, void* pooled, uint8_t* amax,
                           const ConvGeom& g, hipStream_t s) {
  using SL = SmemLayoutB<Cfg, true, true>;
  const int nWin = g.B * g.Hp * g.Wp, Kdw = 9 * g.CiP / 2;
  typename ConvFwdA<Cfg::NVA, Cfg::LT, true>::Params pa{static_cast<const float*>(x), g.H, g.W, g.CiP / 2, g.Hp, g.Wp,
                                                         g.stride, nWin, Kdw};
  typename PlainR<Cfg::NVB, Cfg::LT>::Params pb{static_cast<const float*>(wfT), Kdw, g.Co, Kdw};
  const int tiles_m = (4 * nWin + Cfg::BM - 1) / Cfg::BM, tiles_n = (g.Co + Cfg::BN - 1) / Cfg::BN;
  return launch_kernel(conv_fwd_bf16_kernel<Cfg, OB>, {"attr(conv_fwd_bf16)", "conv_fwd_bf16 launch"}, tiles_m * tiles_n,
                       Cfg::THREADS, SL::BYTES, s, pa, pb, bias, pooled, amax, g.Co, tiles_m, tiles_n, Kdw / BK);
}

template <class Cfg, bool OB>
static int launch_dgrad_bf16(const void* dp, const uint8_t* am, const void* wdT, void* dx, const ConvGeom& g,
                             hipStream_t s) {
  using SL = SmemLayoutB<Cfg, true, true>;
  const int rows = g.B * g.H * g.W, Kdw = 9 * g.Co / 2;
  typename ConvDgradAb<Cfg::NVA, Cfg::LT>::Params pa{dp, am, g.H, g.W, g.Hp, g.Wp, g.Co, g.stride, rows};
  typename PlainR<Cfg::NVB, Cfg::LT>::Params pb{static_cast<const float*>(wdT), Kdw, g.CiP, Kdw};
  const int tiles_m = (rows + Cfg::BM - 1) / Cfg::BM, tiles_n = (g.CiP + Cfg::BN - 1) / Cfg::BN;
  return launch_kernel(conv_dgrad_bf16_kernel<Cfg, OB>, {"attr(conv_dgrad_bf16)", "conv_dgrad_bf16 launch"},
                       tiles_m * tiles_n, Cfg::THREADS, SL::BYTES, s, pa, pb, dx, g.CiP, tiles_m, tiles_n, Kdw / BK);
}

// bias_parts blocks of conv_bias_grad_bf16_kernel, bias_per pool windows each, write the partial bias rows
struct WgradPlanB : WgradPlan { int64_t bias_per; };
static WgradPlanB plan_wgrad_bf16(const ConvGeom& g) {
  WgradPlanB p{plan_splits(g, CfgWb::BM, CfgWb::BN, BKB, 512), 0};
  const int64_t windows = (int64_t)g.B * g.Hp * g.Wp;
  int64_t parts = (windows + 63) / 64;
  if (parts > 2048) parts = 2048;
  p.bias_per = (windows + parts - 1) / parts;
  p.bias_parts = (int)((windows + p.bias_per - 1) / p.bias_per);
  return p;
}

}  // namespace vqa

using namespace vqa;

extern "C" {

/* ---- bf16 path (BASELINE configs[3]) ------------------------------------------------------------------------ */
int vqa_conv_pack_weights_bf16(const float* w, void* wfT, void* wdT, int Co, int Ci, int CiP, vqa_stream_t stream) {
  VQA_REQUIRE(w && wfT && Ci <= CiP && CiP % 8 == 0, "vqa_conv_pack_weights_bf16: bad args Ci=%d CiP=%d", Ci, CiP);
  const int total = 9 * CiP * Co;
  hipLaunchKernelGGL(pack_weights_bf16_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, w,
                     static_cast<uint16_t*>(wfT), static_cast<uint16_t*>(wdT), Co, Ci, CiP);
  return check_hip(hipGetLastError(), "pack_weights_bf16 launch");
}

// what the bf16 kernels ask on top of check_geom, per launch
static int check_channels_bf16(const char* fn, const ConvGeom& g, int k_channels) {
  VQA_REQUIRE(k_channels % 64 == 0, "%s: the reduction-side channel count (%d) must be a multiple of 64", fn, k_channels);
  VQA_REQUIRE(g.CiP % 8 == 0 && g.Co % 8 == 0, "%s: channel counts must be multiples of 8 (CiP=%d Co=%d)", fn, g.CiP, g.Co);
  return VQA_OK;
}

int vqa_conv3x3_relu_pool_fwd_bf16(const void* x, const void* wfT, const float* bias, void* pooled, int pooled_is_bf16,
                                   uint8_t* argmax, int B, int H, int W, int CiP, int Co, int stride, int tag,
                                   vqa_stream_t stream) {
  VQA_REQUIRE(x && wfT && bias && pooled && argmax && B > 0, "vqa_conv3x3_relu_pool_fwd_bf16: null pointer");
  const ConvWalk w{"vqa_conv3x3_relu_pool_fwd_bf16", B, H, W, CiP, Co, stride, batch_chunk(B, H, W, CiP, Co, stride)};
  hipStream_t s = (hipStream_t)stream;
  return for_each_chunk(w, VQA_K_CONV_FWD, tag, s, [&](const ConvChunk& c) {
    int rc = check_channels_bf16(w.fn, c.g, CiP);
    if (rc) return rc;
    auto go = [&](auto cfg) {
      return with_flag(pooled_is_bf16, [&](auto ob) {
        return launch_fwd_bf16<decltype(cfg), decltype(ob)::value>(
            static_cast<const char*>(x) + c.xo * 2, wfT, bias, static_cast<char*>(pooled) + c.po * (pooled_is_bf16 ? 2 : 4),
            argmax + c.po, c.g, s);
      });
    };
    if (Co > 64 && knobs().big_tiles == 1) return go(Cfg256x128{});
    return Co > 64 ? go(Cfg128F{}) : go(Cfg128x64{});
  });
}

int vqa_conv3x3_dgrad_bf16(const void* dpooled, const uint8_t* argmax, const void* wdT, void* dx, int dx_is_bf16, int B,
                           int H, int W, int CiP, int Co, int stride, int tag, vqa_stream_t stream) {
  VQA_REQUIRE(dpooled && argmax && wdT && dx && B > 0, "vqa_conv3x3_dgrad_bf16: null pointer");
  const ConvWalk w{"vqa_conv3x3_dgrad_bf16", B, H, W, CiP, Co, stride, batch_chunk(B, H, W, CiP, Co, stride)};
  hipStream_t s = (hipStream_t)stream;
  return for_each_chunk(w, VQA_K_CONV_DGRAD, tag, s, [&](const ConvChunk& c) {
    int rc = check_channels_bf16(w.fn, c.g, Co);
    if (rc) return rc;
    auto go = [&](auto cfg) {
      return with_flag(dx_is_bf16, [&](auto ob) {
        return launch_dgrad_bf16<decltype(cfg), decltype(ob)::value>(
            static_cast<const char*>(dpooled) + c.po * 2, argmax + c.po, wdT,
            static_cast<char*>(dx) + c.xo * (dx_is_bf16 ? 2 : 4), c.g, s);
      });
    };
    const int bt = knobs().big_tiles;
    if (bt == 1) return CiP > 64 ? go(Cfg256x128{}) : go(Cfg256x64{});
    if (CiP > 64) return go(Cfg128{});
    return bt == 0 ? go(Cfg128x64{}) : go(Cfg128x64L8{});
  });
}

int64_t vqa_conv3x3_wgrad_bf16_workspace_bytes(int B, int H, int W, int CiP, int Co, int stride) {
  if (no_windows(B, H, W, stride)) return 0;
  const ConvWalk w{"vqa_conv3x3_wgrad_bf16", B, H, W, CiP, Co, stride, batch_chunk(B, H, W, CiP, Co, stride)};
  return slab_bytes(w, count_slabs(w, plan_wgrad_bf16));
}

int vqa_conv3x3_wgrad_bf16(const void* x, const void* dpooled, const uint8_t* argmax, float* dw, float* dbias, int B,
                           int H, int W, int CiP, int Ci, int Co, int stride, float* workspace,
                           int64_t workspace_bytes, int tag, vqa_stream_t stream) {
  VQA_REQUIRE(x && dpooled && argmax && dw && dbias && workspace && B > 0, "vqa_conv3x3_wgrad_bf16: null pointer");
  VQA_REQUIRE(Ci >= 1 && Ci <= CiP, "vqa_conv3x3_wgrad_bf16: Ci=%d CiP=%d", Ci, CiP);
  VQA_REQUIRE(Co % 8 == 0 && Co <= 2048, "vqa_conv3x3_wgrad_bf16: Co=%d must be a multiple of 8, at most 2048", Co);
  const ConvWalk w{"vqa_conv3x3_wgrad_bf16", B, H, W, CiP, Co, stride, batch_chunk(B, H, W, CiP, Co, stride)};
  hipStream_t s = (hipStream_t)stream;
  return wgrad_walk(
      w, plan_wgrad_bf16, 0, workspace, workspace_bytes, dw, Ci, tag, s,
      [&](const ConvChunk& c, const WgradPlanB& p, float* slab, float* bias_rows) {
        int rc = check_channels_bf16(w.fn, c.g, 64);
        if (rc) return rc;
        using SL = SmemLayoutB<CfgWb, false, false>;
        WgradGeom wg{c.g.H, c.g.W, c.g.CiP, c.g.Hp, c.g.Wp, c.g.Co, c.g.stride, p.Mtot};
        const char* dpc = static_cast<const char*>(dpooled) + c.po * 2;
        typename WgradAb<CfgWb::BM, CfgWb::LT>::Params pa{static_cast<const char*>(x) + c.xo * 2, wg, p.KI};
        typename WgradBb<CfgWb::BN, CfgWb::LT>::Params pb{dpc, argmax + c.po, wg};
        rc = launch_kernel(conv_wgrad_bf16_kernel<CfgWb>, {"attr(conv_wgrad_bf16)", "conv_wgrad_bf16 launch"},
                           p.tiles_m * p.tiles_n * p.splits, CfgWb::THREADS, SL::BYTES, s, pa, pb, slab, p.tiles_m,
                           p.tiles_n, p.nk, p.ks_per_split);
        if (rc) return rc;
        hipLaunchKernelGGL(conv_bias_grad_bf16_kernel, dim3(p.bias_parts), dim3(256), (size_t)(256 / (Co / 8)) * Co * 4, s,
                           reinterpret_cast<const uint16_t*>(dpc), argmax + c.po, bias_rows, (int64_t)c.g.B * c.g.Hp * c.g.Wp,
                           Co, p.bias_per);
        return check_hip(hipGetLastError(), "conv_bias_grad_bf16 launch");
      },
      [&](const float* bias_rows, int n) { return reduce_bias_rows(bias_rows, dbias, n, Co, s); });
}

}  // extern "C"
