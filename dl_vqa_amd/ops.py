"""Tensor-level wrappers over the C ABI (one Python function per entry point of include/vqa_hip.h).

torch supplies device memory and the current HIP stream; every computation happens in the HIP
library.  Nothing here falls back to torch arithmetic.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import call, ptr, stream

_ws = {}


def workspace(nbytes: int, device) -> torch.Tensor:
    """A scratch buffer that only grows (split-K slabs, reduction partials), one per (device, stream):
    launch sequences that run concurrently on different HIP streams must not share slabs."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    t = _ws.get(key)
    if t is None or t.numel() * 4 < nbytes:
        t = torch.empty(_workspace_floats(nbytes), dtype=torch.float32, device=device)
        _ws[key] = t
    return t


def _workspace_floats(nbytes: int) -> int:
    """Elements of a workspace made for a claim of nbytes."""
    return max(nbytes // 4 + 1024, 1 << 20)


def _chk(t: torch.Tensor, dtype=torch.float32):
    assert t.is_cuda and t.dtype == dtype, (t.device, t.dtype)


def _ld(t: torch.Tensor) -> int:
    """The leading dimension of a row-major 2-D view with unit column stride: its row stride, or its width for a single row."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _cache_suffix(t: torch.Tensor) -> str:
    """The entry-point suffix for an image-feature cache operand (vn, v', a bank): fp32, or float16 read natively by the
    *_f16 entry points.  Every other operand of those calls stays fp32."""
    assert t.is_cuda and t.dtype in (torch.float32, torch.float16), (t.device, t.dtype)
    return "_f16" if t.dtype == torch.float16 else ""


def _gemm(name: str, c_kind: tuple, A, B, C, M, N, K, transA, transB, lda, ldb, ldc, bias1, bias2, rowgroup, rg_div, rg_op, relu,
          accumulate, aux, tag) -> torch.Tensor:
    """The call of vqa_gemm / vqa_gemm_x3 / vqa_gemm_bf16: leading dimensions default to the stored row length, the workspace
    is what the entry point's *_workspace_bytes asks for.  c_kind: the arguments between ldc and M (bf16: c_is_bf16)."""
    lib = _lib.load()
    lda = lda if lda is not None else (M if transA else K)
    ldb = ldb if ldb is not None else (K if transB else N)
    ldc = ldc if ldc is not None else N
    nbytes = getattr(lib, name + "_workspace_bytes")(M, N, K)
    ws = workspace(nbytes, A.device) if nbytes else None
    call(name, ptr(A), lda, int(transA), ptr(B), ldb, int(transB), ptr(C), ldc, *c_kind, M, N, K,
         ptr(bias1), ptr(bias2), ptr(rowgroup), (rowgroup.stride(0) if rowgroup is not None else 0),
         rg_div, rg_op, int(relu), int(accumulate), ptr(aux), ptr(ws), (ws.numel() * 4 if ws is not None else 0),
         tag, stream())
    return C


def gemm(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, M: int, N: int, K: int, *, transA=False,
         transB=True, lda=None, ldb=None, ldc=None, bias1=None, bias2=None, rowgroup=None, rg_div=1,
         rg_op=0, relu=False, accumulate=False, aux=None, tag=0, x3=False) -> torch.Tensor:
    """C[M,N] = act(op(A) op(B) (op) rowgroup + bias) (+C).  Leading dims default to the stored row length.
    x3: the contraction on the bf16 matrix cores with exact 3 x bf16 operand splits (csrc/x3_core.hpp)."""
    return _gemm("vqa_gemm_x3" if x3 else "vqa_gemm", (), A, B, C, M, N, K, transA, transB, lda, ldb, ldc, bias1, bias2, rowgroup,
                 rg_div, rg_op, relu, accumulate, aux, tag)


GEMM_ENGINES = {"vqa_gemm": 0, "vqa_gemm_x3": 1, "vqa_gemm_bf16": 2}
GEMM_PLAN_FIELDS = ("BM", "BN", "tiles_m", "tiles_n", "nk", "splits", "ks_per_split", "order", "persistent", "wide")


def gemm_plan(engine: str, M: int, N: int, K: int, *, transA=False, transB=True, workspace_bytes=None) -> dict:
    """The plan vqa_gemm / vqa_gemm_x3 / vqa_gemm_bf16 (engine: the entry point's name) runs for this shape under the VQA_* knobs
    in force, from the planners the launchers use (vqa_gemm_plan); makes no HIP call.  workspace_bytes: what the call would pass;
    the default is what _gemm passes with a workspace made for this claim (an older, larger workspace passes more)."""
    import ctypes
    lib = _lib.load()
    if workspace_bytes is None:
        nbytes = getattr(lib, engine + "_workspace_bytes")(M, N, K) if min(M, N, K) > 0 else 0     # vqa_gemm_plan rejects the rest
        workspace_bytes = _workspace_floats(nbytes) * 4 if nbytes else 0
    out = (ctypes.c_int32 * len(GEMM_PLAN_FIELDS))()
    call("vqa_gemm_plan", GEMM_ENGINES[engine], M, N, K, int(transA), int(transB), workspace_bytes, out, len(out))
    return dict(zip(GEMM_PLAN_FIELDS, out))


def nchw_to_nhwc4(x: torch.Tensor) -> torch.Tensor:
    B, Cc, H, W = x.shape
    y = torch.empty(B, H, W, 4, dtype=torch.float32, device=x.device)
    call("vqa_nchw_to_nhwc4", ptr(x), ptr(y), B, Cc, H, W, stream())
    return y


def conv_pack_weights(w: torch.Tensor, CiP: int, need_wd: bool = True):
    Co, Ci = w.shape[0], w.shape[1]
    wf = torch.empty(9 * CiP, Co, dtype=torch.float32, device=w.device)
    wd = torch.empty(9 * Co, CiP, dtype=torch.float32, device=w.device) if need_wd else None
    call("vqa_conv_pack_weights", ptr(w), ptr(wf), ptr(wd), Co, Ci, CiP, stream())
    return wf, wd


def conv_out_hw(H: int, W: int, stride: int) -> Tuple[int, int]:
    return ((H - 3) // stride + 1) // 2, ((W - 3) // stride + 1) // 2


def convk_out_hw(H: int, W: int, ks: int, stride: int) -> Tuple[int, int, int, int]:
    """(Ho, Wo, Hp, Wp) of Conv2d(kernel_size=ks, stride, pad=0) -> MaxPool2d(2,2) (models/model.py:80-82)."""
    Ho, Wo = (H - ks) // stride + 1, (W - ks) // stride + 1
    return Ho, Wo, Ho // 2, Wo // 2


def convk_pack_weights(w: torch.Tensor, CiP: int) -> torch.Tensor:
    """torch [Co][Ci][ks][ks] -> wk [Co][ks*ks*CiP], K index (ky*ks + kx)*CiP + ci (the im2col matrix's)."""
    Co, Ci, ks, ks2 = w.shape
    assert ks == ks2
    wk = torch.empty(Co, ks * ks * CiP, dtype=torch.float32, device=w.device)
    call("vqa_convk_pack_weights", ptr(w), ptr(wk), Co, Ci, CiP, ks, stream())
    return wk


def convk_unpack_wgrad(dwk: torch.Tensor, dw: torch.Tensor, CiP: int) -> torch.Tensor:
    Co, Ci, ks, _ = dw.shape
    call("vqa_convk_unpack_wgrad", ptr(dwk), ptr(dw), Co, Ci, CiP, ks, stream())
    return dw


def convk_chunk(B: int, H: int, W: int, CiP: int, Co: int, ks: int, stride: int, limit_bytes: int = 1 << 31) -> int:
    """Images per im2col chunk: the matrix [rows][ks*ks*CiP] (and the GEMM's [rows][Co] result) stay below limit_bytes."""
    Ho, Wo, _, _ = convk_out_hw(H, W, ks, stride)
    per_img = Ho * Wo * max(ks * ks * CiP, Co) * 4
    return max(1, min(B, limit_bytes // per_img))


def convk_fwd(x: torch.Tensor, wk: torch.Tensor, bias: torch.Tensor, ks: int, stride: int = 1, tag: int = 0, chunk: int = 0):
    """Conv block with kernel_size != 3, materialised form (csrc/conv_generic.hip): x NHWC [B,H,W,CiP] ->
    (pooled [B,Hp,Wp,Co], arg-max bytes).  im2col of a batch chunk, vqa_gemm with the bias in its epilogue, ReLU + pool."""
    B, H, W, CiP = x.shape
    Co, K = wk.shape
    assert K == ks * ks * CiP and x.dtype == torch.float32 and x.is_contiguous()
    Ho, Wo, Hp, Wp = convk_out_hw(H, W, ks, stride)
    assert Hp > 0 and Wp > 0, "image too small for conv + pool"
    pooled = torch.empty(B, Hp, Wp, Co, dtype=torch.float32, device=x.device)
    amax = torch.empty(B, Hp, Wp, Co, dtype=torch.uint8, device=x.device)
    nb = chunk or convk_chunk(B, H, W, CiP, Co, ks, stride)
    cols = torch.empty(nb * Ho * Wo, K, dtype=torch.float32, device=x.device)
    y = torch.empty(nb * Ho * Wo, Co, dtype=torch.float32, device=x.device)
    for b0 in range(0, B, nb):
        n = min(nb, B - b0)
        call("vqa_convk_im2col", ptr(x[b0:]), ptr(cols), n, H, W, CiP, ks, stride, stream())
        gemm(cols, wk, y, n * Ho * Wo, Co, K, transB=True, bias1=bias, tag=tag)
        call("vqa_convk_relu_pool", ptr(y), ptr(pooled[b0:]), ptr(amax[b0:]), n, Ho, Wo, Co, stream())
    return pooled, amax


def convk_bwd(x: torch.Tensor, dpooled: torch.Tensor, amax: torch.Tensor, wk: torch.Tensor, dw: torch.Tensor,
              dbias: torch.Tensor, ks: int, stride: int = 1, need_dx: bool = True, tag: int = 0, chunk: int = 0):
    """Backward of convk_fwd: dw [Co][Ci][ks][ks] and dbias are written, dX NHWC is returned (None if not need_dx)."""
    B, H, W, CiP = x.shape
    Co, K = wk.shape
    Ho, Wo, Hp, Wp = convk_out_hw(H, W, ks, stride)
    assert dpooled.shape == (B, Hp, Wp, Co) and dpooled.dtype == torch.float32 and dpooled.is_contiguous()
    nb = chunk or convk_chunk(B, H, W, CiP, Co, ks, stride)
    cols = torch.empty(nb * Ho * Wo, K, dtype=torch.float32, device=x.device)
    dy = torch.empty(nb * Ho * Wo, Co, dtype=torch.float32, device=x.device)
    dcols = torch.empty(nb * Ho * Wo, K, dtype=torch.float32, device=x.device) if need_dx else None
    dwk = torch.empty(Co, K, dtype=torch.float32, device=x.device)
    dx = torch.empty(B, H, W, CiP, dtype=torch.float32, device=x.device) if need_dx else None
    for b0 in range(0, B, nb):
        n = min(nb, B - b0)
        rows = n * Ho * Wo
        call("vqa_convk_route", ptr(dpooled[b0:]), ptr(amax[b0:]), ptr(dy), n, Ho, Wo, Co, stream())
        call("vqa_convk_im2col", ptr(x[b0:]), ptr(cols), n, H, W, CiP, ks, stride, stream())
        # dWk [Co][K] (+)= dY^T . cols over the chunk's rows
        gemm(dy, cols, dwk, Co, K, rows, transA=True, transB=False, accumulate=b0 > 0, tag=tag)
        if need_dx:
            gemm(dy, wk, dcols, rows, K, Co, transA=False, transB=False, tag=tag)
            call("vqa_convk_col2im", ptr(dcols), ptr(dx[b0:]), n, H, W, CiP, ks, stride, stream())
    convk_unpack_wgrad(dwk, dw, CiP)
    # windows whose ReLU was dead (arg-max byte 4) pass no gradient to the bias either
    colsum(dpooled, B * Hp * Wp, Co, dbias, mask=amax)
    return dx


def x3_split(x: torch.Tensor) -> torch.Tensor:
    """The exact three-way bf16 split of the fp32x3 kernels: x (fp32, numel % 4 == 0) -> planes [3, *x.shape] bf16
    (hi, mid, lo) with x == hi + mid + lo."""
    out = torch.empty((3,) + tuple(x.shape), dtype=torch.bfloat16, device=x.device)
    call("vqa_x3_split", ptr(x), ptr(out[0]), ptr(out[1]), ptr(out[2]), x.numel(), stream())
    return out


def x3_pack(x: torch.Tensor) -> torch.Tensor:
    """fp32 activation [..., C] (C % 4 == 0) -> the x3-packed form [..., C/4, 3, 4] bf16: every four channels as
    hi[4] mid[4] lo[4] (include/vqa_hip.h vqa_x3_pack); accepted as the input of conv_fwd / conv_wgrad with x3=True."""
    assert x.dtype == torch.float32 and x.shape[-1] % 4 == 0 and x.is_contiguous()
    out = torch.empty(tuple(x.shape[:-1]) + (x.shape[-1] // 4, 3, 4), dtype=torch.bfloat16, device=x.device)
    call("vqa_x3_pack", ptr(x), ptr(out), x.numel(), stream())
    return out


def nhwc_shape(x) -> tuple:
    """(B, H, W, C) of an NHWC activation, fp32 / bf16 [B,H,W,C] or x3-packed [B,H,W,C/4,3,4]."""
    if x.dim() == 6:
        return (x.shape[0], x.shape[1], x.shape[2], x.shape[3] * 4)
    return tuple(x.shape)


def x3_pack_pooled_grad(dpooled: torch.Tensor, amax: torch.Tensor, dbias: torch.Tensor) -> torch.Tensor:
    """x3_pack(dpooled) and, from the same read, dbias = sum of dpooled over the windows whose ReLU was alive."""
    Co = dpooled.shape[-1]
    out = torch.empty(tuple(dpooled.shape[:-1]) + (Co // 4, 3, 4), dtype=torch.bfloat16, device=dpooled.device)
    ws = workspace(_lib.load().vqa_x3_pack_pooled_grad_workspace_bytes(Co), dpooled.device)
    call("vqa_x3_pack_pooled_grad", ptr(dpooled), ptr(amax), ptr(out), ptr(dbias), dpooled.numel() // Co, Co, ptr(ws),
         ws.numel() * 4, stream())
    return out


def _x3_input(x):
    """(B, H, W, CiP, packed) of a conv input that is fp32 NHWC or x3-packed."""
    if x.dtype == torch.bfloat16 and x.dim() == 6:
        return x.shape[0], x.shape[1], x.shape[2], x.shape[3] * 4, 1
    assert x.dtype == torch.float32 and x.dim() == 4
    return x.shape[0], x.shape[1], x.shape[2], x.shape[3], 0


def conv_x3_supported(H: int, W: int, CiP: int, Co: int, stride: int) -> bool:
    return bool(_lib.load().vqa_conv3x3_x3_supported(H, W, CiP, Co, stride))


CONV_X3_PASSES = {"forward": 0, "dgrad": 1, "wgrad": 2}
CONV_X3_PLAN_FIELDS = ("BM", "BN", "waves", "tiles_m", "tiles_n", "persistent", "chunk", "launches", "nk", "splits", "ks_per_split")


def conv_x3_plan(pass_: str, B: int, H: int, W: int, CiP: int, Co: int, stride: int = 1) -> dict:
    """What conv_fwd / conv_dgrad / conv_wgrad with x3=True run for this layer and batch (pass_: "forward", "dgrad" or
    "wgrad") under the VQA_* knobs in force, from the host functions the launchers use (vqa_conv3x3_x3_plan); makes no HIP
    call.  `tiles` = tiles_m * tiles_n of the first launch; chunk: images per launch."""
    import ctypes
    out = (ctypes.c_int32 * len(CONV_X3_PLAN_FIELDS))()
    call("vqa_conv3x3_x3_plan", CONV_X3_PASSES[pass_], B, H, W, CiP, Co, stride, out, len(out))
    plan = dict(zip(CONV_X3_PLAN_FIELDS, out))
    plan["tiles"] = plan["tiles_m"] * plan["tiles_n"]
    return plan


def conv_fwd(x: torch.Tensor, wf: torch.Tensor, bias: torch.Tensor, stride: int = 1, tag: int = 0, x3: bool = False,
             out_packed: bool = False):
    """x NHWC [B,H,W,CiP] -> (pooled [B,Hp,Wp,Co], argmax uint8 same shape).  x3: fp32 on the bf16 matrix cores
    (exact 3 x bf16 operand split, csrc/x3_core.hpp) instead of the fp32 MFMA; wf is then x3_split(packed weights)."""
    B, H, W, CiP, packed = _x3_input(x) if x3 else (*x.shape, 0)
    Co = wf.shape[-1]
    assert (wf.dtype == torch.bfloat16 and wf.dim() == 3) if x3 else wf.dtype == torch.float32
    Hp, Wp = conv_out_hw(H, W, stride)
    assert x3 or not out_packed
    pooled = (torch.empty(B, Hp, Wp, Co // 4, 3, 4, dtype=torch.bfloat16, device=x.device) if out_packed else
              torch.empty(B, Hp, Wp, Co, dtype=torch.float32, device=x.device))
    amax = torch.empty(B, Hp, Wp, Co, dtype=torch.uint8, device=x.device)
    if x3:
        call("vqa_conv3x3_relu_pool_fwd_x3", ptr(x), packed, ptr(wf), ptr(bias), ptr(pooled), int(out_packed), ptr(amax),
             B, H, W, CiP, Co, stride, tag, stream())
    else:
        call("vqa_conv3x3_relu_pool_fwd", ptr(x), ptr(wf), ptr(bias), ptr(pooled), ptr(amax), B, H, W, CiP, Co, stride,
             tag, stream())
    return pooled, amax


def conv_dgrad(dpooled, amax, wd, x_shape, stride: int = 1, tag: int = 0, out=None, x3: bool = False) -> torch.Tensor:
    """dpooled: fp32 [B,Hp,Wp,Co], or (x3 only) its x3-packed form (x3_pack)."""
    B, H, W, CiP = x_shape
    Co = nhwc_shape(dpooled)[3]
    assert (wd.dtype == torch.bfloat16 and wd.dim() == 3) if x3 else wd.dtype == torch.float32
    dx = out if out is not None else torch.empty(B, H, W, CiP, dtype=torch.float32, device=dpooled.device)
    if x3:
        call("vqa_conv3x3_dgrad_x3", ptr(dpooled), int(dpooled.dim() == 6), ptr(amax), ptr(wd), ptr(dx), B, H, W, CiP, Co,
             stride, tag, stream())
    else:
        call("vqa_conv3x3_dgrad", ptr(dpooled), ptr(amax), ptr(wd), ptr(dx), B, H, W, CiP, Co, stride, tag, stream())
    return dx


def conv_wgrad(x, dpooled, amax, dw: torch.Tensor, dbias: torch.Tensor, stride: int = 1, tag: int = 0, x3: bool = False,
               dpooled_packed=None):
    """x3: x may be x3-packed; dpooled_packed (optional) = x3_pack(dpooled), read by the contraction instead of dpooled;
    dbias None (x3 only): the bias gradient is not computed here (x3_pack_pooled_grad already produced it)."""
    lib = _lib.load()
    B, H, W, CiP, packed = _x3_input(x) if x3 else (*x.shape, 0)
    Co, Ci = dw.shape[0], dw.shape[1]
    nbytes = (lib.vqa_conv3x3_wgrad_x3_workspace_bytes if x3 else lib.vqa_conv3x3_wgrad_workspace_bytes)(B, H, W, CiP, Co, stride)
    ws = workspace(nbytes, x.device)
    if x3:
        call("vqa_conv3x3_wgrad_x3", ptr(x), packed, ptr(dpooled), ptr(dpooled_packed) if dpooled_packed is not None else None,
             ptr(amax), ptr(dw), ptr(dbias), B, H, W, CiP, Ci, Co, stride, ptr(ws), ws.numel() * 4, tag, stream())
        return
    call("vqa_conv3x3_wgrad", ptr(x), ptr(dpooled), ptr(amax), ptr(dw), ptr(dbias), B, H, W, CiP, Ci, Co, stride,
         ptr(ws), ws.numel() * 4, tag, stream())


def conv0_supported(Ci: int, H: int, W: int, Co: int, stride: int) -> bool:
    return bool(_lib.load().vqa_conv0_supported(Ci, H, W, Co, stride))


def conv0_fwd(x_nchw: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out_dtype=torch.float32, bf16_mfma=False,
              out_packed=False, out_c16=False):
    """First conv block straight from the NCHW image: (pooled NHWC [B,Hp,Wp,Co] fp32 or bf16, argmax uint8).
    bf16_mfma (bf16 output only): image and weights rounded to bf16, bf16 MFMA.  out_packed: fp32 MFMA, the output
    written in the x3-packed form [B,Hp,Wp,Co/4,3,4] bf16 (see x3_pack).  out_c16 (with bf16_mfma): the pooled map
    channel-blocked [B,Co/16,Hp,Wp,16] for the patch convolutions; the arg-max bytes stay NHWC."""
    B, Ci, H, W = x_nchw.shape
    Co = w.shape[0]
    Hp, Wp = conv_out_hw(H, W, 1)
    assert not out_c16 or (bf16_mfma and out_dtype == torch.bfloat16 and not out_packed)
    pooled = (torch.empty(B, Hp, Wp, Co // 4, 3, 4, dtype=torch.bfloat16, device=x_nchw.device) if out_packed else
              torch.empty(B, Co // 16, Hp, Wp, 16, dtype=torch.bfloat16, device=x_nchw.device) if out_c16 else
              torch.empty(B, Hp, Wp, Co, dtype=out_dtype, device=x_nchw.device))
    amax = torch.empty(B, Hp, Wp, Co, dtype=torch.uint8, device=x_nchw.device)
    mode = 3 if out_packed else (4 if out_c16 else 2 if bf16_mfma else 1) if out_dtype == torch.bfloat16 else 0
    assert x_nchw.dtype in (torch.float32, torch.float16) and x_nchw.is_contiguous()
    call("vqa_conv0_relu_pool_fwd", ptr(x_nchw), int(x_nchw.dtype == torch.float16), ptr(w), ptr(bias), ptr(pooled), mode,
         ptr(amax), B, Ci, H, W, Co, stream())
    return pooled, amax


def conv0_wgrad(x_nchw, dpooled, amax, dw: torch.Tensor, dbias: torch.Tensor):
    lib = _lib.load()
    B, Ci, H, W = x_nchw.shape
    Co = dw.shape[0]
    ws = workspace(lib.vqa_conv0_wgrad_workspace_bytes(Co), x_nchw.device)
    call("vqa_conv0_wgrad", ptr(x_nchw), int(x_nchw.dtype == torch.float16), ptr(dpooled), ptr(amax), ptr(dw), ptr(dbias), B, Ci, H, W, Co, ptr(ws),
         ws.numel() * 4, stream())


def conv0_wgrad_bf16(x_nchw, dpooled16, amax, dw: torch.Tensor, dbias: torch.Tensor):
    """First block's weight / bias gradient on bf16 MFMA from the bf16 pooled gradient."""
    assert dpooled16.dtype == torch.bfloat16
    lib = _lib.load()
    B, Ci, H, W = x_nchw.shape
    Co = dw.shape[0]
    ws = workspace(lib.vqa_conv0_wgrad_workspace_bytes(Co), x_nchw.device)
    call("vqa_conv0_wgrad_bf16", ptr(x_nchw), int(x_nchw.dtype == torch.float16), ptr(dpooled16), ptr(amax), ptr(dw), ptr(dbias), B, Ci, H, W, Co, ptr(ws),
         ws.numel() * 4, stream())


def conv0_dgrad_supported(Ci: int, H: int, W: int, Co: int, stride: int) -> bool:
    return bool(_lib.load().vqa_conv0_dgrad_supported(Ci, H, W, Co, stride))


def conv0_dgrad(dpooled: torch.Tensor, amax: torch.Tensor, w: torch.Tensor, x_shape, out_dtype=torch.float32,
                round_w_bf16: bool = False) -> torch.Tensor:
    """Input-image gradient of the dedicated first block: dpooled NHWC [B,Hp,Wp,Co] (fp32 or bf16) routed through the
    arg-max bytes and w [Co,Ci,3,3] -> dv NCHW x_shape (fp32 or fp16).  round_w_bf16: the weights as the bf16-path forward
    uses them."""
    B, Ci, H, W = x_shape
    Co = w.shape[0]
    Hp, Wp = conv_out_hw(H, W, 1)
    assert dpooled.dtype in (torch.float32, torch.bfloat16) and dpooled.is_contiguous() and dpooled.shape == (B, Hp, Wp, Co)
    assert amax.dtype == torch.uint8 and amax.shape == dpooled.shape and w.dtype == torch.float32 and w.is_contiguous()
    assert out_dtype in (torch.float32, torch.float16)
    dv = torch.empty(B, Ci, H, W, dtype=out_dtype, device=dpooled.device)
    call("vqa_conv0_dgrad", ptr(dpooled), int(dpooled.dtype == torch.bfloat16), ptr(amax), ptr(w), ptr(dv),
         int(out_dtype == torch.float16), int(round_w_bf16), B, Ci, H, W, Co, stream())
    return dv


def nhwc_to_nchw(x: torch.Tensor, C: int, out_dtype=torch.float32) -> torch.Tensor:
    """fp32 NHWC [B,H,W,CP] -> NCHW [B,C,H,W] (fp32 or fp16), the pad channels dropped: the inverse of nchw_to_nhwc4."""
    B, H, W, CP = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and out_dtype in (torch.float32, torch.float16)
    y = torch.empty(B, C, H, W, dtype=out_dtype, device=x.device)
    call("vqa_nhwc_to_nchw", ptr(x), ptr(y), int(out_dtype == torch.float16), B, C, CP, H, W, stream())
    return y


def dropout(x: torch.Tensor, p: float, seed: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    y = out if out is not None else torch.empty_like(x)
    call("vqa_dropout", ptr(x), ptr(y), x.numel(), p, seed, stream())
    return y


def dropout_add(x: torch.Tensor, y: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    """y += dropout_{p, seed}(x) in one pass."""
    call("vqa_dropout_add", ptr(x), ptr(y), x.numel(), p, seed, stream())
    return y


def l2norm_fwd(pooled: torch.Tensor, p: float, seed: int, drop2=None):
    """drop2 = (p2, seed2, dtype): also return dropout_{p2, seed2}(vn) in fp32 or bf16 (written in the same pass)."""
    C = pooled.shape[-1]
    rows = pooled.numel() // C
    vn = torch.empty_like(pooled)
    norm = torch.empty(rows, dtype=torch.float32, device=pooled.device)
    if drop2 is None:
        call("vqa_l2norm_fwd", ptr(pooled), ptr(vn), ptr(norm), rows, C, p, seed, None, 0, 0.0, 0, stream())
        return vn, norm
    p2, seed2, dtype = drop2
    vd = torch.empty(pooled.shape, dtype=dtype, device=pooled.device)
    call("vqa_l2norm_fwd", ptr(pooled), ptr(vn), ptr(norm), rows, C, p, seed, ptr(vd), int(dtype == torch.bfloat16), p2, seed2,
         stream())
    return vn, norm, vd


def l2norm_bwd(dvn, vn, norm, p: float, seed: int, out=None, out_dtype=torch.float32, c16_hw=None):
    """out_dtype=torch.bfloat16: the gradient is stored as bf16 (the bf16 path's pooled gradient of the last conv block);
    c16_hw=(Hp, Wp): bf16, channel-blocked [B, C/16, Hp, Wp, 16] (what the patch convolutions' backward kernels read)."""
    C = vn.shape[-1]
    rows = vn.numel() // C
    if c16_hw is not None:
        Hp, Wp = c16_hw
        assert out is None and rows % (Hp * Wp) == 0 and C % 16 == 0
        d = torch.empty(rows // (Hp * Wp), C // 16, Hp, Wp, 16, dtype=torch.bfloat16, device=vn.device)
        call("vqa_l2norm_bwd", ptr(dvn), ptr(vn), ptr(norm), ptr(d), 2, rows, Hp * Wp, C, p, seed, stream())
        return d
    d = out if out is not None else torch.empty(vn.shape, dtype=out_dtype, device=vn.device)
    call("vqa_l2norm_bwd", ptr(dvn), ptr(vn), ptr(norm), ptr(d), int(d.dtype == torch.bfloat16), rows, 0, C, p, seed, stream())
    return d


def l2norm_bwd_joined(dout, dout_ld, probs, dv_in, p_v: float, seed_v: int, vn, norm, p: float, seed: int,
                      out_dtype=torch.float32, c16_hw=None):
    """l2norm_bwd whose incoming gradient is joined in the kernel: sum_g probs[b,g,p] * dout[b, g*C:(g+1)*C] (what att_apply_bwd
    would have written) + dropout_{p_v, seed_v}-mask * dv_in (what dropout_add would have added)."""
    B, G, P = probs.shape
    C = vn.shape[-1]
    rows = vn.numel() // C
    assert rows == B * P and dv_in.numel() == rows * C and dv_in.dtype == torch.float32
    if c16_hw is not None:
        Hp, Wp = c16_hw
        assert Hp * Wp == P and C % 16 == 0
        d = torch.empty(B, C // 16, Hp, Wp, 16, dtype=torch.bfloat16, device=vn.device)
        mode = 2
    else:
        d = torch.empty(vn.shape, dtype=out_dtype, device=vn.device)
        mode = int(out_dtype == torch.bfloat16)
    call("vqa_l2norm_bwd_joined", ptr(dout), dout_ld, ptr(probs), G, ptr(dv_in), p_v, seed_v, ptr(vn), ptr(norm), ptr(d), mode,
         rows, P, C, p, seed, stream())
    return d


def embed_tanh_fwd(q: torch.Tensor, emb: torch.Tensor, p: float, seed: int,
                   bad_tokens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bad_tokens: optional device int32 [1], incremented once per token id outside [0, V)."""
    B, T = q.shape
    V, E = emb.shape
    x = torch.empty(T, B, E, dtype=torch.float32, device=emb.device)
    call("vqa_embed_tanh_fwd", ptr(q), ptr(emb), ptr(x), B, T, E, V, p, seed, ptr(bad_tokens), stream())
    return x


def embed_tanh_bwd(q, x, dx, demb, p: float, seed: int, binned: bool = True):
    """binned=False: the workspace-less scanning kernel (O(V * B*T)); same bits."""
    B, T = q.shape
    V, E = demb.shape
    if binned:
        ws = workspace(_lib.load().vqa_embed_tanh_bwd_workspace_bytes(B, T, V), q.device)
        call("vqa_embed_tanh_bwd", ptr(q), ptr(x), ptr(dx), ptr(demb), B, T, E, V, p, seed, ptr(ws), ws.numel() * 4, stream())
    else:
        call("vqa_embed_tanh_bwd", ptr(q), ptr(x), ptr(dx), ptr(demb), B, T, E, V, p, seed, None, 0, stream())


def lstm_cell_fwd(xg_t, hg, c_in, h_in, q_len, t, gates, c_out, h_out, c_final=None, cf_ld=0):
    B, H = c_in.shape
    call("vqa_lstm_cell_fwd", ptr(xg_t), ptr(hg), ptr(c_in), ptr(h_in), ptr(q_len), t, ptr(gates), ptr(c_out),
         ptr(h_out), ptr(c_final), cf_ld, B, H, stream())


def lstm_step_supported(H: int) -> bool:
    return bool(_lib.load().vqa_lstm_step_supported(H))


def _lstm_dirs(dirs):
    """[{w_hh, xg, gates, Hs, Cs, c_final, dgates, dh, dc, reverse}] -> ctypes array of vqa_lstm_dir_t."""
    arr = (_lib.LstmDir * len(dirs))()
    for k, d in enumerate(dirs):
        for f in ("w_hh", "xg", "gates", "Hs", "Cs", "c_final", "dgates", "dh", "dc"):
            setattr(arr[k], f, ptr(d.get(f)))
        arr[k].reverse = int(bool(d.get("reverse", False)))
    return arr


def lstm_seq_fwd(dirs, q_len, B: int, T: int, H: int, cf_ld: int = 0, use_graph: bool = True):
    """The whole recurrence, forward: one call = T launches (each covers every direction), optionally as a cached
    hipGraph.  dirs: list of dicts with tensors w_hh [4H,H], xg [T,B,4H], gates [T,B,4H], Hs / Cs [T+1,B,H]
    (initial slot zeroed by the caller), optional c_final [B, cf_ld], reverse."""
    import ctypes
    arr = _lstm_dirs(dirs)
    call("vqa_lstm_seq_fwd", ctypes.addressof(arr), len(dirs), ptr(q_len), B, T, H, cf_ld, int(use_graph), stream())


def lstm_seq_bwd(dirs, q_len, B: int, T: int, H: int, use_graph: bool = True):
    """BPTT of the recurrence: fills dgates [T,B,4H] per direction; dh (d loss / d h_n: zeros for the model) / dc
    (d loss / d c_n) are updated in place and hold, on return, d loss / d h written by the first processed time and
    d loss / d c_0 (include/vqa_hip.h).  Needs gates, Hs, Cs of the forward pass and w_hh."""
    import ctypes
    arr = _lstm_dirs(dirs)
    call("vqa_lstm_seq_bwd", ctypes.addressof(arr), len(dirs), ptr(q_len), B, T, H, int(use_graph), stream())


def lstm_graph_stats():
    """(replays, builds, plain-launch fallbacks, cached graphs) of the library's LSTM-sequence hipGraph cache."""
    import ctypes
    a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    n = _lib.load().vqa_lstm_graph_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return a.value, b.value, c.value, n


def lstm_cell_bwd(gates, c_in, c_out, q_len, t, dh, dc, dgates):
    B, H = c_in.shape
    call("vqa_lstm_cell_bwd", ptr(gates), ptr(c_in), ptr(c_out), ptr(q_len), t, ptr(dh), ptr(dc), ptr(dgates),
         B, H, stream())


def _score_dims(wx, concat: bool):
    """(G, xld, mid) of the x_conv weights wx [G, xld]: xld = mid ('+', '*') or 2*mid ('|', concat)."""
    return wx.shape[0], wx.shape[1], wx.shape[1] // 2 if concat else wx.shape[1]


def att_score_fwd(xs, wx, bx, B, P, p: float, seed: int, qcat=None) -> torch.Tensor:
    """wx [G, xld] with xld = mid ('+', '*') or 2*mid ('|', qcat = q' [B, mid])."""
    G, xld, mid = _score_dims(wx, qcat is not None)
    score = torch.empty(B, G, P, dtype=torch.float32, device=xs.device)
    call("vqa_att_score_fwd", ptr(xs), int(xs.dtype == torch.bfloat16), ptr(wx), xld, ptr(bx), ptr(score), B, P, mid, G, p,
         seed, ptr(qcat), stream())
    return score


def att_score_bwd(dscore, wx, xs_inout, B, P, p: float, seed: int, mode: int = 0, vprime=None, qp=None):
    G, xld, mid = _score_dims(wx, mode == 2)
    RS = _lib.load().vqa_att_row_splits(P)
    dwx_part = torch.empty(B * RS, G * xld, dtype=torch.float32, device=wx.device)
    dq_part = torch.empty(B * RS, mid, dtype=torch.float32, device=wx.device)
    call("vqa_att_score_bwd", ptr(dscore), ptr(wx), xld, ptr(xs_inout), int(xs_inout.dtype == torch.bfloat16), ptr(dwx_part),
         ptr(dq_part), B, P, mid, G, p, seed, mode, ptr(vprime), ptr(qp), stream())
    return dwx_part, dq_part, RS


def att_apply_fwd(score, vn, out, out_ld):
    B, G, P = score.shape
    C = vn.shape[-1]
    probs = torch.empty_like(score)
    call("vqa_att_apply_fwd", ptr(score), ptr(vn), ptr(probs), ptr(out), out_ld, B, P, C, G, stream())
    return probs


def _grouped_score_head(vprime, qp, wx, order, offsets, N: int, B: int, P: int, mode: int, q_rows: int):
    """What the att_score_grouped_*_fwd wrappers check and allocate: (G, xld, mid, score [B, G, P]); qp is [q_rows, mid]."""
    G, xld, mid = _score_dims(wx, mode == 2)
    _chk(order, torch.int32), _chk(offsets, torch.int32)
    assert order.numel() == B and offsets.numel() == N + 1 and vprime.shape == (N * P, mid) and qp.shape == (q_rows, mid)
    return G, xld, mid, torch.empty(B, G, P, dtype=torch.float32, device=vprime.device)


def att_score_grouped_fwd(vprime, qp, wx, bx, order, offsets, N: int, B: int, P: int, mode: int, qrow=None) -> torch.Tensor:
    """Scores [B, G, P] of B questions against N images from ONE v' [N*P, mid] per image: order / offsets (device int32,
    model.group_by_image) list the questions of image n as order[offsets[n]:offsets[n+1]].  mode 0 '+', 1 '*', 2 '|'
    (wx [G, 2*mid]).  vprime is fp32 or float16 (a float16 cache: the same scores as from vprime.float(), bit for bit).
    qrow (device int32 [B]): the pairs form over a table qp [M, mid] of distinct questions -- pair b reads the row
    qp[qrow[b]] --, bit-identical to the plain form on qp[qrow]."""
    _chk(qp)
    sfx = _cache_suffix(vprime)
    if qrow is None:
        G, xld, mid, score = _grouped_score_head(vprime, qp, wx, order, offsets, N, B, P, mode, B)
        call("vqa_att_score_grouped_fwd" + sfx, ptr(vprime), ptr(qp), ptr(wx), xld, ptr(bx), ptr(order), ptr(offsets), ptr(score),
             N, B, P, mid, G, mode, stream())
    else:
        M = qp.shape[0]
        _chk(qrow, torch.int32)
        assert qrow.numel() == B
        G, xld, mid, score = _grouped_score_head(vprime, qp, wx, order, offsets, N, B, P, mode, M)
        call("vqa_att_score_grouped_pairs_fwd" + sfx, ptr(vprime), ptr(qp), ptr(qrow), ptr(wx), xld, ptr(bx), ptr(order),
             ptr(offsets), ptr(score), N, B, M, P, mid, G, mode, stream())
    return score


def att_score_grouped_pairs_fwd(vprime, qp, qrow, wx, bx, order, offsets, N: int, B: int, P: int, mode: int) -> torch.Tensor:
    """att_score_grouped_fwd with qrow: the name the pairs form had when it was a wrapper of its own."""
    return att_score_grouped_fwd(vprime, qp, wx, bx, order, offsets, N, B, P, mode, qrow=qrow)


def gather_rows(src, rows, dst, cols: Optional[int] = None):
    """dst[b, :cols] = src[rows[b], :cols] (rows device int32 [B]; zeros for an index outside [0, M)).  src [M, >= cols] and
    dst [B, >= cols] are fp32 row-major views with unit column stride: a column range of a wider buffer is written in
    place (the leading dimensions are the views' row strides)."""
    M, B = src.shape[0], dst.shape[0]
    cols = src.shape[1] if cols is None else cols
    assert src.dtype == torch.float32 and dst.dtype == torch.float32 and src.is_cuda and dst.is_cuda
    _chk(rows, torch.int32)
    assert rows.numel() == B and src.shape[1] >= cols and dst.shape[1] >= cols
    assert (cols == 1 or (src.stride(1) == 1 and dst.stride(1) == 1))
    call("vqa_gather_rows", ptr(src), _ld(src), ptr(rows), ptr(dst), _ld(dst), B, M, cols, stream())
    return dst


def gather_rows_drop(src, rows, p: float, seed: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[j] = dropout_{p, seed}(src)[rows[j]] without forming the dropped src: src [M, ...] is a contiguous fp32 bank of
    rows, rows device int32 [n]; the mask of element i of bank row r is drop_scale(seed, r * row_len + i) (64-bit), the one
    dropout(src, p, seed) applies.  p = 0 copies; an index outside [0, M) gives a row of zeros.  Returns [n, ...], fp32.
    A float16 bank is widened as it is read: the same bits as from src.float()."""
    _chk(rows, torch.int32)
    assert src.is_contiguous()
    M, n = src.shape[0], rows.numel()
    row_len = src.numel() // M
    if out is None:
        out = torch.empty((n,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and out.numel() == n * row_len
    call("vqa_gather_rows_drop" + _cache_suffix(src), ptr(src), ptr(rows), ptr(out), n, M, row_len, p, seed, stream())
    return out


def gather_rows_drop_norm(src, rows, p: float, seed: int, drop2=None):
    """Image dropout on the asked rows of a bank of L2-normalised features: vn_d[j] = l2norm(dropout_{p, seed}(src)[rows[j]]),
    every feature row of C channels renormalised after the mask (vqa_l2norm_fwd's operations), without forming the dropped
    bank.  src [M, P, C] contiguous, fp32 or float16 (widened as it is read: the bits of src.float()); rows device int32 [n];
    masks are indexed by the BANK row (64-bit), as gather_rows_drop's.  drop2 = (p2, seed2): also return
    v_in = dropout_{p2, seed2}(.)[rows] of vn_d, written in the same pass.  An index outside [0, M) gives zeros.  Returns
    vn_d [n, P, C] fp32, or (vn_d, v_in)."""
    _chk(rows, torch.int32)
    assert src.dim() == 3 and src.is_contiguous()
    (M, P, C), n = src.shape, rows.numel()
    vn_d = torch.empty(n, P, C, dtype=torch.float32, device=src.device)
    name = "vqa_gather_rows_drop_norm" + _cache_suffix(src)
    if drop2 is None:
        call(name, ptr(src), ptr(rows), ptr(vn_d), None, n, M, P, C, p, seed, 0.0, 0, stream())
        return vn_d
    p2, seed2 = drop2
    v_in = torch.empty_like(vn_d)
    call(name, ptr(src), ptr(rows), ptr(vn_d), ptr(v_in), n, M, P, C, p, seed, p2, seed2, stream())
    return vn_d, v_in


def _apply_gather_head(probs, vn, img):
    """What the att_apply_gather_* wrappers check: (B, G, P, N, C) of probs-shaped [B, G, P], vn [N, P, C], img int32 [B]."""
    (B, G, P), N, C = probs.shape, vn.shape[0], vn.shape[-1]
    _chk(img, torch.int32)
    assert img.numel() == B and vn.numel() == N * P * C
    return B, G, P, N, C


def att_apply_gather_dscore(dout, dout_ld, probs, vn, img, rowsum=None):
    """The dscore half of att_apply_gather_bwd (same device code, same bits), for a vn nobody wants a gradient of: vn
    [N, P, C] may be a large bank, fp32 or float16, only the rows img[b] (device int32 [B]) are read."""
    B, G, P, N, C = _apply_gather_head(probs, vn, img)
    dscore = torch.empty_like(probs)
    call("vqa_att_apply_gather_dscore" + _cache_suffix(vn), ptr(dout), dout_ld, ptr(probs), ptr(vn), ptr(img), ptr(dscore), ptr(rowsum), N, B, P, C, G,
         stream())
    return dscore


def att_attr_apply_gather(dout, dout_ld, probs, vn, img, rowsum=None):
    """att_apply_gather_dscore (the same device code, the same dscore / rowsum bits) that also returns r1 [B, P] =
    sum_g probs * (vn[img] . dout_g): the weighted-sum path of the gradient x input map (include/vqa_hip.h).  Returns
    (dscore [B, G, P], r1 [B, P]); vn fp32 or float16."""
    B, G, P, N, C = _apply_gather_head(probs, vn, img)
    dscore = torch.empty_like(probs)
    r1 = torch.empty(B, P, dtype=torch.float32, device=probs.device)
    call("vqa_att_attr_apply_gather" + _cache_suffix(vn), ptr(dout), dout_ld, ptr(probs), ptr(vn), ptr(img), ptr(dscore), ptr(rowsum), ptr(r1),
         N, B, P, C, G, stream())
    return dscore, r1


def att_attr_score_grouped_path(mode: int, mid: int) -> int:
    """The kernel att_attr_score_grouped runs for (mode, mid): 0 = the register kernel, else the general kernel with that many
    positions per wave."""
    return _lib.load().vqa_att_attr_score_grouped_path(mode, mid)


def att_attr_score_grouped(r1, dscore, vprime, qp, wx, order, offsets, N: int, B: int, P: int, mode: int, qrow=None, out=None):
    """The gradient x input map R [B, P] = r1 + r2 (include/vqa_hip.h) from r1 [B, P], dscore [B, G, P] (att_attr_apply_gather),
    ONE v' [N*P, mid] per image (fp32 or float16), q' and wx [G, xld]; order / offsets as att_score_grouped_fwd.  qrow (device
    int32 [B]): the pairs form over a table qp [M, mid], bit-identical to the plain form on qp[qrow].  mode 2 ('|') reads no
    q' (qp may be None).  out: written in place where a listed question has a row; rows of images nobody asks about and of
    questions that are not listed are left as they are."""
    G, xld, mid = _score_dims(wx, mode == 2)
    _chk(order, torch.int32), _chk(offsets, torch.int32), _chk(r1), _chk(dscore)
    M = qp.shape[0] if qp is not None else (B if qrow is None else 1)
    assert order.numel() == B and offsets.numel() == N + 1 and vprime.shape == (N * P, mid)
    assert r1.shape == (B, P) and dscore.shape == (B, G, P) and r1.is_contiguous() and dscore.is_contiguous()
    assert qp is None or (qp.dtype == torch.float32 and qp.shape == (M if qrow is not None else B, mid))
    if out is None:
        out = torch.empty(B, P, dtype=torch.float32, device=vprime.device)
    assert out.shape == (B, P) and out.is_contiguous() and out.dtype == torch.float32
    sfx = _cache_suffix(vprime)
    if qrow is None:
        call("vqa_att_attr_score_grouped" + sfx, ptr(r1), ptr(dscore), ptr(vprime), ptr(qp), ptr(wx), xld, ptr(order), ptr(offsets),
             ptr(out), N, B, P, mid, G, mode, stream())
    else:
        _chk(qrow, torch.int32)
        assert qrow.numel() == B
        call("vqa_att_attr_score_grouped_pairs" + sfx, ptr(r1), ptr(dscore), ptr(vprime), ptr(qp), ptr(qrow), ptr(wx), xld, ptr(order),
             ptr(offsets), ptr(out), N, B, M, P, mid, G, mode, stream())
    return out


ATT_PATH_MAX_STEPS = 64     # VQA_ATT_PATH_MAX_STEPS


def att_path_score_grouped(vprime, qp, wx, bx, alphas, order, offsets, N: int, B: int, P: int, mode: int, qrow=None,
                           out=None) -> torch.Tensor:
    """att_score_grouped_fwd at every step of the path alpha * v' (include/vqa_hip.h): score [B, S, G, P] from ONE v' [N*P, mid]
    per image (fp32 or float16), read once whatever S is; alphas device fp32 [S], 1 <= S <= 64.  qrow: the pairs form, as
    att_score_grouped_fwd's.  out: written in place (a [>= B, S, G, P] workspace's first B rows)."""
    _chk(qp), _chk(alphas)
    S = alphas.numel()
    G, xld, mid = _score_dims(wx, mode == 2)
    _chk(order, torch.int32), _chk(offsets, torch.int32)
    assert order.numel() == B and offsets.numel() == N + 1 and vprime.shape == (N * P, mid)
    assert qp.shape == (B if qrow is None else qp.shape[0], mid) and alphas.is_contiguous()
    if out is None:
        out = torch.empty(B, S, G, P, dtype=torch.float32, device=vprime.device)
    assert out.shape == (B, S, G, P) and out.is_contiguous() and out.dtype == torch.float32
    sfx = _cache_suffix(vprime)
    if qrow is None:
        call("vqa_att_path_score_grouped" + sfx, ptr(vprime), ptr(qp), ptr(wx), xld, ptr(bx), ptr(alphas), ptr(order), ptr(offsets),
             ptr(out), N, B, S, P, mid, G, mode, stream())
    else:
        _chk(qrow, torch.int32)
        assert qrow.numel() == B
        call("vqa_att_path_score_grouped_pairs" + sfx, ptr(vprime), ptr(qp), ptr(qrow), ptr(wx), xld, ptr(bx), ptr(alphas),
             ptr(order), ptr(offsets), ptr(out), N, B, qp.shape[0], S, P, mid, G, mode, stream())
    return out


def att_path_scale_rows(x, alphas, cols: int):
    """x[r, :cols] *= alphas[r % S] in place, for the step-rows r = b*S + s of a 2-D fp32 view x with unit column stride (the
    image half of the classifier input at each step's path position); alphas device fp32 [S]."""
    _chk(x), _chk(alphas)
    assert x.dim() == 2 and x.shape[1] >= cols and (x.shape[1] == 1 or x.stride(1) == 1) and alphas.is_contiguous()
    call("vqa_att_path_scale_rows", ptr(x), _ld(x), ptr(alphas), alphas.numel(), x.shape[0], cols, stream())
    return x


def att_path_attr_grouped(r1, dscore, vprime, qp, wx, alphas, scale: float, order, offsets, N: int, B: int, P: int, mode: int,
                          qrow=None, out=None):
    """The path sum of att_attr_score_grouped (include/vqa_hip.h): out [B, P] = scale * sum_s (r1[:, s] + r2_s) from r1
    [B, S, P] and dscore [B, S, G, P] (att_attr_apply_gather on the B*S step-rows), ONE v' [N*P, mid] per image (fp32 or
    float16), read once whatever S is; alphas device fp32 [S].  qrow, mode 2 without q' and out: att_attr_score_grouped's."""
    G, xld, mid = _score_dims(wx, mode == 2)
    _chk(order, torch.int32), _chk(offsets, torch.int32), _chk(r1), _chk(dscore), _chk(alphas)
    S = alphas.numel()
    M = qp.shape[0] if qp is not None else (B if qrow is None else 1)
    assert order.numel() == B and offsets.numel() == N + 1 and vprime.shape == (N * P, mid) and alphas.is_contiguous()
    assert r1.shape == (B, S, P) and dscore.shape == (B, S, G, P) and r1.is_contiguous() and dscore.is_contiguous()
    assert qp is None or (qp.dtype == torch.float32 and qp.shape == (M if qrow is not None else B, mid))
    if out is None:
        out = torch.empty(B, P, dtype=torch.float32, device=vprime.device)
    assert out.shape == (B, P) and out.is_contiguous() and out.dtype == torch.float32
    sfx = _cache_suffix(vprime)
    if qrow is None:
        call("vqa_att_path_attr_grouped" + sfx, ptr(r1), ptr(dscore), ptr(vprime), ptr(qp), ptr(wx), xld, ptr(alphas), scale,
             ptr(order), ptr(offsets), ptr(out), N, B, S, P, mid, G, mode, stream())
    else:
        _chk(qrow, torch.int32)
        assert qrow.numel() == B
        call("vqa_att_path_attr_grouped_pairs" + sfx, ptr(r1), ptr(dscore), ptr(vprime), ptr(qp), ptr(qrow), ptr(wx), xld,
             ptr(alphas), scale, ptr(order), ptr(offsets), ptr(out), N, B, M, S, P, mid, G, mode, stream())
    return out


def att_attr_dq_grouped(dscore, vprime, qp, wx, order, offsets, N: int, B: int, P: int, mode: int, dq_part=None):
    """d logit / d q' through the attention scores (include/vqa_hip.h), from the dscore [B, G, P] of att_attr_apply_gather:
    att_score_grouped_bwd at p = 0 without dvprime and dwx_part, bit for bit.  Returns (dq_part [B*NT, mid], NT);
    sum_parts(dq_part, out, B, NT, mid) finishes it.  vprime fp32 or float16; mode 0 '+' or 1 '*' (2, '|': the library
    refuses -- that gradient is identically zero).  dq_part: written in place; the rows of questions that are not listed in
    order / offsets are left as they are."""
    G, xld, mid = _score_dims(wx, mode == 2)
    _chk(order, torch.int32), _chk(offsets, torch.int32), _chk(dscore), _chk(qp)
    assert order.numel() == B and offsets.numel() == N + 1 and vprime.shape == (N * P, mid) and qp.shape == (B, mid)
    assert dscore.shape == (B, G, P) and dscore.is_contiguous()
    NT = _lib.load().vqa_att_score_grouped_tiles(P)
    if dq_part is None:
        dq_part = torch.empty(B * NT, mid, dtype=torch.float32, device=vprime.device)
    assert dq_part.shape == (B * NT, mid) and dq_part.is_contiguous() and dq_part.dtype == torch.float32
    call("vqa_att_attr_dq_grouped" + _cache_suffix(vprime), ptr(dscore), ptr(vprime), ptr(qp), ptr(wx), xld, ptr(order),
         ptr(offsets), ptr(dq_part), N, B, P, mid, G, mode, stream())
    return dq_part, NT


def embed_attr(q, emb, x, dx0, dx1, q_len, out=None):
    """Gradient x input per token slot (include/vqa_hip.h vqa_embed_attr): words [B, T] from q int64 [B, T], the embedding
    table emb [V, E], x = tanh(emb[q]) [T, B, E] as embed_tanh_fwd wrote it, the gradient at x as dx0 (+ dx1, or None)
    [T*B, E] and q_len int64 [B].  Every element is written, 0 for t >= q_len[b] and for a token id outside [0, V)."""
    B, T = q.shape
    V, E = emb.shape
    _chk(q, torch.int64), _chk(q_len, torch.int64)
    for t in (emb, x, dx0) + (() if dx1 is None else (dx1,)):
        _chk(t)
        assert t.is_contiguous()
    assert q.is_contiguous() and q_len.numel() == B and x.numel() == T * B * E and dx0.numel() == T * B * E
    assert dx1 is None or dx1.numel() == T * B * E
    if out is None:
        out = torch.empty(B, T, dtype=torch.float32, device=emb.device)
    assert out.shape == (B, T) and out.is_contiguous() and out.dtype == torch.float32
    call("vqa_embed_attr", ptr(q), ptr(emb), ptr(x), ptr(dx0), ptr(dx1), ptr(q_len), ptr(out), B, T, E, V, stream())
    return out


def _occl_operands(base, U, slot, probs, score, cnull, W2=None, b2=None, answers=None):
    """What occl_logit and occl_curves ask of the operands they share: (B, G, P, R, hid, A, w2_ld).  Without the column
    operands W2, b2 and answers (occl_curves_hidden, which explains no column): (B, G, P, R, hid)."""
    (B, G, P), R, hid = probs.shape, U.shape[0], base.shape[1]
    for t in (base, U, probs, score, cnull):
        _chk(t)
        assert t.is_contiguous()
    _chk(slot, torch.int32)
    assert score.shape == probs.shape and base.shape == (B, hid) and U.shape == (R, P, G, hid)
    assert cnull.numel() == B * G and slot.numel() == B
    if W2 is None:
        return B, G, P, R, hid
    A = W2.shape[0]
    _chk(b2), _chk(answers, torch.int32), _chk(W2)
    assert b2.is_contiguous() and answers.numel() == B
    assert W2.shape[1] == hid and b2.numel() == A and (hid == 1 or W2.stride(1) == 1)
    return B, G, P, R, hid, A, _ld(W2)


def occl_logit(base, Z, U, slot, probs, score, cnull, W2, b2, answers, logits, gh: int, gw: int, window: int, slot0: int = 0,
               out=None):
    """Occlusion maps [B, P] (include/vqa_hip.h vqa_occl_logit): maps[b, p] = logits[b, a_b] - the same logit with the window x
    window square of grid positions around p taken out of image slot[b].  base [B, hid], Z [B, G, hid], U [R, P, G, hid] (the
    rows slot0 .. slot0 + R - 1; a question whose slot is outside them is left alone), slot and answers device int32 [B], probs
    and score [B, G, P], cnull [B, G], W2 [A, hid] and logits [B, A] row-major views with unit column stride, b2 [A].  out:
    written in place."""
    B, G, P, R, hid, A, w2_ld = _occl_operands(base, U, slot, probs, score, cnull, W2, b2, answers)
    _chk(Z), _chk(logits)
    assert P == gh * gw and Z.shape == (B, G, hid) and Z.is_contiguous()
    assert logits.shape == (B, A) and (A == 1 or logits.stride(1) == 1)
    if out is None:
        out = torch.empty(B, P, dtype=torch.float32, device=probs.device)
    assert out.shape == (B, P) and out.is_contiguous() and out.dtype == torch.float32
    call("vqa_occl_logit", ptr(base), ptr(Z), ptr(U), ptr(slot), slot0, ptr(probs), ptr(score), ptr(cnull), ptr(W2), w2_ld,
         ptr(b2), ptr(answers), ptr(logits), _ld(logits), ptr(out), R, B, gh, gw, hid, G, A, window, stream())
    return out


RANK_MAX_P = 8192   # include/vqa_hip.h vqa_rank_desc: the row's keys live in LDS


def rank_desc(maps, out=None):
    """The positions of every row of maps fp32 [B, P] by descending value (include/vqa_hip.h vqa_rank_desc): int32 [B, P], equal
    values by the smaller position, -0.0 equal to +0.0, NaN last; a permutation of 0 .. P-1 for any input.  P <= 8192."""
    _chk(maps)
    assert maps.dim() == 2 and maps.is_contiguous()
    B, P = maps.shape
    if out is None:
        out = torch.empty(B, P, dtype=torch.int32, device=maps.device)
    assert out.shape == (B, P) and out.is_contiguous() and out.dtype == torch.int32
    call("vqa_rank_desc", ptr(maps), ptr(out), B, P, stream())
    return out


def occl_curves_chunk() -> int:
    """L: the steps per chunk of the ranking that vqa_occl_curves was built with."""
    return _lib.load().vqa_occl_curves_chunk()


def occl_curves_workspace_bytes(T: int, P: int, G: int, hid: int) -> int:
    """vqa_occl_curves_workspace_bytes(T, P, G, hid): the chunk sums of T walks -- T questions, or the T = B * M (question, order)
    pairs of vqa_occl_curves_orders, whose vqa_occl_curves_orders_workspace_bytes(B, M, ...) is the same formula."""
    return _lib.load().vqa_occl_curves_workspace_bytes(T, P, G, hid)


def occl_curves_workspace(B: int, P: int, G: int, hid: int, device):
    """A buffer of vqa_occl_curves_workspace_bytes(B, P, G, hid): the chunk sums of one call, freed with the call."""
    return torch.empty(max(occl_curves_workspace_bytes(B, P, G, hid) // 4, 4), dtype=torch.float32, device=device)


def _curves_buffers(order, rows: int, P: int, out, n_out: int, shape, workspace, walks: int, G: int, hid: int, device):
    """What the three curve wrappers ask beside _occl_operands: order int32 [rows, P]; out, n_out fp32 tensors of `shape`, made
    where None; workspace, a float32 buffer, made for `walks` walks where None.  Returns (out, workspace)."""
    _chk(order, torch.int32)
    assert order.shape == (rows, P) and order.is_contiguous()
    if out is None:
        out = tuple(torch.empty(shape, dtype=torch.float32, device=device) for _ in range(n_out))
    for t in out:
        assert t.shape == shape and t.is_contiguous() and t.dtype == torch.float32
    if workspace is None:
        workspace = occl_curves_workspace(walks, P, G, hid, device)
    _chk(workspace)
    assert workspace.is_contiguous()
    return out, workspace


def occl_curves(base, U, slot, probs, score, cnull, W2, b2, answers, order, slot0: int = 0, out=None, workspace=None):
    """Deletion and insertion curves (include/vqa_hip.h vqa_occl_curves): (deletion, insertion) fp32 [B, P+1], the logit of
    column answers[b] with the positions order[b, :k] absent / alone present, k = 0 .. P, in the kept form.  The operands are
    occl_logit's without Z, window and logits, plus order int32 [B, P].  out: (deletion, insertion), written in place for the
    questions whose slot is in [slot0, slot0 + R); workspace: a float32 buffer of at least vqa_occl_curves_workspace_bytes."""
    B, G, P, R, hid, A, w2_ld = _occl_operands(base, U, slot, probs, score, cnull, W2, b2, answers)
    (deletion, insertion), workspace = _curves_buffers(order, B, P, out, 2, (B, P + 1), workspace, B, G, hid, probs.device)
    call("vqa_occl_curves", ptr(base), ptr(U), ptr(slot), slot0, ptr(probs), ptr(score), ptr(cnull), ptr(W2), w2_ld, ptr(b2),
         ptr(answers), ptr(order), ptr(workspace), workspace.numel() * 4, ptr(deletion), ptr(insertion), R, B, P, hid, G, A,
         stream())
    return deletion, insertion


def occl_curves_hidden(base, U, slot, probs, score, cnull, order, slot0: int = 0, out=None, workspace=None):
    """The hidden rows of both curves (include/vqa_hip.h vqa_occl_curves_hidden): H fp32 [B, 2, P+1, hid], H[b, 0, k] = relu(base[b]
    + sum_g alpha * acc) of the kept set order[b, k:] (deletion), H[b, 1, k] of order[b, :k] (insertion), k = 0 .. P -- what
    occl_curves multiplies by one row of W2, for every column at once.  The operands are occl_curves' without W2, b2 and
    answers.  out: H, written in place for the questions whose slot is in [slot0, slot0 + R); workspace: as occl_curves'."""
    B, G, P, R, hid = _occl_operands(base, U, slot, probs, score, cnull)
    (out,), workspace = _curves_buffers(order, B, P, None if out is None else (out,), 1, (B, 2, P + 1, hid), workspace, B, G, hid,
                                        probs.device)
    call("vqa_occl_curves_hidden", ptr(base), ptr(U), ptr(slot), slot0, ptr(probs), ptr(score), ptr(cnull), ptr(order),
         ptr(workspace), workspace.numel() * 4, ptr(out), R, B, P, hid, G, stream())
    return out


def occl_curves_orders_workspace(B: int, M: int, P: int, G: int, hid: int, device):
    """A buffer of vqa_occl_curves_orders_workspace_bytes(B, M, P, G, hid): the chunk sums of one launch over M orders."""
    return occl_curves_workspace(B * M, P, G, hid, device)


def occl_curves_orders(base, U, slot, probs, score, cnull, W2, b2, answers, orders, slot0: int = 0, out=None, workspace=None):
    """occl_curves over (question, order) pairs (include/vqa_hip.h vqa_occl_curves_orders): (deletion, insertion) fp32
    [B, M, P+1], row (b, m) what occl_curves gives question b with orders[m] as its order, bit for bit.  The operands are
    occl_curves' with orders int32 [M, P], one table for every question, in place of order [B, P].  out and workspace (at least
    vqa_occl_curves_orders_workspace_bytes): as occl_curves'."""
    B, G, P, R, hid, A, w2_ld = _occl_operands(base, U, slot, probs, score, cnull, W2, b2, answers)
    assert orders.dim() == 2 and orders.shape[0] >= 1
    M = orders.shape[0]
    (deletion, insertion), workspace = _curves_buffers(orders, M, P, out, 2, (B, M, P + 1), workspace, B * M, G, hid, probs.device)
    call("vqa_occl_curves_orders", ptr(base), ptr(U), ptr(slot), slot0, ptr(probs), ptr(score), ptr(cnull), ptr(W2), w2_ld,
         ptr(b2), ptr(answers), ptr(orders), ptr(workspace), workspace.numel() * 4, ptr(deletion), ptr(insertion), R, B, M, P, hid,
         G, A, stream())
    return deletion, insertion


def shapley_accumulate(deletion, insertion, rank, slot, answers, state, A: int, R: int, slot0: int = 0, m0: int = 0, total: int = 0,
                       out=None, empty=None):
    """The curves of a group of orders folded into the running Shapley state (include/vqa_hip.h vqa_shapley_accumulate).
    deletion, insertion [B, Mg, P+1] from occl_curves_orders, rank int32 [Mg, P] the inverse of the group's orders, slot and
    answers device int32 [B]; state = (mean, M2) fp32 [B, P], updated in place (m0 == 0: started from zero); m0 the orders
    folded before.  total == m0 + Mg on the last group: out = (maps, stderr) fp32 [B, P] are written (made when None) and
    returned; otherwise total == 0 and None is returned.  empty (fp32 [B]) with m0 == 0: receives the logit of the empty image,
    insertion[:, 0, 0].  Questions whose slot is outside [slot0, slot0 + R) are left alone."""
    _chk(deletion), _chk(insertion), _chk(rank, torch.int32), _chk(slot, torch.int32), _chk(answers, torch.int32)
    B, Mg, P1 = deletion.shape
    P = P1 - 1
    assert insertion.shape == deletion.shape and deletion.is_contiguous() and insertion.is_contiguous()
    assert rank.shape == (Mg, P) and rank.is_contiguous() and slot.numel() == B and answers.numel() == B
    mean, m2 = state
    for t in state:
        _chk(t)
        assert t.shape == (B, P) and t.is_contiguous()
    assert total in (0, m0 + Mg)
    if empty is not None:
        _chk(empty)
        assert empty.numel() == B and empty.is_contiguous()
    if total and out is None:
        out = tuple(torch.empty(B, P, dtype=torch.float32, device=deletion.device) for _ in range(2))
    maps, err = out if total else (None, None)
    for t in (out if total else ()):
        _chk(t)
        assert t.shape == (B, P) and t.is_contiguous()
    call("vqa_shapley_accumulate", ptr(deletion), ptr(insertion), ptr(rank), ptr(slot), slot0, ptr(answers), ptr(mean), ptr(m2),
         ptr(maps), ptr(err), ptr(empty), R, B, P, Mg, m0, total, A, stream())
    return out if total else None


def lstm_occl_cell_fwd(xg_base, xg0, hg, h_var, c_var, q_len, var_b, var_t, s: int, n: Optional[int] = None, c_final=None,
                       cf_row=None):
    """One step, time s, of the variant recurrence of exact word occlusion (include/vqa_hip.h vqa_lstm_occl_cell_fwd), in place
    on the first n rows (default: all) of h_var / c_var [V, H] (row-major views with unit column stride and the same row
    stride): row r is the variant (var_b[r], var_t[r]) (device int32 [>= n]); held for s >= q_len[b], otherwise the cell on
    (xg0 if s == t else xg_base[s, b]) + hg[r].  xg_base [T, B, 4H] and hg [>= n, 4H] contiguous, xg0 [4H] (the base product's
    bits for a zero input row), q_len int64 [B].  c_final (a view [V, >= H] with unit column stride): the new cell state also
    goes to its row cf_row[r] (device int32, None: row r) on every active step."""
    T, B, H4 = xg_base.shape
    H = H4 // 4
    n = h_var.shape[0] if n is None else n
    for t in (xg_base, xg0, hg):
        _chk(t)
        assert t.is_contiguous()
    _chk(h_var), _chk(c_var), _chk(q_len, torch.int64), _chk(var_b, torch.int32), _chk(var_t, torch.int32)
    assert H4 == 4 * H and xg0.numel() == H4 and hg.dim() == 2 and hg.shape[1] == H4 and hg.shape[0] >= n and q_len.numel() == B
    assert h_var.dim() == 2 and h_var.shape == c_var.shape and h_var.shape[1] == H and 0 <= n <= h_var.shape[0]
    assert (H == 1 or (h_var.stride(1) == 1 and c_var.stride(1) == 1)) and var_b.numel() >= n and var_t.numel() >= n
    assert _ld(c_var) == _ld(h_var)
    cf_ld = 0
    if c_final is not None:
        _chk(c_final)
        assert c_final.dim() == 2 and c_final.shape[1] >= H and (c_final.shape[1] == 1 or c_final.stride(1) == 1)
        cf_ld = _ld(c_final)
        if cf_row is not None:
            _chk(cf_row, torch.int32)
            assert cf_row.numel() >= n
        else:
            assert c_final.shape[0] >= n
    else:
        assert cf_row is None
    call("vqa_lstm_occl_cell_fwd", ptr(xg_base), ptr(xg0), ptr(hg), ptr(h_var), ptr(c_var), _ld(h_var), ptr(q_len), ptr(var_b),
         ptr(var_t), s, ptr(c_final), cf_ld, ptr(cf_row), n, B, T, H, stream())


def occl_words(h1, W2, b2, answers, logits, var_b, var_t, q_len, out, b0: int = 0, nb: Optional[int] = None):
    """The tail of exact word occlusion (include/vqa_hip.h vqa_occl_words): out[b, t] = logits[b, a_b] - (W2[a_b] . h1[r] + b2[a_b])
    for the variant rows r = (var_b[r], var_t[r]) (device int32 [n]) and +0.0 for t >= q_len[b], for the questions b0 .. b0 + nb
    - 1 (default: all B) of out [B, T]: every element of those rows is written, no other row is touched.  h1 [n, hid], W2
    [A, hid] and logits [B, A] row-major views with unit column stride, b2 [A], answers device int32 [B] (a column outside
    [0, A): a row of zeros), q_len int64 [B]."""
    B, T = out.shape
    n, hid = h1.shape
    A = W2.shape[0]
    nb = B - b0 if nb is None else nb
    _chk(h1), _chk(W2), _chk(b2), _chk(logits), _chk(answers, torch.int32), _chk(q_len, torch.int64), _chk(out)
    _chk(var_b, torch.int32), _chk(var_t, torch.int32)
    assert out.is_contiguous() and W2.shape[1] == hid and b2.numel() == A and logits.shape == (B, A) and answers.numel() == B
    assert q_len.numel() == B and var_b.numel() == n and var_t.numel() == n and 0 <= b0 and 0 <= nb and b0 + nb <= B
    assert hid == 1 or (W2.stride(1) == 1 and h1.stride(1) == 1)
    assert A == 1 or logits.stride(1) == 1
    call("vqa_occl_words", ptr(h1), _ld(h1), ptr(W2), _ld(W2), ptr(b2), ptr(answers), ptr(logits), _ld(logits), ptr(var_b),
         ptr(var_t), ptr(q_len), ptr(out), n, b0, nb, T, hid, A, stream())
    return out


def att_apply_gather_fwd(score, vn, img, out, out_ld):
    """att_apply_fwd where sample b weights the rows of image img[b] (device int32 [B]); vn [N, P, C], fp32 or
    float16."""
    B, G, P, N, C = _apply_gather_head(score, vn, img)
    probs = torch.empty_like(score)
    call("vqa_att_apply_gather_fwd" + _cache_suffix(vn), ptr(score), ptr(vn), ptr(img), ptr(probs), ptr(out), out_ld, N, B, P, C, G, stream())
    return probs


def att_score_grouped_drop_fwd(vprime, qp, wx, bx, order, offsets, N: int, B: int, P: int, mode: int, p: float,
                               seed: int) -> torch.Tensor:
    """att_score_grouped_fwd with the x_conv dropout mask drop_scale(seed, (b*P + pos)*xld + m) on x (train mode); p = 0
    runs the same device code as att_score_grouped_fwd."""
    G, xld, mid, score = _grouped_score_head(vprime, qp, wx, order, offsets, N, B, P, mode, B)
    call("vqa_att_score_grouped_drop_fwd", ptr(vprime), ptr(qp), ptr(wx), xld, ptr(bx), ptr(order), ptr(offsets), ptr(score),
         N, B, P, mid, G, mode, p, seed, stream())
    return score


def att_apply_gather_bwd(dout, dout_ld, probs, vn, img, order, offsets, rowsum=None):
    """att_apply_bwd where sample b weighted the rows of image img[b] (vn [N, P, C]; img / order / offsets device int32):
    (dscore [B, G, P], dvn [N, P, C] = the weighted-sum branch of d loss / d vn summed over the questions of each image,
    zeros for an image without questions)."""
    B, G, P, N, C = _apply_gather_head(probs, vn, img)
    _chk(order, torch.int32), _chk(offsets, torch.int32)
    assert order.numel() == B and offsets.numel() == N + 1
    dscore = torch.empty_like(probs)
    dvn = torch.empty(N, P, C, dtype=torch.float32, device=vn.device)
    call("vqa_att_apply_gather_bwd", ptr(dout), dout_ld, ptr(probs), ptr(vn), ptr(img), ptr(order), ptr(offsets), ptr(dscore), ptr(dvn),
         ptr(rowsum), N, B, P, C, G, stream())
    return dscore, dvn


def att_score_grouped_bwd(dscore, vprime, qp, wx, order, offsets, N: int, B: int, P: int, mode: int, p: float, seed: int):
    """Backward of att_score_grouped_drop_fwd: (dvprime [N*P, mid], dq_part [B*NT, mid], dwx_part [N*NT, G*xld], NT);
    sum_parts(dq_part, out, B, NT, mid) and colsum(dwx_part, N*NT, G*xld, out) finish d loss / d q' and d loss / d wx."""
    G, xld, mid = _score_dims(wx, mode == 2)
    _chk(order, torch.int32), _chk(offsets, torch.int32)
    assert order.numel() == B and offsets.numel() == N + 1 and vprime.shape == (N * P, mid) and qp.shape == (B, mid)
    assert dscore.shape == (B, G, P) and dscore.is_contiguous()
    NT = _lib.load().vqa_att_score_grouped_tiles(P)
    dev = vprime.device
    dvprime = torch.empty(N * P, mid, dtype=torch.float32, device=dev)
    dq_part = torch.empty(B * NT, mid, dtype=torch.float32, device=dev)
    dwx_part = torch.empty(N * NT, G * xld, dtype=torch.float32, device=dev)
    call("vqa_att_score_grouped_bwd", ptr(dscore), ptr(vprime), ptr(qp), ptr(wx), xld, ptr(order), ptr(offsets), ptr(dvprime),
         ptr(dq_part), ptr(dwx_part), N, B, P, mid, G, mode, p, seed, stream())
    return dvprime, dq_part, dwx_part, NT


def att_apply_bwd(dout, dout_ld, probs, vn, dvn_out=None, rowsum=None, want_dvn=True):
    """rowsum: optional [B, G] output, sum over positions of dscore (per-sample x_conv bias gradient).
    want_dvn=False: the weighted-sum branch of d loss / d vn is not written (l2norm_bwd_joined recomputes it)."""
    B, G, P = probs.shape
    C = vn.shape[-1]
    dscore = torch.empty_like(probs)
    dvn = (dvn_out if dvn_out is not None else torch.empty_like(vn)) if want_dvn else None
    call("vqa_att_apply_bwd", ptr(dout), dout_ld, ptr(probs), ptr(vn), ptr(dscore), ptr(dvn), ptr(rowsum), B, P, C, G,
         stream())
    return dscore, dvn


def softce(logits, ld, a_idx, a_val, A, inv_batch, dlogits=None, dld=0):
    B = logits.shape[0]
    kmax = a_idx.shape[1]
    loss_rows = torch.empty(B, dtype=torch.float32, device=logits.device)
    score_rows = torch.empty(B, dtype=torch.float32, device=logits.device)
    call("vqa_softce_fwd_bwd", ptr(logits), ld, ptr(a_idx), ptr(a_val), kmax, B, A, inv_batch, ptr(loss_rows),
         ptr(score_rows), ptr(dlogits), dld, stream())
    return loss_rows, score_rows


def softmax_topk(logits: torch.Tensor, k: int, want_lse: bool = False):
    """(idx int32 [B,k], prob fp32 [B,k][, lse fp32 [B]]): the first k columns of every row -- larger value first, equal
    values by smaller column (the score kernel's arg-max rule), NaN above +inf -- with their softmax probabilities, in one
    launch (include/vqa_hip.h vqa_softmax_topk).  logits: any 2-D fp32 CUDA tensor with stride(1) == 1; a row view into a
    padded buffer is read in place (ld = stride(0))."""
    _chk(logits)
    assert logits.dim() == 2 and (logits.shape[1] == 1 or logits.stride(1) == 1), (tuple(logits.shape), logits.stride())
    B, A = logits.shape
    idx = torch.empty(B, k, dtype=torch.int32, device=logits.device)
    prob = torch.empty(B, k, dtype=torch.float32, device=logits.device)
    lse = torch.empty(B, dtype=torch.float32, device=logits.device) if want_lse else None
    call("vqa_softmax_topk", ptr(logits), _ld(logits), B, A, k, ptr(idx), ptr(prob), ptr(lse), stream())
    return (idx, prob, lse) if want_lse else (idx, prob)


def softmax_pick(logits: torch.Tensor, answers: torch.Tensor, rows_per_question: int, out=None):
    """(top int32 [R], top_prob fp32 [R], prob_at fp32 [R]) of the logits rows [R, A] (include/vqa_hip.h vqa_softmax_pick): top
    and top_prob are softmax_topk(logits, 1)'s, bit for bit; prob_at[r] = softmax(logits[r])[answers[r // rows_per_question]],
    +0.0 for a column outside [0, A).  answers: device int32 [R // rows_per_question].  logits: as softmax_topk's, a row view
    into a padded buffer included.  out: (top, top_prob, prob_at), contiguous with R elements each, written in place."""
    _chk(logits), _chk(answers, torch.int32)
    assert logits.dim() == 2 and (logits.shape[1] == 1 or logits.stride(1) == 1), (tuple(logits.shape), logits.stride())
    R, A = logits.shape
    assert rows_per_question >= 1 and R % rows_per_question == 0 and answers.numel() == R // rows_per_question
    assert answers.is_contiguous()
    if out is None:
        out = (torch.empty(R, dtype=torch.int32, device=logits.device), torch.empty(R, dtype=torch.float32, device=logits.device),
               torch.empty(R, dtype=torch.float32, device=logits.device))
    top, top_prob, prob_at = out
    _chk(top, torch.int32), _chk(top_prob), _chk(prob_at)
    assert all(t.numel() == R and t.is_contiguous() for t in out)
    call("vqa_softmax_pick", ptr(logits), _ld(logits), R, A, ptr(answers), rows_per_question, ptr(top), ptr(top_prob), ptr(prob_at),
         stream())
    return top, top_prob, prob_at


def colsum(x: torch.Tensor, rows: int, cols: int, out: torch.Tensor, *, ld=None, mask=None, accumulate=False):
    lib = _lib.load()
    nbytes = lib.vqa_colsum_workspace_bytes(rows, cols)
    ws = workspace(nbytes, x.device)
    call("vqa_colsum", ptr(x), ld if ld is not None else cols, ptr(mask), rows, cols, ptr(out), int(accumulate),
         ptr(ws), ws.numel() * 4, stream())
    return out


def sum_bgp(x: torch.Tensor, out: torch.Tensor):
    B, G, P = x.shape
    call("vqa_sum_bgp", ptr(x), ptr(out), B, G, P, stream())
    return out


def sum_parts(part: torch.Tensor, out: torch.Tensor, batch: int, parts: int, cols: int):
    call("vqa_sum_parts", ptr(part), ptr(out), batch, parts, cols, stream())
    return out


def relu_drop_bwd(y, dy, dx, p: float, seed: int):
    call("vqa_relu_drop_bwd", ptr(y), ptr(dy), ptr(dx), y.numel(), p, seed, stream())
    return dx


def add2d(a, lda, b, ldb, out, ldo, rows, cols):
    """out[r, c] = a[r, c] + (b[r, c] if b is not None else 0) on strided row-major views."""
    call("vqa_add2d", ptr(a), lda, ptr(b), ldb, ptr(out), ldo, rows, cols, stream())
    return out


def add(a, b, out):
    return add2d(a, a.numel(), b, a.numel(), out, a.numel(), 1, a.numel())


def half_to_float(x: torch.Tensor) -> torch.Tensor:
    """fp16 image features -> fp32 on the device, layout unchanged (reference: host-side cast in
    preprocessing/data_preprocessing.py:167-176)."""
    assert x.dtype == torch.float16 and x.is_contiguous()
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    call("vqa_half_to_float", ptr(x), ptr(y), x.numel(), stream())
    return y


def to_half(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 -> float16 on the device, layout unchanged: round to nearest even, overflow to +-inf, NaN kept, subnormals kept
    (what torch's .half() gives).  The one rounding of a float16 image-feature cache.  out: a contiguous float16 tensor of
    x's element count to write into."""
    _chk(x)
    assert x.is_contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    assert out.is_cuda and out.dtype == torch.float16 and out.is_contiguous() and out.numel() == x.numel()
    call("vqa_float_to_half", ptr(x), ptr(out), x.numel(), stream())
    return out


# ---------------------------------------------------------------------------- image preprocessing (csrc/preprocess.hip)
def last_error() -> str:
    return _lib.load().vqa_last_error().decode()


def preprocess_supported(desc, coef, S: int) -> int:
    """Band height the preprocessing kernel would use for the batch that desc / coef (dl_vqa_amd.preprocess.build_plan: HOST
    numpy arrays) describe, 0 when it does not cover it (last_error() says why).  Host code only: needs no GPU."""
    assert desc.dtype.itemsize == 56 and coef.dtype.kind == "i" and coef.dtype.itemsize == 4
    assert desc.flags.c_contiguous and coef.flags.c_contiguous
    return _lib.load().vqa_preprocess_supported(desc.ctypes.data, coef.ctypes.data, coef.size, len(desc), S)


def preprocess_images(src: torch.Tensor, src_bytes: int, desc, coef, desc_dev: torch.Tensor, coef_dev: torch.Tensor, S: int,
                      lut: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out [N,3,S,S] (fp16 or fp32) from the packed uint8 source buffer src, one launch (include/vqa_hip.h
    vqa_preprocess_images).  desc / coef are the host plan (numpy), desc_dev / coef_dev its device copy (uint8 views of the
    same bytes); lut is the [3,256] table of out's dtype on the device."""
    N = len(desc)
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous() and src.numel() >= src_bytes
    assert desc.dtype.itemsize == 56 and desc.flags.c_contiguous and coef.dtype.itemsize == 4 and coef.flags.c_contiguous
    assert desc_dev.is_cuda and desc_dev.numel() * desc_dev.element_size() == desc.nbytes
    assert coef_dev.is_cuda and coef_dev.numel() * coef_dev.element_size() == coef.nbytes
    assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == (N, 3, S, S) and out.dtype in (torch.float16, torch.float32)
    assert lut.is_cuda and lut.is_contiguous() and lut.dtype == out.dtype and tuple(lut.shape) == (3, 256)
    call("vqa_preprocess_images", ptr(src), src_bytes, desc.ctypes.data, coef.ctypes.data, coef.size, ptr(desc_dev),
         ptr(coef_dev), N, S, ptr(lut), int(out.dtype == torch.float32), ptr(out), stream())
    return out


# ---------------------------------------------------------------------------- bf16 path (BASELINE configs[3])
def to_bf16(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 -> bf16 copy (round to nearest even) by the library's converter."""
    assert x.dtype == torch.float32 and x.is_contiguous()
    y = out if out is not None else torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    call("vqa_f32_to_bf16", ptr(x), ptr(y), x.numel(), stream())
    return y


def dropout_to_bf16(x: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    call("vqa_dropout_to_bf16", ptr(x), ptr(y), x.numel(), p, seed, stream())
    return y


def to_f32(x: torch.Tensor) -> torch.Tensor:
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    call("vqa_bf16_to_f32", ptr(x), ptr(y), x.numel(), stream())
    return y


def to_bf16_transposed(x: torch.Tensor) -> torch.Tensor:
    """[rows, cols] fp32 -> [cols, rows] bf16."""
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    rows, cols = x.shape
    y = torch.empty(cols, rows, dtype=torch.bfloat16, device=x.device)
    call("vqa_f32_to_bf16_transpose", ptr(x), ptr(y), rows, cols, stream())
    return y


def gemm_bf16(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, M: int, N: int, K: int, *, transA=False, transB=True,
              lda=None, ldb=None, ldc=None, bias1=None, bias2=None, rowgroup=None, rg_div=1, rg_op=0, relu=False,
              accumulate=False, aux=None, tag=0) -> torch.Tensor:
    """vqa_gemm with bf16 A / B (fp32 accumulation); C fp32 or bf16 by its dtype."""
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and C.dtype in (torch.float32, torch.bfloat16)
    return _gemm("vqa_gemm_bf16", (int(C.dtype == torch.bfloat16),), A, B, C, M, N, K, transA, transB, lda, ldb, ldc, bias1, bias2,
                 rowgroup, rg_div, rg_op, relu, accumulate, aux, tag)


def gemm_tall_bf16_supported(M: int, N: int, K: int, rg_div: int = 0, has_rowgroup: bool = False) -> bool:
    return bool(_lib.load().vqa_gemm_tall_bf16_supported(M, N, K, rg_div, int(has_rowgroup)))


GEMM_TALL_PLAN_FIELDS = ("BM", "tiles_m", "tiles_n", "grid", "nk")


def gemm_tall_bf16_plan(M: int, N: int, K: int) -> dict:
    """The launch geometry of vqa_gemm_tall_bf16 for this shape under the VQA_TALL_BM knob in force, from the query its launcher
    calls (vqa_gemm_tall_bf16_plan); makes no HIP call.  grid: workgroups; workgroup w walks tiles w, w + grid, ..."""
    import ctypes
    out = (ctypes.c_int32 * len(GEMM_TALL_PLAN_FIELDS))()
    call("vqa_gemm_tall_bf16_plan", M, N, K, out, len(out))
    return dict(zip(GEMM_TALL_PLAN_FIELDS, out))


def gemm_tall_bf16(A: torch.Tensor, W: torch.Tensor, C: torch.Tensor, M: int, N: int, K: int, *, rowgroup=None, rg_div=1,
                   rg_op=0, relu=False, tag=0) -> torch.Tensor:
    """C [M,N] bf16 = act(A [M,K] . W [N,K]^T (+|*) rowgroup[row // rg_div]) on persistent 256 x 128 tiles (short K)."""
    assert A.dtype == torch.bfloat16 and W.dtype == torch.bfloat16 and C.dtype == torch.bfloat16
    call("vqa_gemm_tall_bf16", ptr(A), A.stride(0), ptr(W), W.stride(0), ptr(C), C.stride(0), M, N, K, ptr(rowgroup),
         (rowgroup.stride(0) if rowgroup is not None else 0), rg_div, rg_op, int(relu), tag, stream())
    return C


def conv_pack_weights_bf16(w: torch.Tensor, CiP: int, need_wd: bool = True):
    """fp32 [Co,Ci,3,3] -> bf16 wfT [Co, 9*CiP] and wdT [CiP, 9*Co] (K index = (tap, channel))."""
    Co, Ci = w.shape[0], w.shape[1]
    wfT = torch.empty(Co, 9 * CiP, dtype=torch.bfloat16, device=w.device)
    wdT = torch.empty(CiP, 9 * Co, dtype=torch.bfloat16, device=w.device) if need_wd else None
    call("vqa_conv_pack_weights_bf16", ptr(w), ptr(wfT), ptr(wdT), Co, Ci, CiP, stream())
    return wfT, wdT


def conv_fwd_bf16(x: torch.Tensor, wfT: torch.Tensor, bias: torch.Tensor, stride: int = 1, out_dtype=torch.bfloat16,
                  tag: int = 0):
    """x NHWC bf16 [B,H,W,CiP] -> (pooled [B,Hp,Wp,Co] bf16 or fp32, argmax uint8)."""
    assert x.dtype == torch.bfloat16 and wfT.dtype == torch.bfloat16
    B, H, W, CiP = x.shape
    Co = wfT.shape[0]
    Hp, Wp = conv_out_hw(H, W, stride)
    pooled = torch.empty(B, Hp, Wp, Co, dtype=out_dtype, device=x.device)
    amax = torch.empty(B, Hp, Wp, Co, dtype=torch.uint8, device=x.device)
    call("vqa_conv3x3_relu_pool_fwd_bf16", ptr(x), ptr(wfT), ptr(bias), ptr(pooled), int(out_dtype == torch.bfloat16),
         ptr(amax), B, H, W, CiP, Co, stride, tag, stream())
    return pooled, amax


def conv_dgrad_bf16(dpooled, amax, wdT, x_shape, stride: int = 1, out_dtype=torch.bfloat16, tag: int = 0):
    assert dpooled.dtype == torch.bfloat16
    B, H, W, CiP = x_shape
    Co = dpooled.shape[3]
    dx = torch.empty(B, H, W, CiP, dtype=out_dtype, device=dpooled.device)
    call("vqa_conv3x3_dgrad_bf16", ptr(dpooled), ptr(amax), ptr(wdT), ptr(dx), int(out_dtype == torch.bfloat16), B, H, W,
         CiP, Co, stride, tag, stream())
    return dx


def conv_wgrad_bf16(x, dpooled, amax, dw: torch.Tensor, dbias: torch.Tensor, stride: int = 1, tag: int = 0):
    assert x.dtype == torch.bfloat16 and dpooled.dtype == torch.bfloat16
    lib = _lib.load()
    B, H, W, CiP = x.shape
    Co, Ci = dw.shape[0], dw.shape[1]
    ws = workspace(lib.vqa_conv3x3_wgrad_bf16_workspace_bytes(B, H, W, CiP, Co, stride), x.device)
    call("vqa_conv3x3_wgrad_bf16", ptr(x), ptr(dpooled), ptr(amax), ptr(dw), ptr(dbias), B, H, W, CiP, Ci, Co, stride,
         ptr(ws), ws.numel() * 4, tag, stream())


# ------------------------------------------------------------------ fp32 patch backward-data (csrc/conv_patch_f32.hip)
def pconvf_supported(H: int, W: int, Ci: int, Co: int, stride: int = 1) -> bool:
    return bool(_lib.load().vqa_pconvf_supported(H, W, Ci, Co, stride))


def pconvf_pack_weights(w: torch.Tensor) -> torch.Tensor:
    """fp32 [Co,Ci,3,3] -> the flipped, transposed, fragment-ordered fp32 image pconvf_dgrad reads."""
    Co, Ci = w.shape[0], w.shape[1]
    wd = torch.empty(9 * Ci * Co, dtype=torch.float32, device=w.device)
    call("vqa_pconvf_pack_weights", ptr(w), ptr(wd), Co, Ci, stream())
    return wd


def pconvf_dgrad(dpooled: torch.Tensor, amax: torch.Tensor, wd_img: torch.Tensor, x_shape, tag: int = 0, out=None) -> torch.Tensor:
    """dpooled fp32 NHWC [B,Hp,Wp,Co] + arg-max bytes NHWC -> dX fp32 NHWC; x_shape = (B, H, W, Ci) of the block's input."""
    B, H, W, Ci = x_shape
    Co = dpooled.shape[3]
    assert dpooled.dtype == torch.float32 and dpooled.is_contiguous() and amax.dtype == torch.uint8 and amax.is_contiguous()
    assert tuple(dpooled.shape[1:3]) == conv_out_hw(H, W, 1) and amax.shape == dpooled.shape
    dx = out if out is not None else torch.empty(B, H, W, Ci, dtype=torch.float32, device=dpooled.device)
    call("vqa_pconvf_dgrad", ptr(dpooled), ptr(amax), ptr(wd_img), ptr(dx), B, H, W, Ci, Co, tag, stream())
    return dx


# ------------------------------------------------------------------ bf16 patch convolutions (csrc/conv_patch_bf16.hip)
# Everything a patch is cut from lives in HBM channel-blocked, "C16" = [B][C/16][H][W][16] bf16 (a K-slice of a patch row is
# one contiguous run); pooled fp32 outputs, dX, pooled gradients and arg-max bytes stay NHWC.
def to_c16(x_nhwc: torch.Tensor) -> torch.Tensor:
    """NHWC -> C16 by torch (tests / tools; the kernels write C16 themselves)."""
    B, H, W, C = x_nhwc.shape
    return x_nhwc.view(B, H, W, C // 16, 16).permute(0, 3, 1, 2, 4).contiguous()


def from_c16(x_c16: torch.Tensor) -> torch.Tensor:
    B, Cb, H, W, _ = x_c16.shape
    return x_c16.permute(0, 2, 3, 1, 4).reshape(B, H, W, Cb * 16).contiguous()


def pconv_supported(H: int, W: int, Ci: int, Co: int, stride: int = 1) -> bool:
    return bool(_lib.load().vqa_pconv_supported(H, W, Ci, Co, stride))


def pconv_pack_weights(w: torch.Tensor, need_wd: bool = True):
    """fp32 [Co,Ci,3,3] -> fragment-ordered bf16 images (forward; flipped + transposed for backward-data)."""
    Co, Ci = w.shape[0], w.shape[1]
    n = 9 * Ci * Co
    wf = torch.empty(n, dtype=torch.bfloat16, device=w.device)
    wd = torch.empty(n, dtype=torch.bfloat16, device=w.device) if need_wd else None
    call("vqa_pconv_pack_weights", ptr(w), ptr(wf), ptr(wd), Co, Ci, stream())
    return wf, wd


def pconv_fwd(x: torch.Tensor, wf_img: torch.Tensor, bias: torch.Tensor, Co: int, out_dtype=torch.bfloat16, tag: int = 0):
    """x C16 bf16 [B,Ci/16,H,W,16] -> (pooled: bf16 C16 [B,Co/16,Hp,Wp,16] or fp32 NHWC [B,Hp,Wp,Co]; argmax uint8 C16)."""
    assert x.dtype == torch.bfloat16 and wf_img.dtype == torch.bfloat16 and x.is_contiguous() and x.dim() == 5
    B, Cb, H, W, _ = x.shape
    Hp, Wp = conv_out_hw(H, W, 1)
    if out_dtype == torch.bfloat16:
        pooled = torch.empty(B, Co // 16, Hp, Wp, 16, dtype=torch.bfloat16, device=x.device)
    else:
        pooled = torch.empty(B, Hp, Wp, Co, dtype=out_dtype, device=x.device)
    amax = torch.empty(B, Co // 16, Hp, Wp, 16, dtype=torch.uint8, device=x.device)
    call("vqa_pconv_fwd", ptr(x), ptr(wf_img), ptr(bias), ptr(pooled), int(out_dtype == torch.bfloat16), ptr(amax),
         B, H, W, Cb * 16, Co, tag, stream())
    return pooled, amax


def pconv_dgrad(dpooled: torch.Tensor, amax: torch.Tensor, wd_img: torch.Tensor, x_shape, out_dtype=torch.bfloat16,
                out_c16: bool = False, tag: int = 0):
    """Pooled gradient (bf16 C16 [B,Co/16,Hp,Wp,16]) + arg-max bytes (C16) -> dX of the block whose input is x_shape =
    (B, H, W, Ci): NHWC (bf16 or fp32), or bf16 C16 (the pooled gradient of the block below).  The pre-pool gradient is routed
    inside the kernel."""
    B, H, W, Ci = x_shape
    assert dpooled.dtype == torch.bfloat16 and dpooled.dim() == 5 and dpooled.is_contiguous() and dpooled.shape[0] == B
    assert amax.dtype == torch.uint8 and amax.shape == dpooled.shape and amax.is_contiguous()
    assert tuple(dpooled.shape[2:4]) == conv_out_hw(H, W, 1)
    Co = dpooled.shape[1] * 16
    if out_c16:
        assert out_dtype == torch.bfloat16
        dx = torch.empty(B, Ci // 16, H, W, 16, dtype=torch.bfloat16, device=dpooled.device)
    else:
        dx = torch.empty(B, H, W, Ci, dtype=out_dtype, device=dpooled.device)
    mode = 2 if out_c16 else int(out_dtype == torch.bfloat16)
    call("vqa_pconv_dgrad", ptr(dpooled), ptr(amax), ptr(wd_img), ptr(dx), mode, B, H, W, Ci, Co, tag, stream())
    return dx


def pconv_wgrad_supported(H: int, W: int, Ci: int, Co: int) -> bool:
    return bool(_lib.load().vqa_pconv_wgrad_supported(H, W, Ci, Co))


def pconv_wgrad(x, dpooled, amax, dw: torch.Tensor, dbias: torch.Tensor, tag: int = 0):
    """dw [Co,Ci,3,3], dbias [Co] (fp32) from x (C16 bf16), the pooled gradient (C16 bf16) and the arg-max bytes (C16)."""
    assert x.dtype == torch.bfloat16 and dpooled.dtype == torch.bfloat16 and amax.dtype == torch.uint8
    assert x.is_contiguous() and dpooled.is_contiguous() and amax.is_contiguous() and amax.shape == dpooled.shape
    lib = _lib.load()
    B, Cib, H, W, _ = x.shape
    Ci, Co = Cib * 16, dpooled.shape[1] * 16
    assert tuple(dpooled.shape[2:4]) == conv_out_hw(H, W, 1) and dpooled.shape[0] == B
    ws = workspace(lib.vqa_pconv_wgrad_workspace_bytes(B, H, W, Ci, Co), x.device)
    call("vqa_pconv_wgrad", ptr(x), ptr(dpooled), ptr(amax), ptr(dw), ptr(dbias), B, H, W, Ci, Co, ptr(ws), ws.numel() * 4, tag,
         stream())


def scale_by(x, scalar_dev):
    call("vqa_scale_by", ptr(x), x.numel(), ptr(scalar_dev), stream())
    return x


def adam(param, grad, exp_avg, exp_avg_sq, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    call("vqa_adam", ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), lr, beta1, beta2, eps,
         step, grad_scale, stream())


ADAM_SEGMENT_FIELDS = ("begin", "end", "lr", "beta1", "beta2", "eps", "weight_decay", "step", "decoupled")


def adam_segment_table(segments):
    """The host array vqa_adam_segments reads, from a list of segments: each a tuple in the order of ADAM_SEGMENT_FIELDS
    (beta1 onwards may be left out: 0.9, 0.999, 1e-8, no decay, step 1, not decoupled) or a dict with those keys."""
    defaults = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, decoupled=0)
    table = (_lib.AdamSegment * len(segments))()
    for row, s in zip(table, segments):
        if not isinstance(s, dict):
            s = dict(zip(ADAM_SEGMENT_FIELDS, s))
        unknown = set(s) - set(ADAM_SEGMENT_FIELDS)
        if unknown or not {"begin", "end", "lr"} <= set(s):
            raise ValueError(f"adam_segments: a segment needs begin, end, lr and may have {ADAM_SEGMENT_FIELDS[3:]}; got {sorted(s)}")
        s = {**defaults, **s}
        row.begin, row.end, row.step, row.decoupled = int(s["begin"]), int(s["end"]), int(s["step"]), int(bool(s["decoupled"]))
        row.lr, row.beta1, row.beta2, row.eps, row.weight_decay = s["lr"], s["beta1"], s["beta2"], s["eps"], s["weight_decay"]
    return table


def adam_segments(param, grad, exp_avg, exp_avg_sq, segments, grad_scale=1.0):
    """Adam / AdamW over the listed ranges of the flat buffers in ONE launch (vqa_adam_segments); every range has its own
    step, lr, betas, eps and weight decay, and what no range covers is not touched.  `segments`: see adam_segment_table."""
    table = adam_segment_table(segments)
    call("vqa_adam_segments", ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), table, len(table),
         grad_scale, stream())
