"""Forward / backward schedule of the VqaNet hot path over the HIP kernels.

This is the host-side mirror of ``models/model.py:53-67`` (VqaNet.forward) and of what autograd
would do for it: a fixed sequence of C-ABI calls (dl_vqa_amd.ops) on torch's current HIP stream.
torch only provides the buffers.  Layouts: images NHWC (channels padded to 4), question
activations time-major [T][B][*], the classifier input `combined` = [weighted v | c_fwd | c_bwd].
"""
from __future__ import annotations

import functools
import inspect
import os
from collections import namedtuple
from types import SimpleNamespace
from typing import Callable, Dict, Optional

import torch

from . import ops

Tensor = torch.Tensor

# dropout sites (models/model.py:84,156,185,186,194,201,204)
SITE_IMAGE, SITE_TEXT, SITE_ATT_V, SITE_ATT_Q, SITE_ATT_X, SITE_CLS1, SITE_CLS2 = 1, 2, 3, 4, 5, 6, 7
_MASK64 = (1 << 64) - 1


def _site_seed(base: int, site: int) -> int:
    return (base * 0x9E3779B97F4A7C15 + site * 0xD1B54A32D192ED03 + 0x632BE59BD9B4E019) & _MASK64


_SFX = ("", "_reverse")     # parameter-name suffix of LSTM direction d

# what Engine.conv_routes decides for one conv block; both passes read it
ConvRoute = namedtuple("ConvRoute", "kind x_shape Co src out dy dx x3 pdg pack_in need_wd")
_OUT16 = {"nhwc32": torch.float32, "nhwc16": torch.bfloat16, "c16": torch.bfloat16}     # a bf16 block's out_dtype by route.out


def _gemm(A, B, C, M, N, K, x3=False, **kw):
    """One dense product C[M,N] = op(A) op(B), by the form its operands are in: bf16 A and B take the bf16 MFMA GEMM
    (fp32 accumulation), fp32 operands the fp32 GEMM (x3: the split GEMM).  Arguments as ops.gemm."""
    if A.dtype == torch.bfloat16:
        assert not x3
        return ops.gemm_bf16(A, B, C, M, N, K, **kw)
    return ops.gemm(A, B, C, M, N, K, x3=x3, **kw)


def _device_current(name: str, device=lambda x: x.device):
    """Decorator of an Engine schedule: the argument called `name` says where the schedule's tensors live (device(argument):
    a tensor's device unless told otherwise), and that device is current while the schedule runs."""
    def deco(schedule):
        pos = list(inspect.signature(schedule).parameters).index(name) - 1      # behind self

        @functools.wraps(schedule)
        def guarded(self, *args, **kw):
            with torch.cuda.device(device(args[pos] if pos < len(args) else kw[name])):
                return schedule(self, *args, **kw)
        return guarded
    return deco


_cache_device = lambda feats: feats.vn.device       # of an ImageFeatures


class Engine:
    def __init__(self, cfg: dict, embedding_tokens: int, compute_dtype: str = "fp32"):
        t, i, a, c = cfg["text"], cfg["image"], cfg["attention"], cfg["classifier"]
        self.V = embedding_tokens
        self.E = t["embedding_features"]
        self.H = t["question_features"]
        self.ndir = 2 if t["bidirectional"] else 1
        if t["num_lstm_layers"] != 1:
            raise NotImplementedError("num_lstm_layers != 1 (the reference notes it 'needs change of code' too, "
                                      "config.yaml:55)")
        self.channels = list(i["num_channels"])
        self.L = len(self.channels) - 1
        self.stride = i["stride"]
        # kernel_size 3 (config.yaml:58) has the implicit-GEMM / patch kernels; any other size the schema admits
        # (utils/config_schema.py:59) takes the materialised im2col + GEMM form (csrc/conv_generic.hip), fp32 only
        self.ks = int(i["kernel_size"])
        if not 1 <= self.ks <= 15:
            raise ValueError(f"image.kernel_size={self.ks}: 1..15")
        self.mid = a["hidden_dim"]
        self.G = a["glimpses"]
        self.do_option = a["do_option"]
        if self.do_option not in ("+", "*", "|"):
            raise ValueError(f"attention do_option {self.do_option!r} (the reference knows '+', '*', '|')")
        self.att_mode = {"+": 0, "*": 1, "|": 2}[self.do_option]
        self.hid = c["hidden_dim"]
        self.A = cfg["max_answers"]
        self.p_text, self.p_image, self.p_att, self.p_cls = t["dropout"], i["dropout"], a["dropout"], c["dropout"]
        self.C = self.channels[-1]
        self.Q = self.ndir * self.H
        self.GC = self.G * self.C
        self.Dc = self.GC + self.Q
        for name, val in (("embedding_features", self.E), ("question_features", self.H), ("hidden_dim(att)", self.mid),
                          ("hidden_dim(cls)", self.hid)) + tuple((f"num_channels[{k}]", ch) for k, ch in
                                                                 enumerate(self.channels[1:], 1)):
            if val % 4:
                raise ValueError(f"{name}={val}: the HIP kernels need multiples of 4 (16-byte vector loads)")
        if self.channels[0] > 4:
            raise ValueError("input images with more than 4 channels are not supported")
        # bf16 path (BASELINE configs[3]): conv blocks 1.. and the v_conv products on bf16 MFMA (fp32 accumulate),
        # activations between the conv blocks stored as bf16; parameters, LSTM, reductions and the optimiser stay
        # fp32.  Opt-in; fp32 is the parity path.
        # fp32x3: the same fp32 tensors everywhere, but the conv blocks' contractions run on the bf16 matrix cores with every
        # fp32 operand split exactly into three bf16 terms (csrc/x3_core.hpp) -- fp32-level accuracy, opt-in.
        if compute_dtype not in ("fp32", "bf16", "fp32x3"):
            raise ValueError(f"compute_dtype {compute_dtype!r} (fp32, fp32x3 or bf16)")
        if self.ks != 3 and compute_dtype != "fp32":
            raise ValueError(f"compute_dtype {compute_dtype!r} needs image.kernel_size=3 (kernel_size={self.ks} runs in fp32)")
        self.bf16 = compute_dtype == "bf16"
        self.x3 = compute_dtype == "fp32x3"
        self.x3_gemm = self.x3 and os.environ.get("VQA_X3_GEMM", "1") != "0"     # diagnostic switch, read once
        # bf16 path: q_lin / lin1 / lin2 on bf16 MFMA too (BASELINE configs[3] "bf16 conv/FC") when every dimension is a multiple
        # of 8 (16-byte operand rows); VQA_FC16=0 keeps them on the fp32 GEMM
        self.fc16 = (self.bf16 and os.environ.get("VQA_FC16", "1") != "0"
                     and all(d % 8 == 0 for d in (self.Q, self.mid, self.Dc, self.hid, self.A)))
        # bf16 path: the LSTM's non-recurrent products (xg = x . W_ih^T, dW_hh, dW_ih, dx) on bf16 MFMA, operands staged as bf16,
        # fp32 accumulation ("bf16 conv/FC + fp32 LSTM accumulate"); the recurrence stays fp32.  VQA_LSTM16=0: all fp32
        self.lstm16 = self.bf16 and os.environ.get("VQA_LSTM16", "1") != "0" and self.H % 8 == 0
        if self.bf16:
            if self.L < 2 or any(ch % 64 for ch in self.channels[1:]) or self.mid % 8 or self.stride != 1:
                raise ValueError("the bf16 path needs >= 2 conv blocks, stride 1 and channel counts that are multiples "
                                 f"of 64 after the first block (num_channels={self.channels}, stride={self.stride})")
        self._sides = {}        # the side stream of each device (_on_side_stream)

    def conv_routes(self, v_shape, keep: bool, need_dx: bool = False):
        """The kernel family of every conv block for an image batch of v_shape [B,C,H,W], decided once for both passes: one
        ConvRoute per block (the table in DESIGN.md, "Conv routes").  Makes no launch and allocates nothing.
        kind: convk (kernel_size != 3), conv0 (dedicated first block), pconv (bf16 patch), conv16 (bf16 implicit GEMM) or conv32
        (fp32 implicit GEMM; x3: split kernels; pdg: patch backward-data; pack_in: x3-packs its own input, the producer could
        not).  x_shape: the NHWC input.  Layouts nchw / nhwc32 / nhwc16 / x3 / c16: src and out of input and pooled output, dy
        of the pooled gradient backward reads, dx of the input gradient it writes (None: none).  need_wd: forward packs the
        backward-data weights (a pdg block the patch image instead; wds[l] is a tensor or None)."""
        B, C, H, W = v_shape
        L, ch, bf16 = self.L, self.channels, self.bf16
        # the first block has a dedicated kernel that reads the NCHW image as is (K = 27 is too thin for the generic implicit
        # GEMM), fp16 features included; otherwise the image is converted to NHWC4 once
        fast0 = self.ks == 3 and ops.conv0_supported(C, H, W, ch[1], self.stride)
        if bf16 and not fast0:
            raise ValueError("the bf16 path needs the dedicated first-block kernel (3-channel NCHW image, "
                             "W % 4 == 0, 32 or 64 output channels)")
        shapes = [(B, H, W, C if fast0 else 4)]
        for l in range(1, L):
            H, W = ops.convk_out_hw(H, W, self.ks, self.stride)[2:]
            shapes.append((B, H, W, ch[l]))
        # bf16 path: blocks 1.. on the patch convolutions (csrc/conv_patch_bf16.hip: LDS-resident input patch, activations
        # between the blocks channel-blocked) when EVERY block's shape has them; VQA_PCONV=0 keeps the implicit-GEMM kernels
        # (A/B runs, parity tests of both)
        use_pc = bf16 and os.environ.get("VQA_PCONV", "1") != "0" and all(
            ops.pconv_supported(h, w, ci, co, 1) and ci % 64 == 0 and ops.pconv_wgrad_supported(h, w, ci, co)
            for (_, h, w, ci), co in zip(shapes[1:], ch[2:]))
        kinds = ["convk" if self.ks != 3 else "conv0" if l == 0 and fast0 else
                 ("pconv" if use_pc else "conv16") if bf16 else "conv32" for l in range(L)]
        x3 = [k == "conv32" and self._x3_layer(s, co) for k, s, co in zip(kinds, shapes, ch[1:])] + [False]
        # fp32 backward-data of blocks 1.. on the patch kernel (csrc/conv_patch_f32.hip: the pre-pool gradient built in LDS once
        # per K-slice instead of routed once per tap by the loaders); VQA_PDGRAD=0 keeps the implicit-GEMM kernel
        # (measured at B = 256, 224 x 224: 64-channel input 3.96 -> 3.69 ms; 128-channel input 3.20 -> 3.32 ms, so blocks whose
        # input has a multiple of 128 channels stay on the implicit-GEMM kernel unless VQA_PDGRAD=2 forces the patch kernel)
        pdg_mode = os.environ.get("VQA_PDGRAD", "1")
        routes = []
        for l, (kind, s) in enumerate(zip(kinds, shapes)):
            last, src = l == L - 1, routes[-1].out if l else "nchw" if fast0 else "nhwc32"
            pdg = (kind == "conv32" and keep and l > 0 and not x3[l] and self.stride == 1 and pdg_mode != "0"
                   and (s[3] % 128 != 0 or pdg_mode == "2") and ops.pconvf_supported(s[1], s[2], s[3], ch[l + 1]))
            # fp32x3: a block whose successor runs on the split kernels writes its output x3-packed (split once per tensor by
            # the producer's epilogue; forward and wgrad of the successor read that form).  bf16: fp32 out of the last block
            # (the L2 normalisation consumes it)
            out = ("x3" if x3[l + 1] and (x3[l] or kind == "conv0") else
                   "nhwc32" if last or not bf16 else "c16" if use_pc else "nhwc16")
            # the patch kernels read their pooled gradient channel-blocked as well; block 0 has an input gradient only on demand
            dy = "c16" if kind == "pconv" else "nhwc16" if bf16 else "nhwc32"
            dx = routes[-1].dy if l else src if need_dx else None
            need_wd = keep and kind != "conv0" and not pdg and (kind != "conv32" or dx is not None)
            routes.append(ConvRoute(kind, s, ch[l + 1], src, out, dy, dx, x3[l], pdg, x3[l] and src != "x3", need_wd))
        return routes

    @staticmethod
    def _rows16(x: Tensor, ld: int, rows: int, cols: int, rows8: int) -> Tensor:
        """bf16 copy [rows8, cols] of the fp32 matrix x (leading dimension ld), rows beyond `rows` zero."""
        if ld != cols or not x.is_contiguous():
            t = torch.empty(rows, cols, dtype=torch.float32, device=x.device)
            ops.add2d(x, ld, None, 0, t, cols, rows, cols)
            x = t
        out = torch.zeros(rows8, cols, dtype=torch.bfloat16, device=x.device) if rows8 != rows else \
            torch.empty(rows, cols, dtype=torch.bfloat16, device=x.device)
        ops.to_bf16(x.view(rows, cols), out=out[:rows])
        return out

    @staticmethod
    def _cols16(x: Tensor, rows: int, cols: int, cols8: int) -> Tensor:
        """bf16 copy [rows, cols8] of the contiguous fp32 matrix x [rows, cols], columns beyond `cols` zero."""
        x = x.reshape(rows, cols)
        if cols8 == cols:
            return ops.to_bf16(x)
        t = torch.zeros(rows, cols8, dtype=torch.float32, device=x.device)
        ops.add2d(x, cols, None, 0, t, cols8, rows, cols)
        return ops.to_bf16(t)

    def _x3_layer(self, x_shape, Co) -> bool:
        """fp32x3 mode: does this conv block (NHWC input shape, output channels) run on the split kernels?"""
        return self.x3 and len(x_shape) == 4 and ops.conv_x3_supported(x_shape[1], x_shape[2], x_shape[3], Co, self.stride)

    def _x3_gemm(self, rows) -> bool:
        """fp32x3 mode: the three v_conv products (rows = B * positions) run on the split GEMM when they are large
        enough to fill the chip with 192 x 128 tiles."""
        return self.x3_gemm and rows >= 192 * 64 and self.mid >= 128 and self.C >= 64

    # ------------------------------------------------------------------ stream fork / join
    def _on_side_stream(self, dev, job, backward=False):
        """Run job() on the side stream, after everything enqueued so far.  Returns (what job returned, the event that
        marks its end); the caller joins with current_stream.wait_event(event)."""
        # VQA_STREAMS: 0 = one stream; 1 = the question branch on a side stream, joined before the image branch;
        # 2 (default) = the question branch runs UNDER the convolutions (forward: joined before the attention stage,
        # backward: joined at the end).  VQA_STREAMS_BWD (default: VQA_STREAMS) picks the BACKWARD schedule on its
        # own: under data parallelism "1" joins the BPTT chain before the convolution backward starts, so the 'text'
        # bucket (66 % of the gradient bytes) is all-reduced under ALL of the convolution kernels instead of their
        # last 2-3 ms (bench.py --gpus N measures both).  Same box, interleaved, B=256: 27.33 / 26.99 ms per step for 1 / 2 -- the
        # LSTM step launches leave bubbles (prologue / cell epilogue / launch seams of a 44 us kernel) that
        # convolution workgroups fill.
        mode = os.environ.get("VQA_STREAMS", "2")
        main = torch.cuda.current_stream(dev)
        if mode == "0":
            side = main
        else:
            if str(dev) not in self._sides:
                # (a high-priority side stream measured no difference: 27.03 / 27.05 ms per step, 115.4 / 115.6 at the
                # stress shape)
                self._sides[str(dev)] = torch.cuda.Stream(device=dev)
            side = self._sides[str(dev)]
        fork = torch.cuda.Event()
        fork.record(main)
        side.wait_event(fork)
        with torch.cuda.stream(side):
            out = job()
            done = torch.cuda.Event()
            done.record(side)
        if (os.environ.get("VQA_STREAMS_BWD", mode) if backward else mode) == "1":
            main.wait_event(done)
        return out, done

    def _lstm_schedule(self):
        """(fused, use_graph): the recurrence as ONE call per pass, every direction per launch (a cached hipGraph of T
        launches when use_graph), or -- H % 32 != 0, VQA_FUSED_LSTM=0 -- a recurrent GEMM + cell kernel per step."""
        return (ops.lstm_step_supported(self.H) and os.environ.get("VQA_FUSED_LSTM", "1") == "1",
                os.environ.get("VQA_GRAPH", "1") == "1")

    @staticmethod
    def _lstm_steps(T, reverse):
        """(t, state slot read, state slot written) of every step of one direction, in the forward's order."""
        return [(t, t + 1, t) for t in range(T - 1, -1, -1)] if reverse else [(t, t, t + 1) for t in range(T)]

    def _fc_operand(self, fc, x: Tensor, ld: int, cols: int) -> Tensor:
        """The activation x [B, cols] (leading dimension ld) as the FC products take it: as it is, or (bf16 FC) a bf16 copy
        whose rows are padded to a multiple of 8 with zeros: they become the K dimension of the weight-gradient products."""
        return x if fc is None else self._rows16(x, ld, fc.B, cols, fc.B8)

    # ------------------------------------------------------------------ forward
    # kernels launch on HIP's CURRENT device and torch's current stream of that device: _device_current makes the
    # tensors' device current for the whole schedule (a model on cuda:1 while cuda:0 is current would otherwise
    # launch on GPU 0 with GPU-1 pointers)
    @_device_current("v")
    def forward(self, P: Dict[str, Tensor], v: Tensor, q: Tensor, q_len: Tensor, training: bool, seed: int,
                keep: bool, bad_tokens: Optional[Tensor] = None, need_dx: bool = False):
        """Returns (logits [B,A], ctx or None). `keep` = save what backward needs.
        bad_tokens: optional device int32 [1] that counts token ids outside the vocabulary.
        need_dx (with keep): backward also returns the gradient w.r.t. the image v."""
        assert v.is_cuda and v.dtype in (torch.float32, torch.float16) and v.dim() == 4, \
            "v must be a float32 (or the dataset's float16) CUDA tensor [B,C,S,S]"
        v = v.contiguous()
        need_dx = bool(keep and need_dx)
        dev = v.device
        B, T = q.shape
        C, mid, GC = self.C, self.mid, self.GC
        p_txt, p_img, p_att, p_cls = self._rates(training)
        sd = lambda site: _site_seed(seed, site)

        # ---- question encoder (model.py:155-166)
        txt, text_done = self._question_front(P, q, q_len, dev, p_txt, seed, bad_tokens, side=True,
                                              l16=self.lstm16 and (T * B) % 8 == 0)

        # ---- image encoder, image dropout + L2 normalisation over channels (model.py:84,56)
        img = self._image_encoder(P, v, keep, need_dx)
        pooled = img.out
        Pn = pooled.shape[1] * pooled.shape[2]
        # attention.drop(v) (model.py:185) is written by the same pass as a second output: the v_conv operand, as
        # bf16 on the bf16 path
        v_in = v16 = None
        if self.bf16:
            vn, norm, v16 = ops.l2norm_fwd(pooled, p_img, sd(SITE_IMAGE), drop2=(p_att, sd(SITE_ATT_V), torch.bfloat16))
        elif p_att > 0:
            vn, norm, v_in = ops.l2norm_fwd(pooled, p_img, sd(SITE_IMAGE), drop2=(p_att, sd(SITE_ATT_V), torch.float32))
        else:
            vn, norm = ops.l2norm_fwd(pooled, p_img, sd(SITE_IMAGE))
            v_in = vn
        torch.cuda.current_stream(dev).wait_event(text_done)

        # ---- attention (model.py:183-195): v' = v_conv(drop(v)), q' = q_lin(drop(q)), x = relu(v' + q')
        wv16 = ops.to_bf16(P["attention.v_conv.weight"].view(mid, C)) if self.bf16 else None
        qlin = self._q_lin_fwd(P, txt.combined[:, GC:], p_att, seed)
        v_op, wv_op = (v16.view(B * Pn, C), wv16) if self.bf16 else (v_in, P["attention.v_conv.weight"])
        xs, vprime, score, probs = self._attention_fwd(P, v_op, wv_op, vn, qlin[0], txt.combined, B, Pn, p_att, seed, keep)

        # ---- classifier (model.py:198-205)
        logits, *cls = self._classifier_fwd(P, txt.combined, p_cls, seed, qlin[3])
        if not keep:
            return logits, None
        return logits, self._saved(txt, qlin, cls, seed, (p_txt, p_att, p_cls), Pn, vn, v_in, vprime, score, probs, v16=v16,
                                   wv16=wv16, xs=xs, pooled=pooled, **self._encoder_saved(img, norm, p_img, need_dx, v))

    def _rates(self, training):
        """(p_text, p_image, p_att, p_cls) of one forward: the configured dropout rates in train mode, zeros in eval mode."""
        return (self.p_text, self.p_image, self.p_att, self.p_cls) if training else (0.0, 0.0, 0.0, 0.0)

    def _question_front(self, P, q, q_len, dev, p_txt, seed, bad_tokens, side, l16=False):
        """The question prelude of every schedule: q / q_len on the device as int64, embedding + dropout + tanh, the
        classifier-input buffer `combined` [B, Dc], and the question encoder, which fills combined[:, GC:].  Returns (a
        namespace of q, q_len, x_emb [T,B,E], combined, lstm, x16; the event to join on, or None).
        side: the question branch is a chain of small (M = B) launches, independent of the image branch until the
        attention stage; it runs on a side stream, under the convolutions (VQA_STREAMS=2, the default; 1: the main
        stream waits for it before the convolutions start; 0: everything on one stream).  Not side: on the current
        stream (the inference calls have no convolutions to hide it under)."""
        q = q.to(device=dev, dtype=torch.int64).contiguous()
        q_len = q_len.to(device=dev, dtype=torch.int64).contiguous()
        x_emb = ops.embed_tanh_fwd(q, P["text.embedding.weight"], p_txt, _site_seed(seed, SITE_TEXT), bad_tokens)
        combined = torch.empty(q.shape[0], self.Dc, dtype=torch.float32, device=dev)
        encode = lambda: self._question_encoder(P, x_emb, q_len, combined, l16)
        (lstm, x16), done = self._on_side_stream(dev, encode) if side else (encode(), None)
        return SimpleNamespace(q=q, q_len=q_len, x_emb=x_emb, combined=combined, lstm=lstm, x16=x16), done

    @staticmethod
    def _saved(txt, qlin, cls, seed, rates, Pn, vn, v_in, vprime, score, probs, pooled=None, **own):
        """What a backward reads again and what tests and tools look at (stages): the fields every training schedule saves,
        from _question_front's namespace and the results of _q_lin_fwd and _classifier_fwd; `own`: the schedule's own."""
        (qp, q_in, ld_q, fc), (c_in, h1, h1d), (p_txt, p_att, p_cls) = qlin, cls, rates
        B, T = txt.q.shape
        stages = dict(score=score, combined=txt.combined)
        if pooled is not None:
            stages["pooled"] = pooled
        return SimpleNamespace(B=B, T=T, Pn=Pn, q=txt.q, q_len=txt.q_len, x_emb=txt.x_emb, x16=txt.x16, lstm=txt.lstm, vn=vn,
                               v_in=v_in, vprime=vprime, qp=qp, q_in=q_in, ld_q=ld_q, fc=fc, probs=probs, c_in=c_in, h1=h1,
                               h1d=h1d, p_txt=p_txt, p_att=p_att, p_cls=p_cls, seed=seed, stages=stages, **own)

    @staticmethod
    def _encoder_saved(enc, norm, p_img, need_dx, v):
        """The saved fields of a schedule that ran _image_encoder on the image batch v: what the L2-norm backward and
        _conv_bwd read."""
        return dict(routes=enc.routes, acts=enc.acts, idxs=enc.idxs, wds=enc.wds, norm=norm, fast0=enc.fast0, use_pc=enc.use_pc,
                    p_img=p_img, need_dx=need_dx, v_dtype=v.dtype, v_shape=tuple(v.shape))

    def _question_encoder(self, P, x_emb, q_len, combined, l16):
        """LSTM over the embedded question x_emb [T,B,E] on the current stream; the final cell states land in combined[:, GC:].
        Returns (per-direction state: the dicts ops.lstm_seq_fwd takes, plus wih16; x16).
        l16 (bf16 path): the LSTM's non-recurrent products on bf16 MFMA (fp32 accumulation): xg = x . W_ih^T here, dW_hh, dW_ih
        and dx in backward; x and W_ih staged as bf16 (x16, wih16) with the embedding width padded to a multiple of 8
        (16-byte rows).  The recurrence h . W_hh^T, the cells and their gradients stay fp32.  VQA_LSTM16=0: everything fp32."""
        T, B, E = x_emb.shape
        H, Dc, GC = self.H, self.Dc, self.GC
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=x_emb.device)
        Ek = (E + 7) // 8 * 8 if l16 else E
        x16 = self._cols16(x_emb, T * B, E, Ek) if l16 else None
        lstm = []
        for d in range(self.ndir):
            xg = new(T * B, 4 * H)
            w_ih = P["text.lstm.weight_ih_l0" + _SFX[d]]
            wih16 = self._cols16(w_ih, 4 * H, E, Ek) if l16 else None
            _gemm(x16 if l16 else x_emb, wih16 if l16 else w_ih, xg, T * B, 4 * H, Ek,
                  bias1=P["text.lstm.bias_ih_l0" + _SFX[d]], bias2=P["text.lstm.bias_hh_l0" + _SFX[d]], tag=10)
            st = dict(w_hh=P["text.lstm.weight_hh_l0" + _SFX[d]], xg=xg, gates=new(T, B, 4 * H), Hs=new(T + 1, B, H),
                      Cs=new(T + 1, B, H), c_final=combined[:, GC + d * H:], reverse=bool(d), wih16=wih16)
            st["Hs"][T if d else 0].zero_()         # h_0 = c_0 = 0: only the initial slot is read before
            st["Cs"][T if d else 0].zero_()         # it is written
            lstm.append(st)
        fused, use_graph = self._lstm_schedule()
        if fused:
            ops.lstm_seq_fwd(lstm, q_len, B, T, H, cf_ld=Dc, use_graph=use_graph)
            return lstm, x16
        for st in lstm:
            hg = new(B, 4 * H)
            for n, (t, si, so) in enumerate(self._lstm_steps(T, st["reverse"])):
                ops.gemm(st["Hs"][si], st["w_hh"], hg, B, 4 * H, H, tag=11)
                ops.lstm_cell_fwd(st["xg"][t * B:(t + 1) * B], hg, st["Cs"][si], st["Hs"][si], q_len, t, st["gates"][t],
                                  st["Cs"][so], st["Hs"][so], st["c_final"] if n == T - 1 else None, Dc)
        return lstm, x16

    def _image_encoder(self, P, v, keep, need_dx=False):
        """conv + relu + pool x L (models/model.py:79-84) over the image v [B,C,S,S].  Returns a namespace: out (the last
        pooled activation), routes, fast0, use_pc and -- when `keep` -- what backward reads: acts (every block's input, then
        out), idxs (arg-max bytes) and wds (backward-data weights or None) per block.  Nothing kept: an activation is dropped
        as soon as the next block has consumed it."""
        routes = self.conv_routes(tuple(v.shape), keep, need_dx)
        x = v
        if routes[0].src != "nchw":
            # only shapes the dedicated first-block kernels do not cover take a (widened) NHWC4 copy through the generic path
            x = ops.nchw_to_nhwc4(ops.half_to_float(v) if v.dtype == torch.float16 else v)
        acts, idxs, wds = [], [], []
        for l, r in enumerate(routes):
            w, bias = P[f"image.conv{l}.weight"], P[f"image.conv{l}.bias"]
            assert w.shape[0] == r.Co
            x, y, am, wd = getattr(self, f"_{r.kind}_fwd")(r, l, x, w, bias)
            if keep:
                acts.append(x)
                idxs.append(am)
                wds.append(wd)
            x = y
            del y, am, wd       # nothing kept: only the block's output is alive while the next block runs
        if keep:
            acts.append(x)
        return SimpleNamespace(out=x, routes=routes, acts=acts, idxs=idxs, wds=wds, fast0=routes[0].kind == "conv0",
                               use_pc=any(r.kind == "pconv" for r in routes))

    # one forward per route kind: (the block's input as backward reads it again, pooled output, arg-max bytes, backward-data weights)
    def _convk_fwd(self, r, l, x, w, bias):
        wk = ops.convk_pack_weights(w, r.x_shape[3])
        return (x, *ops.convk_fwd(x, wk, bias, self.ks, self.stride, tag=l), wk)

    def _conv0_fwd(self, r, l, x, w, bias):
        return (x, *ops.conv0_fwd(x, w, bias, out_dtype=torch.bfloat16 if self.bf16 else torch.float32, bf16_mfma=self.bf16,
                                  out_packed=r.out == "x3", out_c16=r.out == "c16"), None)

    def _pconv_fwd(self, r, l, x, w, bias):
        wf, wd = ops.pconv_pack_weights(w, need_wd=r.need_wd)
        return (x, *ops.pconv_fwd(x, wf, bias, r.Co, out_dtype=_OUT16[r.out], tag=l), wd)

    def _conv16_fwd(self, r, l, x, w, bias):
        wf, wd = ops.conv_pack_weights_bf16(w, r.x_shape[3], need_wd=r.need_wd)
        return (x, *ops.conv_fwd_bf16(x, wf, bias, self.stride, out_dtype=_OUT16[r.out], tag=l), wd)

    def _conv32_fwd(self, r, l, x, w, bias):
        wf, wd = ops.conv_pack_weights(w, r.x_shape[3], need_wd=r.need_wd)
        if r.pdg:
            wd = ops.pconvf_pack_weights(w)
        if r.x3:
            # operands are split once per tensor, not by every workgroup in every K-step: the weights here, the
            # input activation by its producer (or here, when the producer could not: it replaces the fp32 tensor)
            wf, wd = ops.x3_split(wf), (ops.x3_split(wd) if wd is not None else None)
            if r.pack_in:
                x = ops.x3_pack(x)
        return (x, *ops.conv_fwd(x, wf, bias, self.stride, tag=l, x3=r.x3, out_packed=r.out == "x3"), wd)

    def _q_lin_fwd(self, P, qf, p_att, seed):
        """q' = q_lin(drop(qf)) for the question features qf [B,Q] (leading dimension Dc).  Returns (q' [B,mid], the
        product's input q_in with its leading dimension, fc).  fc: None, or on the bf16 FC path the bf16 weights of q_lin /
        lin1 / lin2 and the bf16 activations that backward reads again: activations and weights are rounded to bf16 where
        the GEMM stages them, fp32 accumulation, fp32 outputs."""
        B, Q, mid, Dc = qf.shape[0], self.Q, self.mid, self.Dc
        if p_att > 0:
            q_in, ld_q = torch.empty(B, Q, dtype=torch.float32, device=qf.device), Q
            ops.add2d(qf, Dc, None, 0, q_in, Q, B, Q)
            ops.dropout(q_in, p_att, _site_seed(seed, SITE_ATT_Q), out=q_in)
        else:
            q_in, ld_q = qf, Dc
        qp = torch.empty(B, mid, dtype=torch.float32, device=qf.device)
        fc = None
        if self.fc16:
            fc = SimpleNamespace(B=B, B8=(B + 7) // 8 * 8,
                                 wq=ops.to_bf16(P["attention.q_lin.weight"]), w1=ops.to_bf16(P["classifier.lin1.weight"]),
                                 w2=ops.to_bf16(P["classifier.lin2.weight"]))
            fc.q16 = self._fc_operand(fc, q_in, ld_q, Q)
        a, wq, lda = (fc.q16, fc.wq, Q) if fc is not None else (q_in, P["attention.q_lin.weight"], ld_q)
        _gemm(a, wq, qp, B, mid, Q, lda=lda, bias1=P["attention.q_lin.bias"], tag=20)
        return qp, q_in, ld_q, fc

    def _attention_fwd(self, P, v_op, wv_op, vn, qp, combined, B, Pn, p_att, seed, keep):
        """x = relu(v' + q') | relu(v' * q') | relu(cat[v', q']) (model.py:188-193) with v' = v_op . wv_op^T (both fp32 or
        both bf16), the scores, and softmax over positions + weighted sum of vn (model.py:208-221) -> combined[:, :G*C].
        Returns (x, v' or None, score, probs)."""
        C, mid, G, Dc, mode = self.C, self.mid, self.G, self.Dc, self.att_mode
        # v' itself is only kept for '*' (its backward needs it), as the aux output of the same GEMM
        # (bf16 path: x is stored as bf16 -- it is streamed three more times and becomes, overwritten in place by
        # d loss / d v', the bf16 operand of both v_conv gradient products)
        xs = torch.empty(B * Pn, mid, dtype=torch.bfloat16 if self.bf16 else torch.float32, device=vn.device)
        vprime = torch.empty(B * Pn, mid, dtype=torch.float32, device=vn.device) if (mode == 1 and keep) else None
        epi = dict(rowgroup=(qp if mode != 2 else None), rg_div=Pn, rg_op=(1 if mode == 1 else 0), relu=True, tag=21)
        if self.bf16 and vprime is None and os.environ.get("VQA_TALL_GEMM", "1") != "0" and \
                ops.gemm_tall_bf16_supported(B * Pn, mid, C, Pn, mode != 2):
            # tall GEMM with K = C only: persistent 256 x 128 tiles (csrc/gemm_tall_bf16.hip)
            ops.gemm_tall_bf16(v_op, wv_op, xs, B * Pn, mid, C, **epi)
        else:
            _gemm(v_op, wv_op, xs, B * Pn, mid, C, aux=vprime, x3=self._x3_gemm(B * Pn), **epi)
        score = ops.att_score_fwd(xs, P["attention.x_conv.weight"].view(G, -1), P["attention.x_conv.bias"], B, Pn, p_att,
                                  _site_seed(seed, SITE_ATT_X), qcat=(qp if mode == 2 else None))
        probs = ops.att_apply_fwd(score, vn, combined, Dc)
        return xs, vprime, score, probs

    def _classifier_fwd(self, P, combined, p_cls, seed, fc):
        """logits = lin2(drop(relu(lin1(drop(combined))))) (model.py:198-205).  Returns (logits, c_in, h1, h1d); on the
        bf16 FC path the bf16 operands stay in fc.c16 / fc.h16 for backward."""
        B, Dc, hid, A = combined.shape[0], self.Dc, self.hid, self.A
        w1, w2 = (fc.w1, fc.w2) if fc is not None else (P["classifier.lin1.weight"], P["classifier.lin2.weight"])
        c_in = ops.dropout(combined, p_cls, _site_seed(seed, SITE_CLS1)) if p_cls > 0 else combined
        h1 = torch.empty(B, hid, dtype=torch.float32, device=combined.device)
        logits = torch.empty(B, A, dtype=torch.float32, device=combined.device)
        c_op = self._fc_operand(fc, c_in, Dc, Dc)
        _gemm(c_op, w1, h1, B, hid, Dc, bias1=P["classifier.lin1.bias"], relu=True, tag=30)
        h1d = ops.dropout(h1, p_cls, _site_seed(seed, SITE_CLS2)) if p_cls > 0 else h1
        h_op = self._fc_operand(fc, h1d, hid, hid)
        _gemm(h_op, w2, logits, B, A, hid, bias1=P["classifier.lin2.bias"], tag=31)
        if fc is not None:
            fc.c16, fc.h16 = c_op, h_op
        return logits, c_in, h1, h1d

    # ------------------------------------------------------------------ many questions per image (inference)
    # Eval mode, fp32 / fp32x3, nothing kept for a backward.  The image encoder, the question encoder, q_lin and the
    # classifier are the forward's own stages; the attention stage runs on ONE v' per image (csrc/att_score.hip).
    @_device_current("v")
    def encode_images(self, P: Dict[str, Tensor], v: Tensor, with_vprime: bool = True, dtype: torch.dtype = torch.float32):
        """v [N,C,S,S] fp32 / fp16 -> (vn [N,Pn,C], v' = v_conv(vn) [N*Pn, mid] or None (with_vprime=False), (gh, gw)).
        dtype float16: both are computed in fp32 as always -- v' from the fp32 vn -- and each is then rounded once
        (ops.to_half); the fp32 temporaries live for this call only."""
        assert not self.bf16, "encode_images: fp32 / fp32x3 only"
        assert dtype in (torch.float32, torch.float16), dtype
        assert v.is_cuda and v.dtype in (torch.float32, torch.float16) and v.dim() == 4, \
            "v must be a float32 (or the dataset's float16) CUDA tensor [N,C,S,S]"
        x = self._image_encoder(P, v.contiguous(), keep=False).out
        N, gh, gw, C = x.shape
        Pn = gh * gw
        vn, _ = ops.l2norm_fwd(x, 0.0, 0)
        vprime = None
        if with_vprime:
            vprime = torch.empty(N * Pn, self.mid, dtype=torch.float32, device=v.device)
            ops.gemm(vn, P["attention.v_conv.weight"], vprime, N * Pn, self.mid, C, tag=21, x3=self._x3_gemm(N * Pn))
        if dtype == torch.float16:
            vn = ops.to_half(vn)
            vprime = ops.to_half(vprime) if vprime is not None else None
        return vn.view(N, Pn, C), vprime, (gh, gw)

    @_device_current("feats", _cache_device)
    def answer(self, P: Dict[str, Tensor], feats, q: Tensor, q_len: Tensor, order: Tensor, offsets: Tensor, img: Tensor,
               bad_tokens: Optional[Tensor] = None):
        """B questions against the N encoded images of `feats` (vn, vprime): question b looks at image img[b]; order /
        offsets (device int32) group the questions by image.  Returns (logits [B,A], probs [B,G,Pn], score [B,G,Pn])."""
        assert not self.bf16, "answer: fp32 / fp32x3 only"
        run = self._answer_tail(P, feats, self._answer_front(P, feats, q, q_len, (order, offsets, img), bad_tokens))
        return run.logits, run.probs, run.score

    def _grouped_scores(self, P, feats, qp, order, offsets, B, qrow=None):
        """Scores [B,G,Pn] straight from v' (one per image) and q' (one per question; a table read through qrow): x is never
        written."""
        N, Pn, _ = feats.vn.shape
        return ops.att_score_grouped_fwd(feats.vprime, qp, P["attention.x_conv.weight"].view(self.G, -1),
                                         P["attention.x_conv.bias"], order, offsets, N, B, Pn, self.att_mode, qrow=qrow)

    # The base run: what a front leaves and every tail reads, one record.  score [B,G,Pn]; combined, the classifier-input
    # buffer [B,Dc]; qp, q' [B,mid] or the pairs' table [M,mid] read through qrow (None on the questions route); cached =
    # (qf, qrow), the pairs' question half of the classifier input (None on the questions route, where the encoder has written
    # it); order / offsets / img; txt, _question_front's namespace on the questions route (the recurrence state, which
    # explain_words goes back through and explain_words_occlusion starts its chains from, stays alive with it).  _answer_tail
    # adds logits, probs and h1.
    def _answer_front(self, P, feats, q, q_len, index, bad_tokens):
        """What answer and the explain calls about questions begin with: the question encoder and q_lin, eval mode, on the
        current stream (there are no convolutions to hide them under), then the scores.  index = (order, offsets, img).
        Returns the base run."""
        order, offsets, img = index
        txt, _ = self._question_front(P, q, q_len, feats.vn.device, 0.0, 0, bad_tokens, side=False)
        qp = self._q_lin_fwd(P, txt.combined[:, self.GC:], 0.0, 0)[0]
        score = self._grouped_scores(P, feats, qp, order, offsets, q.shape[0])
        return SimpleNamespace(score=score, combined=txt.combined, qp=qp, qrow=None, cached=None, order=order, offsets=offsets,
                               img=img, txt=txt)

    def _pairs_front(self, P, feats, qfeats, index):
        """What answer_pairs and the explain calls about pairs begin with: the scores from the two caches.  index = (order,
        offsets, img, qrow).  Returns the base run, with an empty classifier-input buffer."""
        order, offsets, img, qrow = index
        B = img.numel()
        score = self._grouped_scores(P, feats, qfeats.qprime, order, offsets, B, qrow)
        combined = torch.empty(B, self.Dc, dtype=torch.float32, device=feats.vn.device)
        return SimpleNamespace(score=score, combined=combined, qp=qfeats.qprime, qrow=qrow, cached=(qfeats.qf, qrow), order=order,
                               offsets=offsets, img=img, txt=None)

    def _asked_front(self, P, feats, ask):
        """The front of an explain call: _answer_front for an ask that holds questions (q, q_len), _pairs_front for one that
        holds cached questions (qfeats).  ask: what VqaNet._ask_upload leaves -- the source, on_device = (order, offsets, img[,
        qrow]) (device int32), answers (device int32 [B], None: each question's arg-max) and bad_tokens."""
        if ask.qfeats is None:
            return self._answer_front(P, feats, ask.q, ask.q_len, ask.on_device, ask.bad_tokens)
        return self._pairs_front(P, feats, ask.qfeats, ask.on_device)

    def _answer_tail(self, P, feats, run):
        """What every base run ends with: softmax over positions + weighted sum of the image img[b]'s features into
        combined[:, :GC], the pairs' cached question half (models/model.py:64) where there is one, and the eval-mode
        classifier.  Adds logits, probs and h1 = relu(lin1(combined)), which only the explain calls read; returns run."""
        run.probs = ops.att_apply_gather_fwd(run.score, feats.vn, run.img, run.combined, self.Dc)
        if run.cached is not None:
            ops.gather_rows(*run.cached, run.combined[:, self.GC:], self.Q)
        run.logits, _c_in, run.h1, _h1d = self._classifier_fwd(P, run.combined, 0.0, 0, None)
        return run

    @staticmethod
    def _picked(logits, answers):
        """The answer column each question is explained at: `answers`, or (None) topk_answers' arg-max, on the device."""
        return ops.softmax_topk(logits, 1)[0].view(-1) if answers is None else answers

    def _explained(self, what: str, P, feats, ask):
        """What every explain schedule but explain's own tail opens with: the fp32 check in the name of `what`, the finished base
        run of the ask, and the answer column of each question.  Returns (run, answers int32 [B])."""
        assert not self.bf16, f"{what}: fp32 / fp32x3 only"
        run = self._answer_tail(P, feats, self._asked_front(P, feats, ask))
        return run, self._picked(run.logits, ask.answers)

    @staticmethod
    def _fits(cap: int, given: Optional[int], one: int) -> int:
        """How many items of `one` bytes a workspace holds, at least one: under the schedule's *_BYTES constant `cap`, or under
        `given` where a test or a tool passed bytes of its own."""
        return max(1, int((cap if given is None else given) // one))

    # ------------------------------------------------------------------ gradient x input maps from cached features
    # explain / explain_pairs are answer / answer_pairs with the tail kept: from (probs, h1, logits) the gradient of ONE logit
    # per question is carried back to the classifier input (two small products, no parameter gradient), and two kernels turn
    # it into R[b, p] = sum_c vn * d logit / d vn (include/vqa_hip.h) without forming the gradient tensor.
    @_device_current("feats", _cache_device)
    def explain(self, P: Dict[str, Tensor], feats, ask):
        """answer's or answer_pairs' arguments plus answers, as the ask holds them (_asked_front).  Returns (maps [B,Pn],
        answers int32 [B], logits [B,A])."""
        assert not self.bf16, "explain: fp32 / fp32x3 only"
        return self._explain_tail(P, feats, self._asked_front(P, feats, ask), ask.answers)

    def _explain_tail(self, P, feats, run, answers, tail=None):
        """What explain and explain_words end the image side with: _answer_tail, then the gradient of logit[b, answers[b]]
        back to the image half of the classifier input, and the two attribution kernels.  Returns (maps [B,Pn], answers
        int32 [B], logits [B,A]).  tail: a dict that receives dh = d logit / d h1 [B,hid] and dscore [B,G,Pn], which
        explain_words carries on from."""
        logits, probs, h1, img = self._answer_tail(P, feats, run).logits, run.probs, run.h1, run.img
        B, hid, GC, dev = img.numel(), self.hid, self.GC, feats.vn.device
        N, Pn, _ = feats.vn.shape
        answers = self._picked(logits, answers)
        # d logit[b, a_b] / d h1 = W2[a_b, :] where h1 > 0 (a column outside [0, A): a zero row, hence a zero map)
        dh = torch.empty(B, hid, dtype=torch.float32, device=dev)
        ops.gather_rows(P["classifier.lin2.weight"], answers, dh)
        ops.relu_drop_bwd(h1, dh, dh, 0.0, 0)
        # d logit / d combined[:, :GC] = dh . W1[:, :GC]: the image half only, plain fp32 in every compute mode
        dcomb = torch.empty(B, GC, dtype=torch.float32, device=dev)
        ops.gemm(dh, P["classifier.lin1.weight"], dcomb, B, GC, hid, transB=False, lda=hid, ldb=self.Dc)
        dscore, r1 = ops.att_attr_apply_gather(dcomb, GC, probs, feats.vn, img)
        maps = ops.att_attr_score_grouped(r1, dscore, feats.vprime, run.qp, P["attention.x_conv.weight"].view(self.G, -1),
                                          run.order, run.offsets, N, B, Pn, self.att_mode, qrow=run.qrow)
        if tail is not None:
            tail.update(dh=dh, dscore=dscore)
        return maps, answers, logits

    # ------------------------------------------------------------------ integrated gradients from cached features
    # explain's map averaged over S points alpha_s * (vn, v') of the straight path from the zero cache to the real one
    # (include/vqa_hip.h).  The base run gives logits and the column; then, per chunk of questions, explain's
    # tail on the rows x S step-rows: two walks of v' (path scores, path attribution) that read it once each whatever S is,
    # the apply-gather kernels and the classifier's first layer between them.  No parameter gradient, nothing kept.
    IG_BYTES = 256 << 20            # workspace cap of score, probs, dscore and r1 over rows x S: more questions walk in chunks

    def integrated_rows(self, Pn: int, steps: int, ig_bytes: Optional[int] = None) -> int:
        """Questions per chunk of explain_integrated: score, probs and dscore [rows, S, G, Pn] and r1 [rows, S, Pn] fit the cap."""
        return self._fits(self.IG_BYTES, ig_bytes, steps * Pn * (3 * self.G + 1) * 4)

    @_device_current("feats", _cache_device)
    def explain_integrated(self, P: Dict[str, Tensor], feats, ask, alphas: Tensor, chunks):
        """explain's arguments plus alphas (device fp32 [S], the step positions) and chunks: (b0, b1, order, offsets) per range
        of questions, order / offsets (device int32) grouping the questions b0 .. b1-1, numbered from 0, by image.  Returns
        (maps [B,Pn], answers int32 [B], logits [B,A], baseline_logits [B])."""
        run, answers = self._explained("explain_integrated", P, feats, ask)
        logits, img = run.logits, run.img
        B, S, hid, G, GC, Dc, Q, A, dev = img.numel(), alphas.numel(), self.hid, self.G, self.GC, self.Dc, self.Q, self.A, feats.vn.device
        N, Pn, _ = feats.vn.shape
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        wx, bx = P["attention.x_conv.weight"].view(G, -1), P["attention.x_conv.bias"]
        w1, w2, lin1_bias = P["classifier.lin1.weight"], P["classifier.lin2.weight"], P["classifier.lin1.bias"]
        # the step-rows r = b*S + s of every question: its image, its column, and where its question half lies
        rep = lambda t: t.repeat_interleave(S)
        img_r, ans_r, b_r = rep(img), rep(answers), rep(torch.arange(B, dtype=torch.int32, device=dev))
        maps = new(B, Pn)
        rows = max(b1 - b0 for b0, b1, _, _ in chunks)
        score, comb, h1, dh, dcomb = new(rows, S, G, Pn), new(rows * S, Dc), new(rows * S, hid), new(rows * S, hid), new(rows * S, GC)
        for b0, b1, order, offsets in chunks:
            n, R = b1 - b0, (b1 - b0) * S
            qp, qrow = (run.qp[b0:b1], None) if run.qrow is None else (run.qp, run.qrow[b0:b1])
            ops.att_path_score_grouped(feats.vprime, qp, wx, bx, alphas, order, offsets, N, n, Pn, self.att_mode, qrow=qrow,
                                       out=score[:n])
            # combined of the step-rows: alpha_s * sum_p probs_s vn | the question's own half
            probs = ops.att_apply_gather_fwd(score[:n].view(R, G, Pn), feats.vn, img_r[b0 * S:b1 * S], comb[:R], Dc)
            ops.att_path_scale_rows(comb[:R], alphas, GC)
            ops.gather_rows(run.combined[:, GC:], b_r[b0 * S:b1 * S], comb[:R, GC:], Q)
            _gemm(comb[:R], w1, h1[:R], R, hid, Dc, bias1=lin1_bias, relu=True, tag=30)
            # explain's tail on the step-rows: dh = W2[a_b] where h1_s > 0, dcomb = dh . W1[:, :GC] in plain fp32
            ops.gather_rows(w2, ans_r[b0 * S:b1 * S], dh[:R])
            ops.relu_drop_bwd(h1[:R], dh[:R], dh[:R], 0.0, 0)
            ops.gemm(dh[:R], w1, dcomb[:R], R, GC, hid, transB=False, lda=hid, ldb=Dc)
            dscore, r1 = ops.att_attr_apply_gather(dcomb[:R], GC, probs, feats.vn, img_r[b0 * S:b1 * S])
            ops.att_path_attr_grouped(r1.view(n, S, Pn), dscore.view(n, S, G, Pn), feats.vprime, qp, wx, alphas, 1.0 / S, order,
                                      offsets, N, n, Pn, self.att_mode, qrow=qrow, out=maps[b0:b1])
        # the baseline: the eval-mode classifier on [0, qf_b] at column a_b (a column outside [0, A): +0.0)
        comb0 = torch.zeros(B, Dc, dtype=torch.float32, device=dev)
        ops.add2d(run.combined[:, GC:], Dc, None, 0, comb0[:, GC:], Dc, B, Q)
        logits0 = self._classifier_fwd(P, comb0, 0.0, 0, None)[0]
        flat = torch.where((answers >= 0) & (answers < A), torch.arange(B, dtype=torch.int32, device=dev) * A + answers, -1)
        baseline = ops.gather_rows(logits0.view(B * A, 1), flat.to(torch.int32), new(B, 1), 1).view(B)
        return maps, answers, logits, baseline

    # ------------------------------------------------------------------ occlusion maps from cached features
    # What explain estimates to first order, exactly: the fall of ONE logit per question when a window of grid positions is
    # taken out of the image, for every position, in closed form (include/vqa_hip.h vqa_occl_logit).  answer's
    # front and tail, the classifier's first layer applied to every feature row of the distinct asked images (one product per
    # image, question-independent), and one streaming kernel.  No second forward, no parameter gradient, nothing kept.
    U_BYTES = 256 << 20             # workspace cap of U [images, Pn, G, hid]: more asked images are walked in chunks

    @_device_current("feats", _cache_device)
    def explain_occlusion(self, P: Dict[str, Tensor], feats, ask, rows: Tensor, slot: Tensor, window: int = 1,
                          u_bytes: Optional[int] = None):
        """explain's arguments plus rows [n_u] / slot [B] (device int32, model.compact_image_index of the image index: the
        distinct asked images and each question's place among them) and window.  Returns (maps [B,Pn], answers int32 [B],
        logits [B,A]).  Behind the base run: the per-question operands of the closed form (cnull, base, Z), then U = W1_g . vn
        for the distinct asked images in chunks that fit the workspace cap, each followed by the kernel for the questions of
        its images."""
        run, answers = self._explained("explain_occlusion", P, feats, ask)
        cnull, base, column = self._occlusion_operands(P, run, answers)
        combined = run.combined
        B, hid, G, C, Dc, dev = run.img.numel(), self.hid, self.G, self.C, self.Dc, feats.vn.device
        Pn = feats.vn.shape[1]
        gh, gw = feats.grid
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        # Z_g = W1_g . out_g: the image half of lin1 per glimpse, plain fp32 in every compute mode
        w1 = P["classifier.lin1.weight"]
        Z = new(B, G, hid)
        for g in range(G):
            ops.gemm(combined[:, g * C:], w1[:, g * C:], Z[:, g], B, hid, C, lda=Dc, ldb=Dc, ldc=G * hid)
        maps = new(B, Pn)
        for r0, U in self._u_chunks(P, feats, rows, u_bytes):
            ops.occl_logit(base, Z, U, slot, run.probs, run.score, cnull, *column, run.logits, gh, gw, window, slot0=r0, out=maps)
        return maps, answers, run.logits

    def _occlusion_operands(self, P, run, answers):
        """The per-question operands of the closed form that every set of absent positions shares, from a finished base run:
        (cnull [B,G], base [B,hid], column), column = (W2, b2, answers) as the kernels that explain one column take them."""
        B, G, GC, Dc, dev = run.img.numel(), self.G, self.GC, self.Dc, run.score.device
        # cnull: the score kernel's own bits for a position whose v' is 0 -- one all-zero position, every question in one group
        wx, bx = P["attention.x_conv.weight"].view(G, -1), P["attention.x_conv.bias"]
        zero_v = torch.zeros(1, self.mid, dtype=torch.float32, device=dev)
        order1 = torch.arange(B, dtype=torch.int32, device=dev)
        offsets1 = torch.arange(0, B + 1, B, dtype=torch.int32, device=dev)                     # [0, B]
        cnull = ops.att_score_grouped_fwd(zero_v, run.qp, wx, bx, order1, offsets1, 1, B, 1, self.att_mode, qrow=run.qrow)
        # base = b1 + W1[:, GC:] . qf: the question half of lin1, plain fp32 in every compute mode
        w1 = P["classifier.lin1.weight"]
        base = ops.gemm(run.combined[:, GC:], w1[:, GC:], torch.empty(B, self.hid, dtype=torch.float32, device=dev), B, self.hid,
                        self.Q, lda=Dc, ldb=Dc, bias1=P["classifier.lin1.bias"])
        return cnull, base, (P["classifier.lin2.weight"], P["classifier.lin2.bias"], answers)

    def _u_chunks(self, P, feats, rows, u_bytes=None):
        """U = W1_g . vn [n, Pn, G, hid] for the distinct asked images `rows`, n images at a time under the workspace cap, by the
        rule v' follows in encode_images; _bank_rows gathers the asked rows and widens a float16 cache.  Yields (r0, U of the
        images rows[r0 : r0 + n]); the buffer is reused from one chunk to the next."""
        hid, G, C, Dc = self.hid, self.G, self.C, self.Dc
        Pn = feats.vn.shape[1]
        w1 = P["classifier.lin1.weight"]
        n_u = rows.numel()
        per = self._fits(self.U_BYTES, u_bytes, Pn * G * hid * 4)
        U = torch.empty(min(per, n_u), Pn, G, hid, dtype=torch.float32, device=feats.vn.device)
        for r0 in range(0, n_u, per):
            n = min(per, n_u - r0)
            v_in = self._bank_rows(feats.vn, rows[r0:r0 + n], 0.0, 0.0, 0)[1]
            for g in range(G):
                _gemm(v_in, w1[:, g * C:], U[:n, :, g], n * Pn, hid, C, ldb=Dc, ldc=G * hid, x3=self._x3_gemm(n * Pn))
            yield r0, U[:n]

    # ------------------------------------------------------------------ deletion and insertion curves of an attribution map
    # How well a map ranks the positions: the explained logit with the first k positions of the map's ranking absent (deletion)
    # and alone present (insertion), k = 0 .. Pn, in the kept form of the closed form (include/vqa_hip.h vqa_occl_curves;
    # DESIGN.md 4.20).  explain_occlusion's parts -- the base run, cnull, base, U per chunk of images -- plus the ranking kernel
    # and the curve kernels.  Z is not formed.
    @_device_current("feats", _cache_device)
    def explain_faithfulness(self, P: Dict[str, Tensor], feats, ask, rows: Tensor, slot: Tensor, maps: Tensor,
                             u_bytes: Optional[int] = None):
        """explain_occlusion's arguments with maps fp32 [B,Pn] (on the device) in place of window.  Returns (deletion [B,Pn+1],
        insertion [B,Pn+1], order int32 [B,Pn], answers int32 [B], logits [B,A])."""
        run, answers = self._explained("explain_faithfulness", P, feats, ask)
        B, Pn, dev = run.img.numel(), feats.vn.shape[1], feats.vn.device
        order = ops.rank_desc(maps)
        cnull, base, column = self._occlusion_operands(P, run, answers)
        out = tuple(torch.empty(B, Pn + 1, dtype=torch.float32, device=dev) for _ in range(2))
        ws = ops.occl_curves_workspace(B, Pn, self.G, self.hid, dev)
        for r0, U in self._u_chunks(P, feats, rows, u_bytes):
            ops.occl_curves(base, U, slot, run.probs, run.score, cnull, *column, order, slot0=r0, out=out, workspace=ws)
        return out[0], out[1], order, answers, run.logits

    # ------------------------------------------------------------------ probability curves and flip points
    # explain_faithfulness's curves for EVERY answer column at once: the walk keeps each kept set's hidden row instead of
    # collapsing it onto one row of lin2 (include/vqa_hip.h vqa_occl_curves_hidden), one product with lin2 turns
    # the rows into logits, and one kernel reads each logits row once for the probability of the explained column and the best
    # column with its probability (vqa_softmax_pick).  explain_faithfulness's parts as they are -- the base run, the ranking,
    # cnull, base, U per chunk of images -- and per chunk the questions of its images in sub-chunks of whole questions, so that
    # the curve workspace, the hidden rows and the logits of a sub-chunk stay under a cap.
    PROB_WS_BYTES = 256 << 20       # cap of one sub-chunk's curve workspace, hidden rows and logits: more questions walk in sub-chunks

    def prob_curve_questions(self, Pn: int, ws_bytes: Optional[int] = None) -> int:
        """Questions per sub-chunk of explain_faithfulness_probs: per question the curve workspace, the hidden rows [2, Pn+1,
        hid] and their logits [2, Pn+1, A] fit the cap; at least one."""
        one = ops.occl_curves_workspace_bytes(1, Pn, self.G, self.hid) + 2 * (Pn + 1) * (self.hid + self.A) * 4
        return self._fits(self.PROB_WS_BYTES, ws_bytes, one)

    @_device_current("feats", _cache_device)
    def explain_faithfulness_probs(self, P: Dict[str, Tensor], feats, ask, rows: Tensor, slot: Tensor, by_slot: Tensor, offsets,
                                   maps: Tensor, u_bytes: Optional[int] = None, ws_bytes: Optional[int] = None):
        """explain_faithfulness's arguments plus by_slot (device int32 [B]) and offsets (a HOST list [n_u+1]), the questions
        grouped by their place among the distinct asked images (model.compact_image_index), and ws_bytes, the cap of a
        sub-chunk.  Returns (prob [B,2,Pn+1], top int32 [B,2,Pn+1], top_prob [B,2,Pn+1] -- deletion at [:, 0], insertion at
        [:, 1] --, order int32 [B,Pn], answers int32 [B], logits [B,A])."""
        run, answers = self._explained("explain_faithfulness_probs", P, feats, ask)
        B, Pn, hid, A, dev = run.img.numel(), feats.vn.shape[1], self.hid, self.A, feats.vn.device
        order = ops.rank_desc(maps)
        cnull, base, (w2, b2, _) = self._occlusion_operands(P, run, answers)
        # the questions in the order of their images: a chunk of U then owns a contiguous range of them, cut into sub-chunks
        sel = by_slot.long()
        base, probs, score, cnull, ranked, slot_s, cols = (t.index_select(0, sel) for t in
                                                           (base, run.probs, run.score, cnull.view(B, -1), order, slot, answers))
        K = 2 * (Pn + 1)
        per = min(B, self.prob_curve_questions(Pn, ws_bytes))
        assert per * K < (1 << 31)
        ws = ops.occl_curves_workspace(per, Pn, self.G, hid, dev)
        H = torch.empty(per, 2, Pn + 1, hid, dtype=torch.float32, device=dev)
        Y = torch.empty(per * K, A, dtype=torch.float32, device=dev)
        top = torch.empty(B, 2, Pn + 1, dtype=torch.int32, device=dev)
        top_prob, prob = (torch.empty(B, 2, Pn + 1, dtype=torch.float32, device=dev) for _ in range(2))
        for r0, U in self._u_chunks(P, feats, rows, u_bytes):
            q0, q1 = offsets[r0], offsets[r0 + U.shape[0]]
            for b0 in range(q0, q1, per):
                b1 = min(b0 + per, q1)
                n = b1 - b0
                ops.occl_curves_hidden(base[b0:b1], U, slot_s[b0:b1], probs[b0:b1], score[b0:b1], cnull[b0:b1], ranked[b0:b1],
                                       slot0=r0, out=H[:n], workspace=ws)
                # every column's logit of every step: plain fp32 in every compute mode, as base and Z are
                ops.gemm(H[:n].view(n * K, hid), w2, Y[:n * K], n * K, A, hid, bias1=b2)
                ops.softmax_pick(Y[:n * K], cols[b0:b1], K, out=(top[b0:b1], top_prob[b0:b1], prob[b0:b1]))
        # back to the caller's order
        prob, top, top_prob = (torch.empty_like(t).index_copy_(0, sel, t) for t in (prob, top, top_prob))
        return prob, top, top_prob, order, answers, run.logits

    # ------------------------------------------------------------------ sampled Shapley maps from cached features
    # The Shapley value of every grid position for the set function explain_faithfulness walks -- the explained logit with an
    # arbitrary set of positions present -- from M orders that every question shares, and their reverses (include/vqa_hip.h
    # vqa_occl_curves_orders, vqa_shapley_accumulate).  explain_faithfulness's parts once -- the base run, cnull,
    # base, U per chunk of images -- no ranking, and per chunk the orders in groups: the curve kernels over the (question, order)
    # pairs of a group, then the kernel that folds the group's curves into the running mean and M2 of every (question, position).
    SHAPLEY_WS_BYTES = 256 << 20    # cap of the curve workspace of one launch: more orders walk in groups

    @_device_current("feats", _cache_device)
    def explain_shapley(self, P: Dict[str, Tensor], feats, ask, rows: Tensor, slot: Tensor, orders: Tensor, rank: Tensor,
                        u_bytes: Optional[int] = None, ws_bytes: Optional[int] = None):
        """explain_occlusion's arguments with orders / rank (device int32 [M,Pn]: the shared table of permutations and the
        inverse of each row) in place of window, and ws_bytes, the cap of the curve workspace.  Returns (maps [B,Pn], stderr
        [B,Pn], answers int32 [B], logits [B,A], baseline_logits [B])."""
        run, answers = self._explained("explain_shapley", P, feats, ask)
        cnull, base, column = self._occlusion_operands(P, run, answers)
        B, Pn, dev = run.img.numel(), feats.vn.shape[1], feats.vn.device
        M = orders.shape[0]
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        one = max(1, ops.occl_curves_workspace_bytes(B, Pn, self.G, self.hid))       # of one order: B walks
        per = min(M, self._fits(self.SHAPLEY_WS_BYTES, ws_bytes, one))
        ws = ops.occl_curves_orders_workspace(B, per, Pn, self.G, self.hid, dev)
        curves = (new(B * per * (Pn + 1)), new(B * per * (Pn + 1)))
        state, out, baseline = (new(B, Pn), new(B, Pn)), (new(B, Pn), new(B, Pn)), new(B)
        for r0, U in self._u_chunks(P, feats, rows, u_bytes):
            for m0 in range(0, M, per):
                n = min(per, M - m0)
                group = tuple(c[:B * n * (Pn + 1)].view(B, n, Pn + 1) for c in curves)
                ops.occl_curves_orders(base, U, slot, run.probs, run.score, cnull, *column, orders[m0:m0 + n], slot0=r0, out=group,
                                       workspace=ws)
                ops.shapley_accumulate(*group, rank[m0:m0 + n], slot, answers, state, self.A, U.shape[0], slot0=r0, m0=m0,
                                       total=M if m0 + n == M else 0, out=out, empty=baseline)
        return out[0], out[1], answers, run.logits, baseline

    # ------------------------------------------------------------------ gradient x input per question token
    # explain_words is explain carried on to the other input: the same logit's gradient at the question half of the classifier
    # input and, through the scores, at q' (one kernel, csrc/att_score.hip), back through q_lin and the recurrence to the
    # embedding stage, where one kernel (csrc/elementwise.hip) turns it into words[b, t] = sum_e e * d logit / d e.  Data
    # gradients only: no dW_hh, dW_ih, bias or embedding gradient is formed, nothing is written to a gradient buffer.
    @_device_current("feats", _cache_device)
    def explain_words(self, P: Dict[str, Tensor], feats, ask, stages: Optional[dict] = None):
        """explain's arguments, for an ask that holds questions.  Returns (words [B,T], maps [B,Pn], answers int32 [B], logits
        [B,A]); maps, answers and logits are explain's.  stages (a dict) receives dq_att [B,mid] = d logit / d q' through the
        scores (zeros for '|'), attention_path (the launches made for that path: none for '|'), dqf [B,Q] = d logit / d
        (question features) and dx [T,B,E] = d logit / d tanh(e), summed over the directions."""
        assert not self.bf16, "explain_words: fp32 / fp32x3 only"
        run, tail = self._asked_front(P, feats, ask), {}
        maps, answers, logits = self._explain_tail(P, feats, run, ask.answers, tail)
        txt, qp, order, offsets = run.txt, run.qp, run.order, run.offsets
        B, T = txt.q.shape
        N, Pn, _ = feats.vn.shape
        E, H, Q, GC, mid, hid, dev = self.E, self.H, self.Q, self.GC, self.mid, self.hid, feats.vn.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        # d logit / d combined[:, GC:] = dh . W1[:, GC:]: the question half, a product of its own (the image half keeps
        # explain's tiles, hence explain's bits)
        dqf = new(B, Q)
        ops.gemm(tail["dh"], P["classifier.lin1.weight"][:, GC:], dqf, B, Q, hid, transB=False, lda=hid, ldb=self.Dc)
        # + d logit / d q' through the scores, back through q_lin.  '|': that path is identically zero (the q' half shifts every
        # position's score by the same constant and softmax is shift-invariant): no kernel, no q_lin product
        dq_att = None
        if self.att_mode != 2:
            dq_part, NT = ops.att_attr_dq_grouped(tail["dscore"], feats.vprime, qp, P["attention.x_conv.weight"].view(self.G, -1),
                                                  order, offsets, N, B, Pn, self.att_mode)
            dq_att = ops.sum_parts(dq_part, new(B, mid), B, NT, mid)
            ops.gemm(dq_att, P["attention.q_lin.weight"], dqf, B, Q, mid, transB=False, lda=mid, ldb=Q, accumulate=True, tag=47)
        # back through time from dc_n = dqf[:, d*H:(d+1)*H], dh_n = 0, then dx_d = dgates_d . W_ih_d
        dirs = self._recurrence_bwd(P, txt.lstm, txt.q_len, dqf, Q, B, T)
        dx = []
        for d, st in enumerate(dirs):
            dx.append(ops.gemm(st["dgates"], P["text.lstm.weight_ih_l0" + _SFX[d]], new(T * B, E), T * B, E, 4 * H, transB=False,
                               lda=4 * H, ldb=E, tag=53))
        words = ops.embed_attr(txt.q, P["text.embedding.weight"], txt.x_emb, dx[0], dx[1] if self.ndir > 1 else None, txt.q_len)
        if isinstance(stages, dict):
            stages.update(dq_att=dq_att if dq_att is not None else torch.zeros(B, mid, dtype=torch.float32, device=dev),
                          attention_path=("att_attr_dq_grouped", "sum_parts", "q_lin") if dq_att is not None else (),
                          dqf=dqf, dx=(ops.add(dx[0], dx[1], new(T * B, E)) if self.ndir > 1 else dx[0]).view(T, B, E))
        return words, maps, answers, logits

    # ------------------------------------------------------------------ exact word occlusion from cached features
    # What explain_words estimates to first order, exactly: the fall of ONE logit per question when the embedding output of one
    # token slot is the zero vector, for every slot (include/vqa_hip.h vqa_lstm_occl_cell_fwd).  The recurrence has
    # no closed form, but a variant (b, t) shares the forward direction's prefix before t and the reverse direction's after t
    # with the base question, whose states answer's own encoder run has left in Hs / Cs: the variant chains start there.  Per
    # step one recurrent product over the rows whose chain has started and one cell kernel; then q_lin, the grouped scores, the
    # weighted sum and the classifier's first layer on the variant rows (the forward's own stages) and one tail kernel.
    WORDS_BYTES = 256 << 20         # workspace cap of one chunk's variant buffers: more variants are walked in chunks of questions

    def word_occlusion_rows(self, Pn: int) -> int:
        """How many variant rows fit WORDS_BYTES: per row hg [4H], h and c [H] per direction, the classifier input [Dc], q' [mid],
        score and probs [G, Pn] and the hidden layer [hid], fp32."""
        per_row = 4 * (self.ndir * 6 * self.H + self.Dc + self.mid + 2 * self.G * Pn + self.hid)
        return self._fits(self.WORDS_BYTES, None, per_row)

    @_device_current("feats", _cache_device)
    def explain_words_occlusion(self, P: Dict[str, Tensor], feats, ask, chunks):
        """explain's arguments, for an ask that holds questions, plus chunks: model.word_occlusion_table of every chunk of
        questions, its index tensors on the device as int32 and with order / offsets / img, the chunk's variant rows (forward
        order) grouped by their question's image.  Returns (words [B,T], answers int32 [B], logits [B,A]); answers and logits
        are explain's."""
        run, answers = self._explained("explain_words_occlusion", P, feats, ask)
        txt, logits = run.txt, run.logits
        B, T = txt.q.shape
        E, H, GC, Dc, hid, dev = self.E, self.H, self.GC, self.Dc, self.hid, feats.vn.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        # xg0 = b_ih + b_hh in the base product's own bits: the question encoder's xg product on one all-zero input row
        zero_x = torch.zeros(1, E, dtype=torch.float32, device=dev)
        xg0 = [_gemm(zero_x, P["text.lstm.weight_ih_l0" + _SFX[d]], new(1, 4 * H), 1, 4 * H, E,
                     bias1=P["text.lstm.bias_ih_l0" + _SFX[d]], bias2=P["text.lstm.bias_hh_l0" + _SFX[d]], tag=10)
               for d in range(self.ndir)]
        words = new(B, T)
        for tab in chunks:
            V = tab.V
            if V == 0:                                     # no variants: the tail writes the chunk's zeros
                ops.occl_words(new(0, hid), P["classifier.lin2.weight"], P["classifier.lin2.bias"], answers, logits, tab.fwd_b,
                               tab.fwd_t, txt.q_len, words, tab.b0, tab.b1 - tab.b0)
                continue
            combined = new(V, Dc)
            hg = new(V, 4 * H)
            for d, st in enumerate(txt.lstm):
                rev = st["reverse"]
                var_b, var_t, seed = (tab.rev_b, tab.rev_t, tab.rev_seed) if rev else (tab.fwd_b, tab.fwd_t, tab.fwd_seed)
                counts = tab.n_rev if rev else tab.n_fwd
                # the chains' first states: slot t (forward) / t + 1 (reverse) of the base run, one gather per tensor
                h_var = ops.gather_rows(st["Hs"].view((T + 1) * B, H), seed, new(V, H))
                c_var = ops.gather_rows(st["Cs"].view((T + 1) * B, H), seed, new(V, H))
                c_final = combined[:, GC + d * H:]
                for s in (range(tab.steps - 1, -1, -1) if rev else range(tab.steps)):
                    n = counts[s]
                    if n == 0:
                        continue
                    ops.gemm(h_var, st["w_hh"], hg, n, 4 * H, H, tag=11)
                    ops.lstm_occl_cell_fwd(st["xg"].view(T, B, 4 * H), xg0[d], hg, h_var, c_var, txt.q_len, var_b, var_t, s, n,
                                           c_final=c_final, cf_row=tab.rev_row if rev else None)
            # the forward's own stages on V rows: q_lin, the grouped scores, the weighted sum, the classifier's first layer
            qp = self._q_lin_fwd(P, combined[:, GC:], 0.0, 0)[0]
            score_v = self._grouped_scores(P, feats, qp, tab.order, tab.offsets, V)
            ops.att_apply_gather_fwd(score_v, feats.vn, tab.img, combined, Dc)
            h1 = _gemm(combined, P["classifier.lin1.weight"], new(V, hid), V, hid, Dc, bias1=P["classifier.lin1.bias"], relu=True,
                       tag=30)
            ops.occl_words(h1, P["classifier.lin2.weight"], P["classifier.lin2.bias"], answers, logits, tab.fwd_b, tab.fwd_t,
                           txt.q_len, words, tab.b0, tab.b1 - tab.b0)
        return words, answers, logits

    # ------------------------------------------------------------------ cached question features (inference)
    # The mirror image of encode_images / answer: the question encoder and q_lin run once per DISTINCT question, and
    # (image, question) pairs are answered from the two caches -- no recurrence, no convolution in answer_pairs.
    @_device_current("dev", lambda dev: dev)
    def encode_questions(self, P: Dict[str, Tensor], q: Tensor, q_len: Tensor, dev, bad_tokens: Optional[Tensor] = None):
        """q [M,T], q_len [M] -> (qf [M,Q]: the final cell states, a view with row stride Dc; q' = q_lin(qf) [M,mid])."""
        assert not self.bf16, "encode_questions: fp32 / fp32x3 only"
        # the forward's own stages on M rows, eval mode; the encoder writes the question half of a classifier-input buffer
        txt, _ = self._question_front(P, q, q_len, dev, 0.0, 0, bad_tokens, side=False)
        qf = txt.combined[:, self.GC:]
        return qf, self._q_lin_fwd(P, qf, 0.0, 0)[0]

    @_device_current("feats", _cache_device)
    def answer_pairs(self, P: Dict[str, Tensor], feats, qfeats, order: Tensor, offsets: Tensor, img: Tensor, qrow: Tensor):
        """B pairs from the encoded images `feats` (vn, vprime) and the encoded questions `qfeats` (qf, qprime): pair b
        looks at image img[b] with question qrow[b]; order / offsets (device int32) group the pairs by image.  Returns
        (logits [B,A], probs [B,G,Pn], score [B,G,Pn])."""
        assert not self.bf16, "answer_pairs: fp32 / fp32x3 only"
        run = self._answer_tail(P, feats, self._pairs_front(P, feats, qfeats, (order, offsets, img, qrow)))
        return run.logits, run.probs, run.score

    # ------------------------------------------------------------------ training through grouped image features
    # fp32 / fp32x3.  Question b looks at image img[b]; order / offsets group the questions by image.  The question encoder,
    # q_lin and the classifier are the forward's own stages on B questions; the attention stage runs on one v' per image
    # (csrc/att_score.hip) and its backward sums the image-side gradients over the questions of an image.  One schedule
    # (_forward_grouped / backward_grouped) with two image sides:
    #
    # forward_shared: v holds every image ONCE and the image encoder runs on those N images, as a part of the graph.
    # Dropout: the image-side sites (SITE_IMAGE, SITE_ATT_V) draw one mask per IMAGE (logical tensor [N, gh, gw, C]); every
    # question-side site draws per question as forward() does, SITE_ATT_X over [B, P, xld] indexed by the question.
    #
    # forward_features: the image encoder is frozen: `vn` [M,Pn,C] is a bank of its eval-mode outputs (encode_images).  Only the
    # n_u DISTINCT asked rows are touched: rows (ascending) names them, order / offsets group the questions by their slot in
    # rows.  No kernel's grid or byte count depends on M.  v' is recomputed from the current v_conv weight every step.
    # Dropout: SITE_IMAGE is not applied unless image dropout is asked for (a slot index: then it draws per BANK row like
    # SITE_ATT_V, and the asked rows are renormalised after it); SITE_ATT_V draws per BANK row (logical tensor [M, gh, gw, C]);
    # the question-side sites draw per question as forward_shared does.
    @_device_current("v")
    def forward_shared(self, P: Dict[str, Tensor], v: Tensor, q: Tensor, q_len: Tensor, order: Tensor, offsets: Tensor,
                       img: Tensor, training: bool, seed: int, keep: bool, bad_tokens: Optional[Tensor] = None,
                       need_dx: bool = False):
        """v [N,C,S,S]; order / offsets / img: device int32 (model.group_by_image and the image index itself).  Returns
        (logits [B,A], ctx or None), as forward() does."""
        assert not self.bf16, "forward_shared: fp32 / fp32x3 only"
        assert v.is_cuda and v.dtype in (torch.float32, torch.float16) and v.dim() == 4, \
            "v must be a float32 (or the dataset's float16) CUDA tensor [N,C,S,S]"
        v = v.contiguous()
        need_dx = bool(keep and need_dx)
        side = lambda p_img, p_att: self._encoded_images(P, v, keep, need_dx, p_img, p_att, seed)
        return self._forward_grouped(P, side, v.device, q, q_len, order, offsets, img, training, seed, keep, bad_tokens)

    @_device_current("vn")
    def forward_features(self, P: Dict[str, Tensor], vn: Tensor, q: Tensor, q_len: Tensor, rows: Tensor, order: Tensor,
                         offsets: Tensor, img: Tensor, training: bool, seed: int, keep: bool,
                         bad_tokens: Optional[Tensor] = None, slot: Optional[Tensor] = None):
        """vn [M,Pn,C]; rows [n_u], order [B], offsets [n_u+1], img [B]: device int32 (model.compact_image_index and the image
        index itself).  slot [B] (device int32, rows[slot[b]] == img[b]) asks for image dropout: where its rate is above 0
        (train mode, image.dropout > 0) the weighted sum reads the dropped, renormalised rows at slot[b] instead of the bank at
        img[b]; None, or a rate of 0, is the schedule without it.  Returns (logits [B,A], ctx or None)."""
        assert not self.bf16, "forward_features: fp32 / fp32x3 only"
        assert vn.is_cuda and vn.dtype in (torch.float32, torch.float16) and vn.dim() == 3 and vn.is_contiguous() \
            and vn.shape[2] == self.C                   # a float16 bank is read natively: the gather and the weighted sum widen it
        drop = slot is not None and self._rates(training)[1] > 0
        side = lambda p_img, p_att: self._bank_rows(vn, rows, p_img if drop else 0.0, p_att, seed)
        return self._forward_grouped(P, side, vn.device, q, q_len, order, offsets, slot if drop else img, training, seed, keep,
                                     bad_tokens)

    def _encoded_images(self, P, v, keep, need_dx, p_img, p_att, seed):
        """forward_shared's image side: the image encoder on the N images, image dropout + L2 normalisation, attention.drop(v)
        as the same pass's second output.  Returns (vn [N,Pn,C], v_in, N, the schedule's own saved fields)."""
        enc = self._image_encoder(P, v, keep, need_dx)
        N, gh, gw, C = enc.out.shape
        if p_att > 0:
            vn, norm, v_in = ops.l2norm_fwd(enc.out, p_img, _site_seed(seed, SITE_IMAGE),
                                            drop2=(p_att, _site_seed(seed, SITE_ATT_V), torch.float32))
        else:
            vn, norm = ops.l2norm_fwd(enc.out, p_img, _site_seed(seed, SITE_IMAGE))
            v_in = vn
        own = dict(encoded=True, pooled=enc.out, **self._encoder_saved(enc, norm, p_img, need_dx, v))
        return vn.view(N, gh * gw, C), v_in, N, own

    def _bank_rows(self, vn, rows, p_img, p_att, seed):
        """forward_features' image side: the asked rows of the bank vn [M,Pn,C], compacted, with attention.drop(v) indexed by
        the bank row.  Returns (vn: the weighted sum reads the bank itself, undropped; v_in [n_u,Pn,C]; n_u; the schedule's own
        saved fields).  p_img > 0 (image dropout asked for): image.drop and the renormalisation on the compacted rows in the
        same pass, both masks indexed by the bank row; what comes back as vn is then vn_d [n_u,Pn,C], which
        the weighted sum reads at a question's slot in rows."""
        if p_img > 0:
            if p_att > 0:
                vn_d, v_in = ops.gather_rows_drop_norm(vn, rows, p_img, _site_seed(seed, SITE_IMAGE),
                                                       drop2=(p_att, _site_seed(seed, SITE_ATT_V)))
            else:
                vn_d = v_in = ops.gather_rows_drop_norm(vn, rows, p_img, _site_seed(seed, SITE_IMAGE))
            return vn_d, v_in, rows.numel(), dict(encoded=False, rows=rows)
        v_in = ops.gather_rows_drop(vn, rows, p_att, _site_seed(seed, SITE_ATT_V))
        return vn, v_in, rows.numel(), dict(encoded=False, rows=rows)

    def _forward_grouped(self, P, image_side, dev, q, q_len, order, offsets, img, training, seed, keep, bad_tokens):
        """The schedule of forward_shared and forward_features.  image_side(p_img, p_att) -> (vn [*,Pn,C]: what the weighted
        sum reads at row img[b]; v_in [n,Pn,C]: v_conv's input, one entry per group of order / offsets; n; saved fields)."""
        B = q.shape[0]
        C, mid, GC, G = self.C, self.mid, self.GC, self.G
        p_txt, p_img, p_att, p_cls = self._rates(training)

        # ---- question encoder on the side stream, under the image side (as forward())
        txt, text_done = self._question_front(P, q, q_len, dev, p_txt, seed, bad_tokens, side=True)

        # ---- image side, then v' = v_conv(v_in): once per image
        vn, v_in, n, own = image_side(p_img, p_att)
        Pn = vn.shape[1]
        vprime = torch.empty(n * Pn, mid, dtype=torch.float32, device=dev)
        ops.gemm(v_in, P["attention.v_conv.weight"], vprime, n * Pn, mid, C, tag=21, x3=self._x3_gemm(n * Pn))
        torch.cuda.current_stream(dev).wait_event(text_done)

        # ---- attention: scores straight from v' (one per image) and q' (one per question); x is never written
        qlin = self._q_lin_fwd(P, txt.combined[:, GC:], p_att, seed)
        score = ops.att_score_grouped_drop_fwd(vprime, qlin[0], P["attention.x_conv.weight"].view(G, -1),
                                               P["attention.x_conv.bias"], order, offsets, n, B, Pn, self.att_mode, p_att,
                                               _site_seed(seed, SITE_ATT_X))
        probs = ops.att_apply_gather_fwd(score, vn, img, txt.combined, self.Dc)

        # ---- classifier
        logits, *cls = self._classifier_fwd(P, txt.combined, p_cls, seed, qlin[3])
        if not keep:
            return logits, None
        return logits, self._saved(txt, qlin, cls, seed, (p_txt, p_att, p_cls), Pn, vn, v_in, vprime, score, probs, N=n,
                                   order=order, offsets=offsets, img=img, **own)

    @_device_current("dlogits")
    def backward_grouped(self, P: Dict[str, Tensor], ctx, dlogits: Tensor, Gr: Dict[str, Tensor],
                         on_ready: Optional[Callable[[str], None]] = None) -> Optional[Tensor]:
        """backward() for a forward_shared or forward_features context.  forward_shared: the image gradient it returns is
        [N,C,S,S], the questions of an image summed.  forward_features: writes the gradients of classifier, attention and
        text into Gr; the image.* entries of Gr are not touched and there is no image gradient."""
        dev = dlogits.device
        ready = on_ready if on_ready is not None else (lambda group: None)
        B, n, Pn = ctx.B, ctx.N, ctx.Pn
        G, C, mid, Dc = self.G, self.C, self.mid, self.Dc
        encoded = ctx.encoded                   # forward_shared: the gradient goes on into the image encoder
        sd = lambda site: _site_seed(ctx.seed, site)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        dcomb = self._classifier_bwd(P, ctx, dlogits, Gr)
        ready("classifier")
        # ---- attention apply + scores; dvn = the weighted-sum branch of d loss / d vn, summed per image (a bank's has no reader)
        ds_rows = new(B, G, 1)
        if encoded:
            dscore, dvn = ops.att_apply_gather_bwd(dcomb, Dc, ctx.probs, ctx.vn, ctx.img, ctx.order, ctx.offsets, rowsum=ds_rows)
        else:
            dscore = ops.att_apply_gather_dscore(dcomb, Dc, ctx.probs, ctx.vn, ctx.img, rowsum=ds_rows)
        ops.sum_bgp(ds_rows, Gr["attention.x_conv.bias"])
        wx = P["attention.x_conv.weight"].view(G, -1)
        dvprime, dq_part, dwx_part, NT = ops.att_score_grouped_bwd(dscore, ctx.vprime, ctx.qp, wx, ctx.order, ctx.offsets, n, B, Pn,
                                                                   self.att_mode, ctx.p_att, sd(SITE_ATT_X))
        ops.colsum(dwx_part, n * NT, wx.numel(), Gr["attention.x_conv.weight"])
        dqp = new(B, mid)
        ops.sum_parts(dq_part, dqp, B, NT, mid)
        # ---- v_conv over the n * Pn image rows: dW = dv'^T . v_in and, towards the encoder, dv_in = dv' . Wv
        gx3 = self._x3_gemm(n * Pn)
        ops.gemm(dvprime, ctx.v_in, Gr["attention.v_conv.weight"], mid, C, n * Pn, transA=True, transB=False, lda=mid, ldb=C,
                 tag=44, x3=gx3)
        if encoded:
            dv_in = new(n * Pn, C)
            ops.gemm(dvprime, P["attention.v_conv.weight"], dv_in, n * Pn, C, mid, transB=False, lda=mid, ldb=C, tag=45, x3=gx3)
        self._q_lin_bwd(P, ctx, dqp, dcomb, Gr)
        ready("attention")

        def question_branch():
            self._question_bwd(P, ctx, dcomb, Gr)
            ready("text")

        if not encoded:
            question_branch()
            return None
        _, text_done = self._on_side_stream(dev, question_branch, backward=True)
        # ---- image side: join the two branches of d loss / d vn (attention.drop on v, models/model.py:185), L2-norm backward,
        # then the conv blocks.  (vqa_l2norm_bwd_joined recomputes a per-SAMPLE weighted sum and cannot be used here.)
        ops.dropout_add(dv_in, dvn, ctx.p_att, sd(SITE_ATT_V))
        dP = ops.l2norm_bwd(dvn, ctx.vn, ctx.norm, ctx.p_img, sd(SITE_IMAGE)).view_as(ctx.acts[-1])
        dv = self._conv_bwd(P, ctx, dP, Gr)
        ready("image")
        torch.cuda.current_stream(dev).wait_event(text_done)
        return dv

    # ------------------------------------------------------------------ backward
    @_device_current("dlogits")
    def backward(self, P: Dict[str, Tensor], ctx, dlogits: Tensor, Gr: Dict[str, Tensor],
                 on_ready: Optional[Callable[[str], None]] = None) -> Optional[Tensor]:
        """Writes the gradient of every parameter into Gr[name] (caller-owned, same shapes as P).  Returns the gradient
        w.r.t. the image (NCHW, the dtype the forward received) when the forward ran with need_dx, else None.

        `on_ready(group)` is called after the kernels producing a parameter group have been enqueued
        ('classifier', 'attention', 'text', 'image'): the data-parallel wrapper starts that bucket's
        all-reduce there, overlapping the rest of backward."""
        dev = dlogits.device
        ready = on_ready if on_ready is not None else (lambda group: None)
        dcomb = self._classifier_bwd(P, ctx, dlogits, Gr)
        ready("classifier")
        dv_in = self._attention_bwd(P, ctx, dcomb, Gr)
        ready("attention")

        # The question branch's backward runs on a side stream: BPTT, the weight gradients of every direction, the
        # embedding gradient, and from there the 'text' bucket goes to the data-parallel hook, so its all-reduce
        # overlaps the convolution backward.  Default schedule (VQA_STREAMS=2): the branch runs under the convolution
        # backward and is joined at the end; VQA_STREAMS=1: the main stream waits for it before the convolutions.
        def question_branch():
            self._question_bwd(P, ctx, dcomb, Gr)
            ready("text")

        _, text_done = self._on_side_stream(dev, question_branch, backward=True)
        dv = self._image_bwd(P, ctx, dcomb, dv_in, Gr)
        ready("image")
        torch.cuda.current_stream(dev).wait_event(text_done)
        return dv

    def _classifier_bwd(self, P, ctx, dlogits, Gr):
        """Gradients of lin2 / lin1; returns d loss / d combined [B, Dc]."""
        B, Dc, hid, A = ctx.B, self.Dc, self.hid, self.A
        dev = dlogits.device
        sd = lambda site: _site_seed(ctx.seed, site)
        # autograd hands the gradient of a reduction (y.sum()) over as an expanded view with strides 0: add2d and the GEMMs
        # read rows of unit column stride that do not overlap, so such a view is materialised first
        if (A > 1 and dlogits.stride(1) != 1) or (B > 1 and dlogits.stride(0) < A):
            dlogits = dlogits.contiguous()
        # dlogits as a GEMM operand needs a leading dimension that is a multiple of 4
        ldA = (A + 3) // 4 * 4
        if ldA != A or not dlogits.is_contiguous() or dlogits.data_ptr() % 16:
            dl = torch.zeros(B, ldA, dtype=torch.float32, device=dev)
            ops.add2d(dlogits, dlogits.stride(0), None, 0, dl, ldA, B, A)
            dlogits = dl
        # bf16 FC: output gradients staged as bf16 (zero rows up to B8: the K of the dW products), compact rows
        fc = ctx.fc
        if fc is not None:
            Bk, ld_dl, h_op, c_op, w2, w1 = fc.B8, A, fc.h16, fc.c16, fc.w2, fc.w1
        else:
            Bk, ld_dl, h_op, c_op, w2, w1 = B, ldA, ctx.h1d, ctx.c_in, P["classifier.lin2.weight"], P["classifier.lin1.weight"]
        dh1 = torch.empty(B, hid, dtype=torch.float32, device=dev)
        dcomb = torch.empty(B, Dc, dtype=torch.float32, device=dev)
        dl_op = self._fc_operand(fc, dlogits, ldA, A)
        _gemm(dl_op, h_op, Gr["classifier.lin2.weight"], A, hid, Bk, transA=True, transB=False, lda=ld_dl, ldb=hid, tag=40)
        ops.colsum(dlogits, B, A, Gr["classifier.lin2.bias"], ld=ldA)
        _gemm(dl_op, w2, dh1, B, hid, A, transB=False, lda=ld_dl, ldb=hid, tag=41)
        ops.relu_drop_bwd(ctx.h1, dh1, dh1, ctx.p_cls, sd(SITE_CLS2))
        dh_op = self._fc_operand(fc, dh1, hid, hid)
        _gemm(dh_op, c_op, Gr["classifier.lin1.weight"], hid, Dc, Bk, transA=True, transB=False, lda=hid, ldb=Dc, tag=42)
        ops.colsum(dh1, B, hid, Gr["classifier.lin1.bias"])
        _gemm(dh_op, w1, dcomb, B, Dc, hid, transB=False, lda=hid, ldb=Dc, tag=43)
        if ctx.p_cls > 0:
            ops.dropout(dcomb, ctx.p_cls, sd(SITE_CLS1), out=dcomb)
        return dcomb

    def _attention_bwd(self, P, ctx, dcomb, Gr):
        """Gradients of x_conv, v_conv and q_lin; adds d loss / d (question features) into dcomb[:, GC:].  Returns
        dv_in = d loss / d (v_conv's input) [B*Pn, C]."""
        B, Pn = ctx.B, ctx.Pn
        G, C, mid, Dc, GC, Q = self.G, self.C, self.mid, self.Dc, self.GC, self.Q
        sd = lambda site: _site_seed(ctx.seed, site)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dcomb.device)
        # ---- attention apply + scores
        ds_rows = new(B, G, 1)
        # d loss / d vn has two branches -- the weighted sum (probs x dcomb) and attention.drop(v) -> v_conv -- and one reader,
        # the L2-norm backward: it joins them itself (_image_bwd), so the weighted-sum branch is not written here
        dscore, _ = ops.att_apply_bwd(dcomb, Dc, ctx.probs, ctx.vn, rowsum=ds_rows, want_dvn=False)
        ops.sum_bgp(ds_rows, Gr["attention.x_conv.bias"])       # x_conv bias gradient: sum over samples of the row sums
        wx = P["attention.x_conv.weight"].view(G, -1)
        dwx_part, dq_part, RS = ops.att_score_bwd(dscore, wx, ctx.xs, B, Pn, ctx.p_att, sd(SITE_ATT_X),
                                                  mode=self.att_mode, vprime=ctx.vprime, qp=ctx.qp)
        dxpre = ctx.xs                                          # overwritten in place: now d loss / d v'
        ops.colsum(dwx_part, B * RS, wx.numel(), Gr["attention.x_conv.weight"])
        dqp = new(B, mid)
        ops.sum_parts(dq_part, dqp, B, RS, mid)
        # ---- v_conv: dW = dx'^T . v_in (both operands reduction-major), dv_in = dx' . Wv (Wv [mid][C] as the [K][N] operand);
        # bf16 path: both on bf16 MFMA, dx' already is bf16 (written in place over x)
        v_op, wv_op = (ctx.v16.view(B * Pn, C), ctx.wv16) if self.bf16 else (ctx.v_in, P["attention.v_conv.weight"])
        gx3 = self._x3_gemm(B * Pn)
        # the bf16 GEMM takes K in multiples of 8: of an odd batch (B * Pn = 3 * 676, ...) it gets the first rows8 rows, and
        # the fp32 GEMM adds the last 1..7, widened to fp32 -- the products are exact either way, the accumulation fp32
        rows8 = B * Pn // 8 * 8 if self.bf16 else B * Pn
        if rows8:
            _gemm(dxpre, v_op, Gr["attention.v_conv.weight"], mid, C, rows8, transA=True, transB=False, lda=mid, ldb=C, tag=44,
                  x3=gx3)
        if rows8 != B * Pn:
            _gemm(ops.to_f32(dxpre[rows8:]), ops.to_f32(v_op[rows8:]), Gr["attention.v_conv.weight"], mid, C, B * Pn - rows8,
                  transA=True, transB=False, lda=mid, ldb=C, accumulate=rows8 > 0, tag=44)
        dv_in = new(B * Pn, C)
        _gemm(dxpre, wv_op, dv_in, B * Pn, C, mid, transB=False, lda=mid, ldb=C, tag=45, x3=gx3)
        self._q_lin_bwd(P, ctx, dqp, dcomb, Gr)
        return dv_in

    def _q_lin_bwd(self, P, ctx, dqp, dcomb, Gr):
        """Gradients of q_lin from dqp = d loss / d q' [B, mid]; adds d loss / d (question features) into dcomb[:, GC:]."""
        B = ctx.B
        mid, Dc, GC, Q = self.mid, self.Dc, self.GC, self.Q
        sd = lambda site: _site_seed(ctx.seed, site)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dcomb.device)
        ops.colsum(dqp, B, mid, Gr["attention.q_lin.bias"])
        fc = ctx.fc
        if fc is not None:
            Bk, q_op, ld_qop, wq = fc.B8, fc.q16, Q, fc.wq
        else:
            Bk, q_op, ld_qop, wq = B, ctx.q_in, ctx.ld_q, P["attention.q_lin.weight"]
        dqp_op = self._fc_operand(fc, dqp, mid, mid)
        _gemm(dqp_op, q_op, Gr["attention.q_lin.weight"], mid, Q, Bk, transA=True, transB=False, lda=mid, ldb=ld_qop, tag=46)
        # fp32 FC without attention dropout: the GEMM accumulates straight into dcomb's question columns; otherwise the
        # product goes through dq_in, where the dropout mask is applied, and is added from there
        direct = fc is None and ctx.p_att == 0
        dq_in, ld_dq = (dcomb[:, GC:], Dc) if direct else (new(B, Q), Q)
        _gemm(dqp_op, wq, dq_in, B, Q, mid, transB=False, lda=mid, ldb=Q, ldc=ld_dq, accumulate=direct, tag=47)
        if not direct:
            if ctx.p_att > 0:
                ops.dropout(dq_in, ctx.p_att, sd(SITE_ATT_Q), out=dq_in)
            ops.add2d(dcomb[:, GC:], Dc, dq_in, Q, dcomb[:, GC:], Dc, B, Q)

    def _recurrence_bwd(self, P, lstm, q_len, dqf, ld, B, T):
        """Backward through time of every direction, on the current stream: from dc_n = dqf[:, d*H:(d+1)*H] (dqf: d / d
        (question features) [B,Q], leading dimension ld) and dh_n = 0 to dgates [T][B][4H], kept in lstm[d]["dgates"].  The
        recurrence half of _question_bwd, and all of it that explain_words runs; reads the forward's gates, Hs, Cs.  Returns the
        per-direction dicts ops.lstm_seq_bwd takes."""
        H, dev = self.H, dqf.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        dirs = []
        for d, st in enumerate(lstm):
            dc = new(B, H)
            ops.add2d(dqf[:, d * H:], ld, None, 0, dc, H, B, H)
            dh = torch.zeros(B, H, dtype=torch.float32, device=dev)
            st["dgates"] = new(T, B, 4 * H)                   # kept alive until the streams have joined
            dirs.append(dict(w_hh=P["text.lstm.weight_hh_l0" + _SFX[d]], gates=st["gates"], Hs=st["Hs"], Cs=st["Cs"],
                             dgates=st["dgates"], dh=dh, dc=dc, reverse=bool(d)))
        fused, use_graph = self._lstm_schedule()
        if fused:
            # one call: the first cell backward + T-1 fused (dgates . W_hh -> next cell backward) launches,
            # every direction per launch, replayed as a cached hipGraph
            ops.lstm_seq_bwd(dirs, q_len, B, T, H, use_graph=use_graph)
        else:
            for st in dirs:
                for n, (t, si, so) in enumerate(reversed(self._lstm_steps(T, st["reverse"]))):
                    ops.lstm_cell_bwd(st["gates"][t], st["Cs"][si], st["Cs"][so], q_len, t, st["dh"], st["dc"],
                                      st["dgates"][t])
                    if n != T - 1:
                        ops.gemm(st["dgates"][t], st["w_hh"], st["dh"], B, H, 4 * H, transB=False, lda=4 * H, ldb=H,
                                 accumulate=True, tag=50)
        return dirs

    def _question_bwd(self, P, ctx, dcomb, Gr):
        """BPTT over the masked steps, the LSTM weight gradients of every direction and the embedding gradient, on the
        current stream."""
        B, T = ctx.B, ctx.T
        E, H, Dc, GC = self.E, self.H, self.Dc, self.GC
        dev = dcomb.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        # ---- the recurrence: dgates [T][B][4H] of every direction
        self._recurrence_bwd(P, ctx.lstm, ctx.q_len, dcomb[:, GC:], Dc, B, T)
        # ---- weight gradients and dx per direction.  The forward's decision (ctx.x16: bf16 path, T * B a multiple of 8):
        # one bf16 copy of dgates feeds the three products; dW_ih and dx come out Ek wide (the padded embedding width) and
        # their first E columns are copied to where the fp32 products write them
        l16 = ctx.x16 is not None
        x_op, Ek = (ctx.x16, ctx.x16.shape[1]) if l16 else (ctx.x_emb, E)
        dx_parts = []
        for d, st in enumerate(ctx.lstm):
            dgates = st["dgates"]
            h_in = st["Hs"][0:T] if d == 0 else st["Hs"][1:T + 1]
            dw_hh, dw_ih, dx = Gr["text.lstm.weight_hh_l0" + _SFX[d]], Gr["text.lstm.weight_ih_l0" + _SFX[d]], new(T * B, E)
            if l16:
                dg_op, h_op, wih_op = ops.to_bf16(dgates.view(T * B, 4 * H)), ops.to_bf16(h_in.reshape(T * B, H)), st["wih16"]
            else:
                dg_op, h_op, wih_op = dgates, h_in, P["text.lstm.weight_ih_l0" + _SFX[d]]
            _gemm(dg_op, h_op, dw_hh, 4 * H, H, T * B, transA=True, transB=False, lda=4 * H, ldb=H, tag=51)
            dwp = dw_ih if Ek == E else new(4 * H, Ek)
            _gemm(dg_op, x_op, dwp, 4 * H, Ek, T * B, transA=True, transB=False, lda=4 * H, ldb=Ek, tag=52)
            if Ek != E:
                ops.add2d(dwp, Ek, None, 0, dw_ih, E, 4 * H, E)
            ops.colsum(dgates, T * B, 4 * H, Gr["text.lstm.bias_ih_l0" + _SFX[d]])
            ops.add2d(Gr["text.lstm.bias_ih_l0" + _SFX[d]], 4 * H, None, 0, Gr["text.lstm.bias_hh_l0" + _SFX[d]], 4 * H, 1, 4 * H)
            dxp = dx if Ek == E else new(T * B, Ek)
            _gemm(dg_op, wih_op, dxp, T * B, Ek, 4 * H, transB=False, lda=4 * H, ldb=Ek, tag=53)
            if Ek != E:
                ops.add2d(dxp, Ek, None, 0, dx, E, T * B, E)
            dx_parts.append(dx)
        # ---- embedding
        dx_emb = dx_parts[0]
        if self.ndir > 1:
            ops.add(dx_parts[0], dx_parts[1], dx_emb)
        # every row of the embedding gradient is written (deterministic per-row sums)
        ops.embed_tanh_bwd(ctx.q, ctx.x_emb, dx_emb, Gr["text.embedding.weight"], ctx.p_txt, _site_seed(ctx.seed, SITE_TEXT))

    def _image_bwd(self, P, ctx, dcomb, dv_in, Gr):
        """L2-norm (+ dropout) backward, then the conv blocks from the last to the first.  Returns the image gradient
        (ctx.need_dx) or None."""
        sd = lambda site: _site_seed(ctx.seed, site)
        c16_hw = tuple(ctx.idxs[-1].shape[2:4]) if ctx.routes[-1].dy == "c16" else None   # channel-blocked for the routed patches
        dP = ops.l2norm_bwd_joined(dcomb, self.Dc, ctx.probs, dv_in, ctx.p_att, sd(SITE_ATT_V), ctx.vn, ctx.norm, ctx.p_img,
                                   sd(SITE_IMAGE), out_dtype=torch.bfloat16 if self.bf16 else torch.float32, c16_hw=c16_hw)
        if c16_hw is None:
            dP = dP.view_as(ctx.acts[-1])
        return self._conv_bwd(P, ctx, dP, Gr)

    def _conv_bwd(self, P, ctx, dP, Gr):
        """The conv blocks from the last to the first, each as its route says (ctx.routes), from dP = d loss / d (the last
        pooled activation).  Returns the image gradient (ctx.need_dx) or None."""
        for l, r in reversed(list(enumerate(ctx.routes))):
            dP = getattr(self, f"_{r.kind}_bwd")(r, l, ctx, dP, Gr[f"image.conv{l}.weight"], Gr[f"image.conv{l}.bias"],
                                                 P[f"image.conv{l}.weight"])
        if ctx.routes[0].dx == "nhwc32":
            # generic first block (NHWC4 input): drop the pad channel, back to the caller's NCHW layout and dtype
            return ops.nhwc_to_nchw(dP, ctx.v_shape[1], out_dtype=ctx.v_dtype)
        return dP

    # one backward per route kind: writes the block's weight and bias gradients dw, db; returns its input gradient in layout r.dx
    def _convk_bwd(self, r, l, ctx, dP, dw, db, w):
        return ops.convk_bwd(ctx.acts[l], dP, ctx.idxs[l], ctx.wds[l], dw, db, self.ks, self.stride, need_dx=r.dx is not None,
                             tag=l)

    def _conv0_bwd(self, r, l, ctx, dP, dw, db, w):
        (ops.conv0_wgrad_bf16 if self.bf16 else ops.conv0_wgrad)(ctx.acts[0], dP, ctx.idxs[0], dw, db)
        # the image gradient straight from the pooled gradient, in the caller's NCHW layout and dtype (csrc/conv0_dgrad.hip);
        # the bf16 path's forward multiplies by the bf16-rounded weights, so its backward-data does as well
        return ops.conv0_dgrad(dP, ctx.idxs[0], w, ctx.v_shape, out_dtype=ctx.v_dtype, round_w_bf16=self.bf16) if r.dx else None

    def _pconv_bwd(self, r, l, ctx, dP, dw, db, w):
        # both kernels route the pre-pool gradient themselves (pooled gradient + arg-max bytes, C16); a patch block below
        # gets its pooled gradient C16 again, the first block's weight gradient NHWC
        ops.pconv_wgrad(ctx.acts[l], dP, ctx.idxs[l], dw, db, tag=l)
        return ops.pconv_dgrad(dP, ctx.idxs[l], ctx.wds[l], r.x_shape, out_c16=r.dx == "c16", tag=l)

    def _conv16_bwd(self, r, l, ctx, dP, dw, db, w):
        ops.conv_wgrad_bf16(ctx.acts[l], dP, ctx.idxs[l], dw, db, self.stride, tag=l)
        return ops.conv_dgrad_bf16(dP, ctx.idxs[l], ctx.wds[l], r.x_shape, self.stride, tag=l)

    def _conv32_bwd(self, r, l, ctx, dP, dw, db, w):
        # fp32x3: the pooled gradient is split once (x3-packed) for its two readers, wgrad and dgrad
        # (one pass: it also sums the bias gradient)
        dPp = ops.x3_pack_pooled_grad(dP, ctx.idxs[l], db) if r.x3 else None
        ops.conv_wgrad(ctx.acts[l], dP, ctx.idxs[l], dw, None if r.x3 else db, self.stride, tag=l, x3=r.x3, dpooled_packed=dPp)
        if r.pdg:
            return ops.pconvf_dgrad(dP, ctx.idxs[l], ctx.wds[l], r.x_shape, tag=l)
        if r.dx:
            return ops.conv_dgrad(dPp if r.x3 else dP, ctx.idxs[l], ctx.wds[l], r.x_shape, self.stride, tag=l, x3=r.x3)
