/* vqa_hip.h — C ABI of libvqa_hip.so: the MI355X (gfx950) kernels behind VqaNet.forward/backward.
 *
 * The reference (OmerShubi/DL_VQA) has no FFI layer: its hot path is a chain of stock torch
 * operators inside models/model.py:53-67 and train.py:189-206.  Each entry point below replaces
 * one fused stage of that chain; the reference lines it stands in for are cited per function.
 *
 * Conventions:
 *   - every tensor argument is a raw DEVICE pointer into caller-owned memory (torch storage);
 *     the library never allocates, frees or synchronises;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it;
 *   - return value: 0 = success, otherwise a VQA_ERR_* code; vqa_last_error() gives the text;
 *   - no C++ exception crosses the ABI; functions are re-entrant (safe from any host thread, any device);
 *     the only state is the optional profiling hook, the VQA_* knobs (read once), a per-device record of
 *     kernels whose LDS limit has been raised and the cache of LSTM-sequence hipGraphs, all behind mutexes;
 *   - all floating point is IEEE fp32; contractions use v_mfma_f32_32x32x2_f32 (exact fp32);
 *   - matrices are row-major with an explicit leading dimension in ELEMENTS; pointers and leading
 *     dimensions of GEMM operands must be multiples of 4 elements (16-byte vector loads);
 *   - images inside the library are NHWC; question activations are time-major [T][B][*].
 */
#ifndef VQA_HIP_H
#define VQA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an exported entry point changes its argument list or disappears (round 1: 1, round 2: 2, round 3: 3).
 * dl_vqa_amd/_lib.py parses this line and refuses a library that answers differently.
 * Additions are append-only and do not bump it: the entry points of training through shared image features
 * (vqa_att_score_grouped_drop_fwd, vqa_att_apply_gather_bwd, vqa_att_score_grouped_tiles, vqa_att_score_grouped_bwd) joined
 * version 8 that way, vqa_softmax_topk after them, and the two entry points of cached question features
 * (vqa_att_score_grouped_pairs_fwd, vqa_gather_rows) after that, then image preprocessing (vqa_preprocess_supported,
 * vqa_preprocess_images), then the two entry points of training on cached image features (vqa_gather_rows_drop,
 * vqa_att_apply_gather_dscore), then the plan query vqa_gemm_plan, then the tall GEMM's own query vqa_gemm_tall_bf16_plan, then
 * Adam over a table of segments (vqa_adam_segments, with the struct vqa_adam_segment) -- a caller
 * built against the earlier version-8 header finds every prototype it knows unchanged.
 * Version 9 adds the plan query of the fp32x3 conv entry points (vqa_conv3x3_x3_plan), appended at the end; every
 * version-8 prototype is unchanged.  The entry points of float16 image-feature caches joined version 9 the append-only way
 * (vqa_float_to_half, vqa_gather_rows_drop_f16, vqa_att_apply_gather_fwd_f16, vqa_att_apply_gather_dscore_f16,
 * vqa_att_score_grouped_fwd_f16, vqa_att_score_grouped_pairs_fwd_f16), and after them the two of image dropout on a bank of
 * cached image features (vqa_gather_rows_drop_norm, vqa_gather_rows_drop_norm_f16; declared with the entry points of training
 * on cached image features), and then the seven of gradient x input attribution (vqa_att_attr_apply_gather, vqa_att_attr_apply_gather_f16,
 * vqa_att_attr_score_grouped_path, vqa_att_attr_score_grouped, vqa_att_attr_score_grouped_pairs, vqa_att_attr_score_grouped_f16,
 * vqa_att_attr_score_grouped_pairs_f16; declared behind those of the cached-feature paths they extend), and then the three of
 * gradient x input per question token (vqa_att_attr_dq_grouped, vqa_att_attr_dq_grouped_f16, vqa_embed_attr; declared behind
 * the attribution entry points), and then the one of occlusion maps (vqa_occl_logit; declared behind those), and
 * then the two of exact word occlusion (vqa_lstm_occl_cell_fwd, vqa_occl_words; declared behind vqa_occl_logit), and then the
 * four of deletion and insertion curves (vqa_rank_desc, vqa_occl_curves_chunk, vqa_occl_curves_workspace_bytes, vqa_occl_curves;
 * declared behind those), and then those of integrated gradients (vqa_att_path_score_grouped, vqa_att_path_attr_grouped and
 * their _pairs, _f16 and _pairs_f16 forms, with vqa_att_path_scale_rows; declared behind those), and then the three of sampled
 * Shapley maps (vqa_occl_curves_orders_workspace_bytes, vqa_occl_curves_orders, vqa_shapley_accumulate; declared beside the
 * curve entry points), and then the two of probability curves (vqa_occl_curves_hidden, declared behind those, and
 * vqa_softmax_pick, declared behind vqa_softmax_topk). */
#define VQA_ABI_VERSION 9

#define VQA_OK 0
#define VQA_ERR_INVALID 1 /* bad argument (shape, alignment, null pointer) */
#define VQA_ERR_HIP 2     /* a HIP runtime call or kernel launch failed */
#define VQA_ERR_WORKSPACE 3 /* workspace too small */

typedef void* vqa_stream_t; /* hipStream_t */

int vqa_abi_version(void);
const char* vqa_last_error(void);
/* 1 if a gfx950 device is visible to the HIP runtime, else 0 (never fails). */
int vqa_device_ok(void);

/* Re-read the VQA_* environment knobs (forced tile variants for parity tests, diagnostics).  They are read
 * once when the library is first used; tests that switch variants inside one process call this. */
int vqa_reload_knobs(void);

/* ---- profiling hook (bench.py: live HIP-event timing of one kernel family) ------------------ */
enum {
  VQA_K_GEMM = 0,
  VQA_K_CONV_FWD = 1,
  VQA_K_CONV_DGRAD = 2,
  VQA_K_CONV_WGRAD = 3,
  /* HBM-bound stages (bench.py reports GB/s against the 8 TB/s HBM3E peak for these) */
  VQA_K_L2NORM_FWD = 4,
  VQA_K_L2NORM_BWD = 5,
  VQA_K_ATT_SCORE_FWD = 6,
  VQA_K_ATT_SCORE_BWD = 7,
  VQA_K_ATT_APPLY_FWD = 8,
  VQA_K_ATT_APPLY_BWD = 9,
  VQA_K_ADAM = 10,
  VQA_K_SOFTCE = 11,
  VQA_K_DROPOUT = 12,
  VQA_K_LSTM_SEQ = 13, /* one whole vqa_lstm_seq_fwd / _bwd call (T launches or one graph replay) */
  VQA_K_COUNT = 14
};
/* Arm event bracketing for kernel family `kernel_id` whose launch tag equals `tag`
 * (tag < 0: any). kernel_id == VQA_K_COUNT arms every family; kernel_id < 0 disarms.
 * Resets the accumulated numbers. */
int vqa_prof_arm(int kernel_id, int tag);
/* The same for a SET of families: bit k of `mask` arms family k (mask 0 disarms). */
int vqa_prof_arm_mask(uint32_t mask, int tag);
/* Synchronise the recorded events; returns launches counted and their total device time. */
int vqa_prof_read(int* launches, float* total_ms);
/* Per (family, tag) totals of the recorded events: fills up to `cap` entries of ids / tags / launches /
 * total_ms and returns the number of distinct (family, tag) pairs seen. */
int vqa_prof_read_groups(int* ids, int* tags, int* launches, float* total_ms, int cap);

/* ---- generic GEMM ---------------------------------------------------------------------------
 * C[M][N] = act( A.B  (op) rowgroup + bias1 + bias2 ) (+ C if accumulate)
 *   transA = 0: A stored [M][K];  1: A stored [K][M]
 *   transB = 0: B stored [K][N];  1: B stored [N][K]   (torch nn.Linear weight => transB = 1)
 *   rowgroup (optional): value rowgroup[(m / rg_div) * rg_ld + n], rg_op 0 = add, 1 = multiply
 *     (the question projection tiled over image positions, models/model.py:187-193,224-231)
 *   relu: 0/1.   tag: free integer recorded by the profiling hook.
 * Replaces nn.Linear / 1x1 nn.Conv2d / LSTM projections (models/model.py:145,173-174,202,205)
 * and every dX / dW product of their backward passes.
 * Small outputs are split along K over workgroups; partial slabs live in `workspace`. */
int64_t vqa_gemm_workspace_bytes(int M, int N, int K);
int vqa_gemm(const float* A, int64_t lda, int transA, const float* B, int64_t ldb, int transB,
             float* C, int64_t ldc, int M, int N, int K, const float* bias1, const float* bias2,
             const float* rowgroup, int64_t rg_ld, int rg_div, int rg_op, int relu, int accumulate,
             float* aux /* optional [M][ldc]: the raw product A.B before the epilogue (v' for '*') */,
             float* workspace, int64_t workspace_bytes, int tag, vqa_stream_t stream);

/* ---- image encoder: Conv2d(k=3, stride, pad=0) + ReLU + MaxPool2d(2,2) ----------------------
 * (models/model.py:72-84 ImageNet2). Activations NHWC, channel count padded to a multiple of 4
 * (CiP); weights re-packed per step from the torch layout [Co][Ci][3][3]. */
int vqa_nchw_to_nhwc4(const float* x_nchw, float* y_nhwc, int B, int C, int H, int W, vqa_stream_t stream);
/* wf[(ky*3+kx)*CiP + ci][co], wd[(ky*3+kx)*Co + co][ci]  (wd may be NULL) */
int vqa_conv_pack_weights(const float* w, float* wf, float* wd, int Co, int Ci, int CiP, vqa_stream_t stream);
/* pooled[B][Hp][Wp][Co], argmax[B][Hp][Wp][Co] in {0..3 = dy*2+dx of the winning pre-activation,
 * 4 = window dead (max <= 0, ReLU blocks the gradient)}; Hp = ((H-3)/stride+1)/2 (floor). */
int vqa_conv3x3_relu_pool_fwd(const float* x, const float* wf, const float* bias, float* pooled,
                              uint8_t* argmax, int B, int H, int W, int CiP, int Co, int stride,
                              int tag, vqa_stream_t stream);
/* dx[B][H][W][CiP] = gradient w.r.t. the conv input, routed through arg-max and ReLU. */
int vqa_conv3x3_dgrad(const float* dpooled, const uint8_t* argmax, const float* wd, float* dx, int B,
                      int H, int W, int CiP, int Co, int stride, int tag, vqa_stream_t stream);
/* dw[Co][Ci][3][3] and dbias[Co] (torch layouts; written, not accumulated). */
int64_t vqa_conv3x3_wgrad_workspace_bytes(int B, int H, int W, int CiP, int Co, int stride);
int vqa_conv3x3_wgrad(const float* x, const float* dpooled, const uint8_t* argmax, float* dw,
                      float* dbias, int B, int H, int W, int CiP, int Ci, int Co, int stride,
                      float* workspace, int64_t workspace_bytes, int tag, vqa_stream_t stream);

/* Conv blocks with image.kernel_size != 3 (models/model.py:75-82: nn.Conv2d(kernel_size=k, stride) -> ReLU -> MaxPool2d(2,2);
 * utils/config_schema.py:59 admits any int, config.yaml:58 ships 3): the materialised form of the same product
 * (csrc/conv_generic.hip).  The caller writes the im2col matrix of a batch chunk, runs vqa_gemm on it (bias in the GEMM's
 * epilogue, relu = 0) and pools; backward routes the pooled gradient to the pre-pool rows, takes dW = dY^T.cols and
 * dcols = dY.wk with vqa_gemm and folds dcols back.  Ho = (H - ks)/stride + 1, rows r = (b*Ho + yo)*Wo + xo, K index
 * (ky*ks + kx)*CiP + ci; ks in 1..15, stride 1 or 2, CiP % 4 == 0, Co % 4 == 0; arg-max bytes as above (0..3, 4 = dead).
 *   wk [Co][ks*ks*CiP] from torch's [Co][Ci][ks][ks] (channels >= Ci zero); vqa_convk_unpack_wgrad is its inverse for dW. */
int vqa_convk_pack_weights(const float* w, float* wk, int Co, int Ci, int CiP, int ks, vqa_stream_t stream);
int vqa_convk_unpack_wgrad(const float* dwk, float* dw, int Co, int Ci, int CiP, int ks, vqa_stream_t stream);
int vqa_convk_im2col(const float* x, float* cols, int B, int H, int W, int CiP, int ks, int stride, vqa_stream_t stream);
/* y [B*Ho*Wo][Co] = the convolution output with its bias, before the ReLU */
int vqa_convk_relu_pool(const float* y, float* pooled, uint8_t* argmax, int B, int Ho, int Wo, int Co, vqa_stream_t stream);
int vqa_convk_route(const float* dpooled, const uint8_t* argmax, float* dy, int B, int Ho, int Wo, int Co, vqa_stream_t stream);
int vqa_convk_col2im(const float* dcols, float* dx, int B, int H, int W, int CiP, int ks, int stride, vqa_stream_t stream);

/* First conv block, dedicated path (Cin <= 3, stride 1, Co in {32, 64}, W % 4 == 0): reads the caller's
 * NCHW image directly (no layout conversion), weights/bias in torch layout, same pooled/argmax outputs
 * as vqa_conv3x3_relu_pool_fwd.  vqa_conv0_supported() tells whether a shape takes this path. */
int vqa_conv0_supported(int Ci, int H, int W, int Co, int stride);
int vqa_conv0_relu_pool_fwd(const void* x_nchw, int x_is_fp16 /* 1: __half NCHW as the dataset stores it, widened where
                            the patch is staged (preprocess_images.py:39-53); 0: float */, const float* w, const float* bias, void* pooled,
                            int pooled_is_bf16 /* 0: fp32 out; 1: fp32 MFMA, P_0 stored as bf16; 2 (bf16 path):
                            image and weights rounded to bf16, two 32x32x16 bf16 MFMA k-steps, bf16 out; 3 (fp32x3 path): fp32
                            MFMA, the output written x3-packed (vqa_x3_pack's form, 6 bytes per element); 4: as 2 with the
                            pooled map channel-blocked, [B][Co/16][Hp][Wp][16] (what vqa_pconv_* read; arg-max stays NHWC) */, uint8_t* argmax, int B, int Ci,
                            int H, int W, int Co, vqa_stream_t stream);
int64_t vqa_conv0_wgrad_workspace_bytes(int Co);
int vqa_conv0_wgrad(const void* x_nchw, int x_is_fp16, const float* dpooled, const uint8_t* argmax, float* dw, float* dbias,
                    int B, int Ci, int H, int W, int Co, float* workspace, int64_t workspace_bytes,
                    vqa_stream_t stream);

/* bf16 path: the first block's weight gradient on bf16 MFMA (image rounded to bf16 where it is staged, bf16 pooled
 * gradient as written by vqa_conv3x3_dgrad_bf16, fp32 accumulation, fp32 dw / dbias).  Same workspace query. */
int vqa_conv0_wgrad_bf16(const void* x_nchw, int x_is_fp16, const void* dpooled_bf16, const uint8_t* argmax, float* dw,
                         float* dbias, int B, int Ci, int H, int W, int Co, float* workspace,
                         int64_t workspace_bytes, vqa_stream_t stream);

/* ---- input-image gradient (v.requires_grad: saliency, attribution; csrc/conv0_dgrad.hip) ----------------------------
 * The first block's backward-data on the dedicated path (Ci <= 3, stride 1, Co in {32, 64}, W % 4 == 0):
 *   dv[b][c][y][x] = sum_{co,ky,kx} w[co][c][ky][kx] * dY[b][co][y-ky][x-kx], dY routed from the pooled gradient
 *   dpooled [B][Hp][Wp][Co] (fp32, or bf16 when dpooled_is_bf16) through the arg-max bytes (0..3, 4 = dead).
 * w in torch layout [Co][Ci][3][3] (round_w_bf16: rounded to bf16 as the bf16-path forward uses them).  dv is the
 * caller's NCHW layout, fp32 or (dv_is_fp16) fp16; every element is written, no atomics (bit-reproducible). */
int vqa_conv0_dgrad_supported(int Ci, int H, int W, int Co, int stride);
int vqa_conv0_dgrad(const void* dpooled, int dpooled_is_bf16, const uint8_t* argmax, const float* w, void* dv, int dv_is_fp16,
                    int round_w_bf16, int B, int Ci, int H, int W, int Co, vqa_stream_t stream);
/* NHWC [B][H][W][CP] fp32 -> NCHW [B][C][H][W] fp32 or (y_is_fp16) fp16, channels C..CP-1 dropped: the inverse of
 * vqa_nchw_to_nhwc4, for the input gradient of the generic first-block paths. */
int vqa_nhwc_to_nchw(const float* x_nhwc, void* y_nchw, int y_is_fp16, int B, int C, int CP, int H, int W, vqa_stream_t stream);

/* ---- dropout (nn.Dropout, 7 sites: models/model.py:84,156,185,186,194,201,204) ---------------
 * y = x * keep(seed, i) / (1-p); keep() is a counter-based hash, so backward calls the same
 * function on the gradient. In-place allowed. */
int vqa_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, vqa_stream_t stream);
/* y += x * keep(seed, i) / (1-p): the backward of a dropout whose gradient joins another one (attention.drop on v:
 * d loss / d v = dropout-mask * d loss / d v_in + the weighted-sum branch, models/model.py:185,62) in ONE pass. */
int vqa_dropout_add(const float* x, float* y, int64_t n, float p, uint64_t seed, vqa_stream_t stream);

/* ---- L2 normalisation over channels (models/model.py:56), fused with image.drop (model.py:84) -
 * u = dropout(pooled); norm = ||u||_2 per row; vn = u / (norm + 1e-12).  rows = B*P, C channels.
 * vdrop (optional): a second output dropout_{p2, seed2}(vn), fp32 or bf16 -- attention.drop applied to v
 * (models/model.py:185), i.e. the v_conv operand, written in the same pass. */
int vqa_l2norm_fwd(const float* pooled, float* vn, float* norm, int64_t rows, int C, float p,
                   uint64_t seed, void* vdrop, int vdrop_is_bf16, float p2, uint64_t seed2, vqa_stream_t stream);
int vqa_l2norm_bwd(const float* dvn, const float* vn, const float* norm, void* dpooled,
                   int dpooled_mode /* 0 fp32 [rows][C]; 1 bf16 [rows][C] (bf16 path: no separate conversion pass); 2 bf16
                                       channel-blocked [rows / positions][C/16][positions][16] for vqa_pconv_dgrad / _wgrad */,
                   int64_t rows, int positions /* rows per image: mode 2 only */, int C, float p, uint64_t seed,
                   vqa_stream_t stream);
/* The same with the incoming gradient JOINED in the kernel instead of read from a [rows][C] tensor:
 *   d loss / d vn [b*P + p][:] = sum_g probs[b][g][p] * dout[b][g*C : (g+1)*C]            (the weighted-sum branch, model.py:62:
 *                                                                                          what vqa_att_apply_bwd writes as dvn)
 *                               + dropout_{p_v, seed_v}-mask * dv_in[b*P + p][:]           (attention.drop on v, model.py:185:
 *                                                                                          what vqa_dropout_add adds)
 * -- two passes over a [B*P][C] fp32 tensor less per step; vqa_att_apply_bwd is then called with dvn = NULL. */
int vqa_l2norm_bwd_joined(const float* dout, int64_t dout_ld, const float* probs, int G, const float* dv_in, float p_v,
                          uint64_t seed_v, const float* vn, const float* norm, void* dpooled, int dpooled_mode, int64_t rows,
                          int positions, int C, float p, uint64_t seed, vqa_stream_t stream);

/* ---- question encoder (models/model.py:134-166 questionNet) ----------------------------------
 * x[t][b][:] = tanh(dropout(emb[q[b][t]]))   (embedding -> drop -> tanh, model.py:155-157).
 * Token ids outside [0, V) -- nn.Embedding raises for them -- are counted into *bad_tokens (device int32,
 * may be NULL; the caller zeroes and reads it) and contribute a zero row, forward and backward alike. */
int vqa_embed_tanh_fwd(const int64_t* q, const float* emb, float* x, int B, int T, int E, int V,
                       float p, uint64_t seed, int32_t* bad_tokens, vqa_stream_t stream);
/* demb[v][:] = sum over the slots (b,t) with q[b][t] == v of dx * (1 - x^2) * dropmask, in slot order
 * (deterministic, no atomics); every row of demb [V][E] is WRITTEN (row 0 = padding_idx and unused rows: zeros). */
/* workspace (optional, vqa_embed_tanh_bwd_workspace_bytes): the slots are binned by token first and every row sums its own
 * (sorted) bin -- O(B*T + V) instead of the workspace-less form's scan of all B*T slots per vocabulary row; same bits. */
int64_t vqa_embed_tanh_bwd_workspace_bytes(int B, int T, int V);
int vqa_embed_tanh_bwd(const int64_t* q, const float* x, const float* dx, float* demb, int B, int T,
                       int E, int V, float p, uint64_t seed, void* workspace /* may be NULL */, int64_t workspace_bytes,
                       vqa_stream_t stream);
/* One LSTM time step for one direction (gate order i,f,g,o; nn.LSTM, model.py:145-149):
 *   pre = xg[b] + hg[b]   (xg = x W_ih^T + b_ih + b_hh for time t, hg = h_in W_hh^T, both [B][4H])
 *   rows with t >= q_len[b] keep (h,c) unchanged — the packed-sequence semantics of model.py:159-164.
 * Writes activated gates [B][4H], c_out, h_out; if c_final != NULL also c_final[b*cf_ld + j]. */
int vqa_lstm_cell_fwd(const float* xg, const float* hg, const float* c_in, const float* h_in,
                      const int64_t* q_len, int t, float* gates, float* c_out, float* h_out,
                      float* c_final, int64_t cf_ld, int B, int H, vqa_stream_t stream);
/* Backward of one step. In: dh [B][H] (grad w.r.t. h_out), dc [B][H] (grad w.r.t. c_out).
 * Out: dgates [B][4H] (pre-activation grads, 0 for inactive rows), dc <- grad w.r.t. c_in,
 * dh <- pass-through part of grad w.r.t. h_in (dh for inactive rows, 0 for active rows); the caller
 * then accumulates dgates.W_hh onto dh with vqa_gemm(accumulate=1). */
int vqa_lstm_cell_bwd(const float* gates, const float* c_in, const float* c_out, const int64_t* q_len,
                      int t, float* dh, float* dc, float* dgates, int B, int H, vqa_stream_t stream);

/* The whole recurrence of one question batch as ONE call (models/model.py:145-149, 159-164): T dependent launches,
 * each covering every direction; a forward step is h_{t-1} W_hh^T on the MFMA engine with the cell as its epilogue,
 * a backward step is dgates_t W_hh over the whole K = 4H inside one workgroup (split over its MFMA waves by gate,
 * combined through LDS) with the cell backward of the next time as its epilogue -- they replace vqa_gemm +
 * vqa_lstm_cell_fwd, resp. vqa_lstm_cell_bwd + split-K vqa_gemm + reduce, per step and direction.
 * Requires H % 32 == 0 (vqa_lstm_step_supported); other sizes use the unfused entry points above.
 *   use_graph != 0: the chain is replayed as an explicit hipGraph, built once per distinct argument set (shapes AND
 *   pointers) and cached inside the library (at most 32 graphs per process, least recently used dropped; a caller
 *   whose buffers move on every call is detected and served by plain launches).  vqa_lstm_graph_stats reports
 *   replays / graph builds / plain-launch fallbacks since load and returns the number of cached graphs.
 * Layouts: time-major.  The forward direction reads state slot t and writes slot t+1 of Hs / Cs [T+1][B][H] at time
 * t, the reverse direction reads slot t+1 and writes slot t; the caller zeroes the initial slot (0, resp. T). */
typedef struct {
  const float* w_hh; /* [4H][H], PyTorch gate order i,f,g,o */
  const float* xg;   /* fwd: [T][B][4H] = x_t W_ih^T + b_ih + b_hh (vqa_gemm) */
  float* gates;      /* [T][B][4H] gate activations, zero rows where t >= q_len[b] (fwd: out, bwd: in) */
  float* Hs;         /* [T+1][B][H] */
  float* Cs;         /* [T+1][B][H] */
  float* c_final;    /* fwd: optional [B][cf_ld], final cell state c_n (the question feature, model.py:164-166) */
  float* dgates;     /* bwd: [T][B][4H] out: gradient w.r.t. the gate pre-activations */
  float* dh;         /* bwd: [B][H] work; on entry d loss / d h_n (zeros for this model), on exit d loss / d h at the first
                      * processed time: the total gradient w.r.t. the h that time WROTE (T == 1: the entry value).  It is
                      * not d loss / d h_0: that is dgates[first time] . W_hh + this value for the samples inactive there */
  float* dc;         /* bwd: [B][H] work; on entry d loss / d c_n, on exit d loss / d c at the first processed time: the
                      * gradient w.r.t. the c that time READ, i.e. d loss / d c_0 */
  int reverse;       /* 0: t = 0 .. T-1, 1: t = T-1 .. 0 */
} vqa_lstm_dir_t;
int vqa_lstm_step_supported(int H);
int vqa_lstm_seq_fwd(const vqa_lstm_dir_t* dirs, int ndir, const int64_t* q_len, int B, int T, int H,
                     int64_t cf_ld, int use_graph, vqa_stream_t stream);
int vqa_lstm_seq_bwd(const vqa_lstm_dir_t* dirs, int ndir, const int64_t* q_len, int B, int T, int H,
                     int use_graph, vqa_stream_t stream);
int vqa_lstm_graph_stats(int* replays, int* builds, int* plain);

/* ---- attention (models/model.py:169-195 Attention, 208-221 image_question_attention) ---------
 * x = relu(v' (+|*) q') comes from vqa_gemm(rowgroup = q') as xs[m][n]; for do_option '|' (model.py:192)
 * x = relu(cat[v', tile(q')]) has 2*mid channels: xs holds the v' half and qcat = q' [B][mid] the other.
 * score[b][g][p] = bx[g] + sum_n dropout(x[b*P+p][n]) * wx[g*wx_ld + n]            (x_conv, model.py:194) */
int vqa_att_score_fwd(const void* xs, int xs_is_bf16 /* the bf16 path stores x as bf16 */, const float* wx, int wx_ld,
                      const float* bx, float* score, int B, int P, int mid, int G, float p, uint64_t seed,
                      const float* qcat /* '|' only */, vqa_stream_t stream);
/* Backward of the score + combine stage, in place on xs.  mode: 0 '+', 1 '*', 2 '|'.
 *   xs      <- gradient w.r.t. v' (what the v_conv dW / dX GEMMs consume)
 *   dq_part[b*RS+rs][mid]      partial sums of the gradient w.r.t. q' (RS = vqa_att_row_splits(P))
 *   dwx_part[b*RS+rs][G][xld]  partial sums of the x_conv weight gradient, xld = mid (2*mid for '|')
 * '*' needs vprime = the raw v' (aux output of the forward GEMM) and qp = q'; '|' needs qp.
 * Both entry points return VQA_ERR_INVALID, before any HIP call, for: G outside 1..4, a null pointer (those the mode
 * needs included), B < 0, P < 1, mid < 4 or not a multiple of 4, wx_ld not a multiple of 4 or below the channels of x,
 * p outside [0, 1), a mode outside 0..2, and a wx / qcat / qp / vprime / dwx_part / dq_part that is not 16-byte aligned.
 * B = 0 returns VQA_OK without a launch.  The alignment of xs selects the forward's kernel and is no error. */
int vqa_att_row_splits(int P);
int vqa_att_score_bwd(const float* dscore, const float* wx, int wx_ld, void* xs_inout, int xs_is_bf16, float* dwx_part,
                      float* dq_part, int B, int P, int mid, int G, float p, uint64_t seed, int mode,
                      const float* vprime, const float* qp, vqa_stream_t stream);
/* probs = softmax_p(score); out[b*out_ld + g*C + c] = sum_p probs[b][g][p] * vn[b][p][c] */
int vqa_att_apply_fwd(const float* score, const float* vn, float* probs, float* out, int64_t out_ld,
                      int B, int P, int C, int G, vqa_stream_t stream);
/* Many questions per image (inference; VqaNet.encode_images / answer).  One v' = v_conv(vn) [N*P][mid] per IMAGE, the
 * questions grouped by image: order[offsets[n] .. offsets[n+1]) are the questions of image n (device int32; order [B] a
 * permutation of 0..B-1, offsets [N+1] non-decreasing from 0 to B).  x = relu(v' (+|*) q') is never written:
 *   mode 0 '+', 1 '*':  score[b][g][p] = bx[g] + sum_m wx[g*wx_ld + m] * relu(v'[n*P+p][m] (+|*) qp[b][m])
 *   mode 2 '|':         score[b][g][p] = bx[g] + sum_m wx[g*wx_ld + m] * relu(v'[n*P+p][m])
 *                                              + sum_m wx[g*wx_ld + mid + m] * relu(qp[b][m])
 * A workgroup keeps a tile of positions of one image in LDS and walks that image's questions over it: v' is read once
 * per image, an image without questions costs nothing.  No atomics: every element has one summation order whatever the
 * grouping.  mid % 4 == 0, mid <= 4096, wx_ld % 4 == 0, G in 1..4, N <= 65535; vprime, qp, wx 16-byte aligned. */
int vqa_att_score_grouped_fwd(const float* vprime, const float* qp, const float* wx, int wx_ld, const float* bx,
                              const int32_t* order, const int32_t* offsets, float* score, int N, int B, int P, int mid,
                              int G, int mode, vqa_stream_t stream);
/* vqa_att_apply_fwd with an image index (device int32 [B], entries in [0, N)): vn is [N][P][C],
 * probs = softmax_p(score[b][g][:]); out[b*out_ld + g*C + c] = sum_p probs[b][g][p] * vn[img[b]][p][c].
 * With img = 0..B-1 the results equal vqa_att_apply_fwd's bit for bit (same device code). */
int vqa_att_apply_gather_fwd(const float* score, const float* vn, const int32_t* img, float* probs, float* out,
                             int64_t out_ld, int N, int B, int P, int C, int G, vqa_stream_t stream);
/* dscore[b][g][p] and dvn[b][p][c] (written; NULL: skipped, see vqa_l2norm_bwd_joined) from dout[b*dout_ld + g*C + c]; dscore_rowsum (optional)
 * [b][g] = sum_p dscore[b][g][p], the per-sample part of the x_conv bias gradient. */
int vqa_att_apply_bwd(const float* dout, int64_t dout_ld, const float* probs, const float* vn,
                      float* dscore, float* dvn, float* dscore_rowsum, int B, int P, int C, int G,
                      vqa_stream_t stream);

/* ---- training through shared image features (VqaNet.forward_shared): the attention stage with one v' per IMAGE ----------
 * Grouping as in vqa_att_score_grouped_fwd: order[offsets[n] .. offsets[n+1]) are the questions of image n (device int32).
 * No entry point below uses atomics: the same inputs give the same bits on every run.
 *
 * vqa_att_score_grouped_fwd with the x_conv dropout (attention.drop on x, models/model.py:194) applied to
 * x = relu(v' (+|*) q') before the product: x[b][p][m] *= keep(seed, (b*P + p)*xld + m) / (1-p) over the logical tensor
 * [B][P][xld] indexed by the QUESTION b (xld = mid, 2*mid for '|' where the q' half takes channel mid + m) -- the mask
 * vqa_att_score_fwd applies to a materialised x.  p = 0 runs the device code of vqa_att_score_grouped_fwd (same bits). */
int vqa_att_score_grouped_drop_fwd(const float* vprime, const float* qp, const float* wx, int wx_ld, const float* bx,
                                   const int32_t* order, const int32_t* offsets, float* score, int N, int B, int P, int mid,
                                   int G, int mode, float p, uint64_t seed, vqa_stream_t stream);
/* vqa_att_apply_bwd where sample b weighted the rows of image img[b] (device int32 [B], entries in [0, N);
 * models/model.py:208-221 backward); vn is [N][P][C].
 *   dscore[b][g][p], dscore_rowsum[b][g] (optional)      as vqa_att_apply_bwd, reading vn[img[b]]
 *   dvn[n][p][c] = sum_{b in n} sum_g probs[b][g][p] * dout[b*dout_ld + g*C + c]      the weighted-sum branch of d loss / d vn,
 * summed per image in the order of `order`; every row is written, zeros for an image without questions.  C % 4 == 0,
 * dout_ld % 4 == 0; dout, vn, dvn 16-byte aligned.  With N = B and img = order = 0..B-1 the results equal vqa_att_apply_bwd's
 * bit for bit (the same row kernel in its (sample, image) form). */
int vqa_att_apply_gather_bwd(const float* dout, int64_t dout_ld, const float* probs, const float* vn, const int32_t* img,
                             const int32_t* order, const int32_t* offsets, float* dscore, float* dvn, float* dscore_rowsum,
                             int N, int B, int P, int C, int G, vqa_stream_t stream);
/* Backward of vqa_att_score_grouped_drop_fwd (models/model.py:186-194 backward); x is recomputed from v' and q', never read.
 * With dxpre[b][p][m] = (x > 0) * mask[b][p][m] * sum_g dscore[b][g][p] * wx[g*wx_ld + m]  (mask as in the forward):
 *   dvprime[n*P+p][m]          '+': sum_{b in n} dxpre;  '*': sum_{b in n} dxpre * qp[b][m];  '|': as '+' with x = relu(v'),
 *                              the v' half only; zero rows for an image without questions; every row is written
 *   dq_part[b*NT+t][mid]       partial sums over the positions of tile t (NT = vqa_att_score_grouped_tiles(P)) of
 *                              '+': dxpre;  '*': dxpre * v'[n*P+p][m];  '|': (qp > 0) * mask[b][p][mid+m] * sum_g dscore * wx[g][mid+m]
 *                              -- vqa_sum_parts(batch B, parts NT) finishes d loss / d q'
 *   dwx_part[n*NT+t][G][xld]   partial sums over the tile's positions and the image's questions of dscore * x * mask (both
 *                              halves for '|') -- vqa_colsum over the N*NT rows finishes the x_conv weight gradient
 * mode: 0 '+', 1 '*', 2 '|'.  mid % 4 == 0, mid <= 4096, wx_ld % 4 == 0, G in 1..4, N <= 65535, 0 <= p < 1; every float
 * pointer except dscore 16-byte aligned.  B == 0 returns without a launch. */
int vqa_att_score_grouped_tiles(int P);
int vqa_att_score_grouped_bwd(const float* dscore, const float* vprime, const float* qp, const float* wx, int wx_ld,
                              const int32_t* order, const int32_t* offsets, float* dvprime, float* dq_part, float* dwx_part,
                              int N, int B, int P, int mid, int G, int mode, float p, uint64_t seed, vqa_stream_t stream);

/* ---- cached question features (VqaNet.encode_questions / answer_pairs): (image, question) pairs from two caches ----------
 * vqa_att_score_grouped_fwd (models/model.py:186-195: x = relu(v' (+|*) q'), x_conv) where pair b reads the q' row
 * qp[qrow[b]] instead of qp[b]: qp is [M][mid], one row per DISTINCT question, qrow device int32 [B].  Everything else is
 * still indexed by the pair b (order, offsets, the score row).  Same device code as vqa_att_score_grouped_fwd under a
 * compile-time flag, same per-lane operation order: score equals vqa_att_score_grouped_fwd on the expanded qp[qrow] bit
 * for bit.  A qrow[b] outside [0, M) skips pair b as a bad `order` entry is skipped: nothing is read, its score row is
 * left unwritten.  No atomics.  M >= 1; the other limits are vqa_att_score_grouped_fwd's.  B == 0 returns without a launch. */
int vqa_att_score_grouped_pairs_fwd(const float* vprime, const float* qp, const int32_t* qrow, const float* wx, int wx_ld,
                                    const float* bx, const int32_t* order, const int32_t* offsets, float* score, int N, int B,
                                    int M, int P, int mid, int G, int mode, vqa_stream_t stream);
/* dst[b*dst_ld + c] = src[rows[b]*src_ld + c] for b < B, c < cols: the question half of the classifier input
 * combined = cat[weighted v, q] (models/model.py:64) taken from cached question features, rows device int32 [B] with
 * entries in [0, M); an entry outside writes a row of zeros.  16-byte accesses when cols, both leading dimensions
 * (elements) and both pointers allow it, scalar otherwise.  src_ld, dst_ld >= cols.  B == 0 returns without a launch. */
int vqa_gather_rows(const float* src, int64_t src_ld, const int32_t* rows, float* dst, int64_t dst_ld, int B, int M, int cols,
                    vqa_stream_t stream);

/* ---- training on cached image features (VqaNet.forward_features): a frozen image encoder, a bank of feature rows --------
 * Neither entry point uses atomics, and neither launches work that grows with the size of the bank.
 *
 * The asked rows of a bank, compacted and dropped in one pass (attention.drop on v, models/model.py:185, with the mask
 * indexed by the BANK row, as if it had been drawn over the whole bank):
 *   dst[j*row_len + i] = src[rows[j]*row_len + i] * keep(seed, rows[j]*row_len + i) / (1-p)      j < n, i < row_len
 * src is [M][row_len], dst [n][row_len], rows device int32 [n]; the flat index is 64-bit (the mask vqa_dropout applies to
 * the whole bank).  p = 0 is a pure copy; a rows[j] outside [0, M) writes a row of zeros.  16-byte accesses when
 * row_len % 4 == 0 and both pointers are 16-byte aligned, scalar otherwise (same bits).  The flat range n * row_len is
 * spread over a capped grid, so one long row fills the device.  n >= 0, M >= 1, row_len >= 1, 0 <= p < 1; n == 0 returns
 * without a launch. */
int vqa_gather_rows_drop(const float* src, const int32_t* rows, float* dst, int n, int M, int64_t row_len, float p,
                         uint64_t seed, vqa_stream_t stream);
/* vqa_att_apply_gather_bwd without the per-image sum dvn (the image encoder is frozen: nobody reads d loss / d vn):
 * dscore [B][G][P] and dscore_rowsum [B][G] (optional) from the same device code, bit for bit; vn is [N][P][C] and only the
 * rows img[b] are read.  Limits as vqa_att_apply_gather_bwd: C % 4 == 0, dout_ld % 4 == 0, dout_ld >= G*C, G in 1..4,
 * N >= 1; dout and vn 16-byte aligned.  B == 0 returns without a launch. */
int vqa_att_apply_gather_dscore(const float* dout, int64_t dout_ld, const float* probs, const float* vn, const int32_t* img,
                                float* dscore, float* dscore_rowsum, int N, int B, int P, int C, int G, vqa_stream_t stream);

/* ---- image dropout on a bank of cached image features -------------------------------
 * src is a bank [M][P][C] of L2-normalised features, fp32 (vqa_gather_rows_drop_norm) or IEEE half (.._f16, widened on load:
 * the bits of the fp32 form on the same values); rows is device int32 [n].  For j < n, pos < P, c < C, with r = rows[j] and the
 * 64-bit bank index e = (r*P + pos)*C + c:
 *   u         = src[e] * keep(seed, e) / (1 - p)            the mask vqa_dropout(p, seed) applies to the whole bank
 *   nrm       = sqrt(sum over c of u^2)                     of the C channels of (j, pos)
 *   vn_out    [(j*P + pos)*C + c] = u * (1 / (nrm + 1e-12f))    the operations of vqa_l2norm_fwd
 *   vdrop_out [(j*P + pos)*C + c] = vn_out[..] * keep(seed2, e) / (1 - p2)
 * Normalisation is scale-invariant, so on a bank that holds vn = pooled / (|pooled| + 1e-12) this is image.drop followed by
 * the L2 normalisation of the same pooled features, up to how the 1e-12 guard scales; a feature row whose kept part is all
 * zero gives zeros.  vdrop_out is optional: null writes vn_out alone, and p2 and seed2 are then ignored.  A rows[j] outside
 * [0, M) writes zeros to both outputs.  p = 0 renormalises a row (not a bit-exact copy).
 * VQA_ERR_INVALID, before any HIP call, for: a null src, rows or vn_out; n < 0; M < 1; P < 1; C < 4 or C % 4 != 0; p (or, with
 * vdrop_out, p2) outside [0, 1); a src that is not 16-byte (half: 8-byte) aligned; an output that is not 16-byte aligned.
 * n == 0 returns VQA_OK without a launch.  One wave per feature row, no LDS; neither the grid nor the bytes moved depend on M. */
int vqa_gather_rows_drop_norm(const float* src, const int32_t* rows, float* vn_out, float* vdrop_out, int n, int M, int P, int C,
                              float p, uint64_t seed, float p2, uint64_t seed2, vqa_stream_t stream);
int vqa_gather_rows_drop_norm_f16(const void* src_f16, const int32_t* rows, float* vn_out, float* vdrop_out, int n, int M, int P,
                                  int C, float p, uint64_t seed, float p2, uint64_t seed2, vqa_stream_t stream);

/* ---- gradient x input attribution from cached image features (inference; csrc/att_apply.hip, csrc/att_score.hip) ----
 * For question b about image n = img[b] and a chosen answer column a_b, the map at the L2-normalised features vn (eval mode,
 * no dropout, the question held fixed):
 *   R[b][p] = sum_c vn[n][p][c] * d logit[b][a_b] / d vn[n][p][c]
 * vn reaches the logit through the weighted sum and through the scores via v' = v_conv(vn) = vn . Wv^T.  With
 * dwv[b][g][c] = d logit[b][a_b] / d combined[b][g*C + c] (the caller's dout, row stride dout_ld):
 *   t[b][g][p]      = vn[n][p][:] . dwv[b][g][:]
 *   r1[b][p]        = sum_g probs[b][g][p] * t[b][g][p]
 *   dscore[b][g][p] = probs[b][g][p] * (t[b][g][p] - sum_p' probs[b][g][p'] * t[b][g][p'])
 *   c[b][p][m]      = sum_g dscore[b][g][p] * wx[g][m]                      ('|': the first mid columns of wx)
 *   r2[b][p]        = sum_m c[b][p][m] * s[b][p][m] * v'[n][p][m]
 *                     '+': s = [v' + q' > 0]     '*': s = [v' * q' > 0] * q'     '|': s = [v' > 0]
 *   R[b][p]         = r1[b][p] + r2[b][p]
 * r2 uses sum_c vn[p][c] * sum_m dv'[p][m] * Wv[m][c] = sum_m dv'[p][m] * v'[p][m]: nothing of shape [B][P][C] or [B][P][mid]
 * is formed and v_conv does not run.
 *   vqa_att_attr_apply_gather / _f16: vqa_att_apply_gather_dscore (/ _f16) -- the same arguments, limits and alignment rules,
 *     the same device code and therefore the same dscore and dscore_rowsum bits -- that also writes r1 [B][P] (g ascending)
 *     from t before the softmax backward overwrites it.
 *   vqa_att_attr_score_grouped / _pairs / _f16 / _pairs_f16: out [B][P] = r1 + r2 from r1 [B][P], dscore [B][G][P], v'
 *     [N*P][mid] (fp32, or half for a float16 cache, 8-byte aligned), q' [B][mid] (pairs: the table [M][mid] read through qrow
 *     [B]; NULL allowed for '|', which reads no q') and wx [G][wx_ld].  The ownership, checks, limits and path choice of
 *     vqa_att_score_grouped_fwd: a workgroup stages a tile of positions of ONE image in LDS and walks that image's questions;
 *     no atomics; one summation order per (b, p) (a lane's channel quads lane*4 + 256*i in ascending i, x, y, z, w inside a
 *     quad, then the wave butterfly) whatever the grouping.  Every (b, p) of a question listed in order / offsets is written
 *     exactly once; rows of questions that are not listed, and every row when an image has no question, are left alone.  The
 *     pairs form equals the plain form on qp[qrow], the half form the fp32 form on the widened v', bit for bit.
 *   vqa_att_attr_score_grouped_path: the kernel those four run for (mode, mid) -- 0: the register kernel ('+' / '*', mid =
 *     256 * IT <= 1024), else the general kernel with that many positions per wave (4, 2 or 1). */
int vqa_att_attr_apply_gather(const float* dout, int64_t dout_ld, const float* probs, const float* vn, const int32_t* img,
                              float* dscore, float* dscore_rowsum, float* r1, int N, int B, int P, int C, int G,
                              vqa_stream_t stream);
int vqa_att_attr_apply_gather_f16(const float* dout, int64_t dout_ld, const float* probs, const void* vn_f16,
                                  const int32_t* img, float* dscore, float* dscore_rowsum, float* r1, int N, int B, int P, int C,
                                  int G, vqa_stream_t stream);
int vqa_att_attr_score_grouped_path(int mode, int mid);
int vqa_att_attr_score_grouped(const float* r1, const float* dscore, const float* vprime, const float* qp, const float* wx,
                               int wx_ld, const int32_t* order, const int32_t* offsets, float* out, int N, int B, int P, int mid,
                               int G, int mode, vqa_stream_t stream);
int vqa_att_attr_score_grouped_pairs(const float* r1, const float* dscore, const float* vprime, const float* qp,
                                     const int32_t* qrow, const float* wx, int wx_ld, const int32_t* order, const int32_t* offsets,
                                     float* out, int N, int B, int M, int P, int mid, int G, int mode, vqa_stream_t stream);
int vqa_att_attr_score_grouped_f16(const float* r1, const float* dscore, const void* vprime_f16, const float* qp, const float* wx,
                                   int wx_ld, const int32_t* order, const int32_t* offsets, float* out, int N, int B, int P,
                                   int mid, int G, int mode, vqa_stream_t stream);
int vqa_att_attr_score_grouped_pairs_f16(const float* r1, const float* dscore, const void* vprime_f16, const float* qp,
                                         const int32_t* qrow, const float* wx, int wx_ld, const int32_t* order,
                                         const int32_t* offsets, float* out, int N, int B, int M, int P, int mid, int G, int mode,
                                         vqa_stream_t stream);

/* ---- gradient x input per question token (inference, VqaNet.explain_words; csrc/att_score.hip, csrc/elementwise.hip) ----
 * For question b, token slot t and the chosen answer column a_b, with e[b][t][:] = emb[q[b][t]] the embedding output before
 * tanh (eval mode, no dropout, the image features held fixed):
 *   words[b][t] = sum_e e[b][t][e] * d logit[b][a_b] / d e[b][t][e]
 * The question reaches the logit through the question half of the classifier input and through q' = q_lin(qf) in the
 * attention scores.  These two entry points are the ends of that chain; between them run products the library already has
 * (the q_lin data gradient, the LSTM backward through time, dgates . W_ih) and no parameter gradient.
 *   vqa_att_attr_dq_grouped / _f16: d logit / d q' through the scores, from the dscore [B][G][P] of vqa_att_attr_apply_gather:
 *       dxpre[b][p][m]  = [x > 0] * sum_g dscore[b][g][p] * wx[g*wx_ld + m]         x = v'[n*P+p][m] (+|*) q'[b][m], n the image of b
 *       dq_part[b*NT+t][m] = sum over the positions p of tile t of   '+': dxpre      '*': dxpre * v'[n*P+p][m]
 *     with NT = vqa_att_score_grouped_tiles(P); vqa_sum_parts(batch B, parts NT) finishes dq_att [B][mid].  This is
 *     vqa_att_score_grouped_bwd at p = 0 without dvprime and dwx_part -- the same device code under a compile-time flag, the
 *     same ownership (16 positions of one image per workgroup, one channel quad per thread, the image's questions walked in
 *     `order`'s order), the same per-thread operation order -- so dq_part equals that entry point's bit for bit, and the half
 *     form (v' IEEE half, 8-byte aligned, widened on load) equals the fp32 form on the widened v' bit for bit.  No atomics, no
 *     LDS.  Rows of questions that are not listed in order / offsets are left alone.
 *     mode 0 '+' and 1 '*' only.  mode 2 ('|') is VQA_ERR_INVALID: there the q' half adds the same constant to every position's
 *     score and softmax is shift-invariant, so this gradient is identically zero -- a caller launches nothing for it.
 *     Limits and checks as vqa_att_score_grouped_bwd: mid % 4 == 0, mid <= 4096, wx_ld % 4 == 0, wx_ld >= mid, G in 1..4,
 *     N <= 65535; v' (fp32 form), qp, wx and dq_part 16-byte aligned.  B == 0 returns without a launch.
 *   vqa_embed_attr: the other end, from dx = dx0 + dx1 (dx1 may be NULL: a unidirectional encoder), the gradient at the
 *     embedding stage's output x = tanh(e) [T][B][E] that vqa_embed_tanh_fwd wrote (p = 0):
 *       words[b][t] = sum_e emb[q[b][t]*E + e] * (1 - x[t][b][e]^2) * (dx0[(t*B+b)*E + e] + dx1[(t*B+b)*E + e])
 *     q int64 [B][T], q_len int64 [B], words [B][T]: every element is written, +0.0 for t >= q_len[b] and for a token id
 *     outside [0, V) (which vqa_embed_tanh_fwd counts and reads as a zero row).  One wave per slot; lane l adds the terms of
 *     elements 4*(l + 64*i) + k in ascending i, then k, each term rounded before the add, then the wave butterfly: one order,
 *     whatever the grid.  16-byte accesses when E % 4 == 0 and emb, x, dx0, dx1 are 16-byte aligned, scalar otherwise (same
 *     bits).  B >= 0, T, E, V >= 1; B == 0 returns without a launch. */
int vqa_att_attr_dq_grouped(const float* dscore, const float* vprime, const float* qp, const float* wx, int wx_ld,
                            const int32_t* order, const int32_t* offsets, float* dq_part, int N, int B, int P, int mid, int G,
                            int mode, vqa_stream_t stream);
int vqa_att_attr_dq_grouped_f16(const float* dscore, const void* vprime_f16, const float* qp, const float* wx, int wx_ld,
                                const int32_t* order, const int32_t* offsets, float* dq_part, int N, int B, int P, int mid, int G,
                                int mode, vqa_stream_t stream);
int vqa_embed_attr(const int64_t* q, const float* emb, const float* x, const float* dx0, const float* dx1,
                   const int64_t* q_len, float* words, int B, int T, int E, int V, vqa_stream_t stream);

/* ---- occlusion maps from cached features (inference, VqaNet.explain_occlusion; csrc/occlusion.hip) ----
 * What the gradient x input maps estimate to first order, computed exactly: for question b about image n, answer column a_b and
 * every grid position p, how far logit[b][a_b] falls when the features vn[n][s][:] (hence v'[n][s][:]: v_conv has no bias) of the
 * positions s in S(p) are zero -- S(p) the window x window square centred on p, clipped at the grid border (eval mode, the
 * question held fixed):
 *   maps[b][p] = logit[b][a_b] - logit_occluded[b][a_b ; S(p)]
 * An occluded position scores cnull[b][g] (the score of a position whose v' is 0), so per glimpse g, with hid = the
 * classifier's hidden width and W1_g = columns [g*C, (g+1)*C) of lin1.weight,
 *   r[b][g]      = exp(cnull[b][g] - m) / sum_p exp(score[b][g][p] - m),   m = max_p score[b][g][p]
 *   mass[b][g][p] = sum_{s in S(p)} probs[b][g][s]
 *   alpha        = 1 / (1 - mass + |S(p)| * r)                    (> 0: r > 0)
 *   U[n][s][g][:] = W1_g . vn[n][s][:]       Z[b][g][:] = W1_g . out[b][g][:]       base[b][:] = b1 + W1[:, G*C:] . qf[b]
 *   pre'[h]      = base[b][h] + sum_g alpha[b][g][p] * (Z[b][g][h] - sum_{s in S(p)} probs[b][g][s] * U[n][s][g][h])
 *   logit_occluded = W2[a_b][:] . relu(pre') + b2[a_b]
 * base [B][hid], Z [B][G][hid], probs and score [B][G][P] (P = gh * gw), cnull [B][G], answers int32 [B], maps [B][P].  U holds
 * the rows of R images, [R][P][G][hid]; question b reads row slot[b] - slot0 of it, and a question whose row is outside [0, R)
 * is LEFT ALONE -- a caller whose U does not fit one buffer walks it in chunks of images and every question is written by
 * exactly one of the calls.  A column a_b outside [0, A) gives a row of zeros.
 * One workgroup per (question, 16 consecutive positions): its head stages base, Z and W2[a_b] in LDS and forms r by a block
 * reduction (the same order in every workgroup of the question); then one wave per position, lane l over the quads l, l + 64,
 * ... of hid with 16-byte loads, the window's positions row by row, g ascending, and the wave butterfly.  One summation order
 * per (b, p), no atomics, every element written once: permuting the questions permutes the rows of maps bit for bit.  r,
 * mass and alpha are fp32.  Conditioning: Z - sum probs * U is a difference of like-sized numbers whose rounding error alpha
 * multiplies; alpha grows as the window swallows the attention mass (DESIGN.md 4.18 has the measured error).
 * Limits: hid % 4 == 0, w2_ld % 4 == 0, (G + 2) * hid * 4 + 80 <= 65536 bytes of LDS, G in 1..4, window odd in 1..7, base, Z,
 * U and W2 16-byte aligned; anything else is VQA_ERR_INVALID before any HIP call.  B == 0 returns without a launch. */
int vqa_occl_logit(const float* base, const float* Z, const float* U, const int32_t* slot, int slot0, const float* probs,
                   const float* score, const float* cnull, const float* W2, int64_t w2_ld, const float* b2,
                   const int32_t* answers, const float* logits, int64_t logits_ld, float* maps, int R, int B, int gh, int gw,
                   int hid, int G, int A, int window, vqa_stream_t stream);

/* ---- exact word occlusion from cached features (inference, VqaNet.explain_words_occlusion; csrc/lstm_occl.hip, DESIGN.md
 * 4.19) ----
 * What the per-token gradient x input values estimate to first order, computed exactly: for question b, answer column a_b and
 * every token slot t < q_len[b], how far logit[b][a_b] falls when the embedding output e[b][t][:] is the zero vector (eval
 * mode, the image features held fixed, the length and every other token unchanged):
 *   words[b][t] = logit[b][a_b] - logit_t[b][a_b]
 * The LSTM input of that step is tanh(0) = 0, so its gate pre-activation is b_ih + b_hh + h W_hh^T.  A variant is a pair
 * (b, t); zeroing slot t leaves the forward direction's state before t and the reverse direction's state after t as the base
 * run left them, so a variant's chain starts from that saved state and runs the remaining steps only.
 *   vqa_lstm_occl_cell_fwd: one step, time s, of n variant rows.  Row r is the variant (b, t) = (var_b[r], var_t[r]) (int32):
 *       s >= q_len[b]:  h_var[r], c_var[r] are left as they are (vqa_lstm_cell_fwd's rule for a finished sample)
 *       otherwise:      pre = (s == t ? xg0 : xg_base[s][b]) + hg[r]                  [4H], gate order i, f, g, o
 *                       c = sigmoid(f) * c + sigmoid(i) * tanh(g);   h = sigmoid(o) * tanh(c)
 *     with the device functions of vqa_lstm_cell_fwd's kernel, in place in h_var / c_var (row stride st_ld elements, the same
 *     for both).  xg_base [T][B][4H] is the base run's x-projection with both biases (vqa_gemm with bias1 = b_ih, bias2 =
 *     b_hh), hg [n][4H] = h_var . W_hh^T (vqa_gemm, before this call), q_len int64 [B].  xg0 [4H] is b_ih + b_hh in the
 *     base product's own bits for a zero input row: the caller obtains it from THE SAME vqa_gemm call as xg_base (same
 *     weight, biases and epilogue) on one all-zero input row -- the accumulator of a zero row is exactly +0 under every
 *     plan, and the epilogue that adds the two biases is the one the base rows went through.
 *     c_final (optional, leading dimension cf_ld): the new cell state is also written to row cf_row[r] of it (cf_row int32
 *     [n], NULL: row r) on every active step, so after a chain's last step it holds the final cell state.
 *     16-byte accesses when H % 4 == 0, st_ld % 4 == 0, cf_ld % 4 == 0 and xg_base, xg0, hg, h_var, c_var, c_final are
 *     16-byte aligned; scalar otherwise, same bits.  No LDS, no atomics; a row's result depends on that row alone; a row
 *     whose (b, t) is outside [0, B) x [0, T) is left alone.  n == 0 returns without a launch.  Null pointers, n < 0, B, T,
 *     H < 1, s outside [0, T), st_ld < H, cf_ld < H with c_final, cf_row without c_final: VQA_ERR_INVALID before any HIP call.
 *   vqa_occl_words: the tail.  h1 [n][hid] (leading dimension h1_ld) = relu(lin1(.)) of the n variant rows' classifier inputs:
 *       words[b][t] = logits[b][a_b] - (W2[a_b][:] . h1[r][:] + b2[a_b])         for the variant rows r = (b, t)
 *       words[b][t] = +0.0                                                       for t >= q_len[b]
 *     for the questions b in [b0, b0 + nb); words [B][T].  EVERY element of those nb rows is written by this call, and no
 *     other row is touched: a caller that walks the questions in chunks covers each row with exactly one call, and its
 *     variant rows must list every (b, t), t < min(q_len[b], T), of the call's questions once.  A column a_b outside [0, A)
 *     gives +0.0 for the whole row.  One wave per variant row; lane l adds the terms of the quads l + 64*i of hid in ascending
 *     i and, inside a quad, k = 0..3, each term rounded before the add, then the wave butterfly (vqa_embed_attr's order): one
 *     order whatever the grid.  16-byte loads when hid % 4 == 0, h1_ld % 4 == 0, w2_ld % 4 == 0 and h1, W2 are 16-byte
 *     aligned, scalar otherwise (same bits).  No LDS, no atomics.  nb == 0 returns without a launch; n == 0 writes the zeros.
 *     n > nb * T, a leading dimension below its row, T, hid, A < 1 or a null pointer: VQA_ERR_INVALID before any HIP call. */
int vqa_lstm_occl_cell_fwd(const float* xg_base, const float* xg0, const float* hg, float* h_var, float* c_var, int64_t st_ld,
                           const int64_t* q_len, const int32_t* var_b, const int32_t* var_t, int s, float* c_final, int64_t cf_ld,
                           const int32_t* cf_row, int n, int B, int T, int H, vqa_stream_t stream);
int vqa_occl_words(const float* h1, int64_t h1_ld, const float* W2, int64_t w2_ld, const float* b2, const int32_t* answers,
                   const float* logits, int64_t logits_ld, const int32_t* var_b, const int32_t* var_t, const int64_t* q_len,
                   float* words, int n, int b0, int nb, int T, int hid, int A, vqa_stream_t stream);

/* ---- deletion and insertion curves of an attribution map (inference, VqaNet.explain_faithfulness; csrc/faithfulness.hip,
 * DESIGN.md 4.20) ----
 * How well a map over the P grid positions ranks them: for question b about image n and answer column a_b, with order[b][:] the
 * positions by descending map value,
 *   insertion[b][k] = logit[b][a_b] with only the positions order[b][0 .. k) present
 *   deletion[b][k]  = logit[b][a_b] with the positions order[b][0 .. k) absent                      k = 0 .. P
 * "absent" in the sense of vqa_occl_logit: the rows of vn and v' are zero, so the position keeps the score cnull[b][g].  Both
 * are computed in the KEPT FORM, for the kept set K (order[b][0 .. k) for insertion, order[b][k .. P) for deletion), with r,
 * cnull, base and U as vqa_occl_logit defines them:
 *   m[b][g]      = sum_{s in K} probs[b][g][s]
 *   acc[b][g][:] = sum_{s in K} probs[b][g][s] * U[n][s][g][:]
 *   alpha[b][g]  = 1 / (m + (P - |K|) * r[b][g])
 *   logit_K      = W2[a_b][:] . relu(base[b] + sum_g alpha * acc[b][g]) + b2[a_b]
 * Sums over what remains: nothing is subtracted, so neither the Z - sum nor the 1 - mass cancellation of vqa_occl_logit occurs
 * and Z is not an operand.  deletion[b][0] and insertion[b][P] are the full logit by this route, deletion[b][P] and
 * insertion[b][0] the logit of the empty image, bit-equal to each other.
 *   vqa_rank_desc: order int32 [B][P] from maps fp32 [B][P] under ONE total order -- larger value first, equal values by the
 *     smaller position (vqa_softmax_topk's rule); -0.0 and +0.0 are equal; every NaN ranks below -inf, several NaNs by position.
 *     Each float becomes a monotone 32-bit key and rank[p] = #{s : key[s] > key[p] or (key[s] == key[p] and s < p)}, order[rank[p]]
 *     = p: a permutation of 0 .. P-1 for any input.  One workgroup per row, the row's keys in LDS; 1 <= P <= 8192, anything else
 *     is VQA_ERR_INVALID before any HIP call.  B == 0 returns without a launch.
 *   vqa_occl_curves_chunk: L, the compile-time number of steps per chunk of the ranking (16).
 *   vqa_occl_curves: the operands of vqa_occl_logit without Z, window, logits and maps, plus order int32 [B][P] (any int32
 *     values: an entry outside [0, P) adds nothing to m and acc and is never used as an address; it still counts as a step, so
 *     |K| is the number of steps), a workspace of vqa_occl_curves_workspace_bytes(B, P, G, hid) bytes, and deletion / insertion
 *     [B][P + 1].  Three launches.  (1) one wave per (b, chunk of L steps): the chunk's sum of probs * U rows, its steps in
 *     ascending order from 0, and of the weights.  (2) per element, over the chunks: the sums of the chunks before each chunk,
 *     ascending, and of the chunks after it, descending.  (3) one wave per (b, chunk), four chunks per workgroup, whose head
 *     stages base and W2[a_b] in LDS and forms r by vqa_occl_logit's two block reductions: the insertion sums start from the
 *     chunk's prefix and add its rows forward, the deletion sums start from its suffix and add its rows backward, the masses
 *     likewise; lane l over the quads l, l + 64, ... of hid with 16-byte loads, g ascending, and the wave butterfly per step.
 *     One summation order per (b, k), fixed by order[b] and L alone: it does not depend on the grid, on the batch or on how the
 *     images are chunked; no atomics; every element written once.  Permuting the questions permutes the rows bit for bit.
 *     A question whose row slot[b] - slot0 is outside [0, R) is LEFT ALONE (both outputs), as by vqa_occl_logit; a column a_b
 *     outside [0, A) gives two rows of +0.0.
 *     Limits: hid % 4 == 0, w2_ld % 4 == 0, 2 * hid * 4 + 80 <= 65536 bytes of LDS, G in 1..4, P <= 2^20, base, U, W2 and the
 *     workspace 16-byte aligned, the workspace large enough; anything else is VQA_ERR_INVALID before any HIP call.  B == 0
 *     returns without a launch and needs no workspace. */
int vqa_rank_desc(const float* maps, int32_t* order, int B, int P, vqa_stream_t stream);
int vqa_occl_curves_chunk(void);
int64_t vqa_occl_curves_workspace_bytes(int B, int P, int G, int hid);
int vqa_occl_curves(const float* base, const float* U, const int32_t* slot, int slot0, const float* probs, const float* score,
                    const float* cnull, const float* W2, int64_t w2_ld, const float* b2, const int32_t* answers,
                    const int32_t* order, float* workspace, int64_t workspace_bytes, float* deletion, float* insertion, int R,
                    int B, int P, int hid, int G, int A, vqa_stream_t stream);

/* ---- sampled Shapley maps (inference, VqaNet.explain_shapley; csrc/faithfulness.hip) ----
 * The Shapley value of grid position p for the set function f_b(S) = logit[b][a_b] with only the positions S present ("absent"
 * as above: the rows of vn and v' zero; eval mode, the question held fixed), estimated from M orders of the positions and their
 * reverses.  orders int32 [M][P], every row a permutation of 0 .. P-1, is ONE table shared by every question of the call: each
 * question's estimate is unbiased, only the errors of different questions become correlated, and a row of the result depends
 * on its question and the table alone -- not on the batch, its order or its split.  With ins_m, del_m the insertion and
 * deletion curves of question b along orders[m] (vqa_occl_curves' definition),
 *   e_m[b][orders[m][k]] = 0.5 * ((ins_m[k+1] - ins_m[k]) + (del_m[k] - del_m[k+1]))                 k = 0 .. P-1
 * the mean of the marginal contribution of that position under orders[m] (the insertion step) and under its reverse (the
 * deletion curve read backwards is the insertion curve of the reversed order: insertion_rev[k] = deletion[P-k]).  Then
 *   maps[b][p]   = mean over m of e_m[b][p]
 *   stderr[b][p] = sqrt(sum_m (e_m - maps)^2 / (M (M - 1))),  NaN for M == 1
 * Every e_m telescopes: sum_p e_m[b][p] = ins_m[P] - ins_m[0] up to rounding, so the maps sum to the logit minus the logit of
 * the empty image, ins_m[b][0] (bit-equal for every m).
 *   vqa_occl_curves_orders: vqa_occl_curves over the (question, order) pairs.  The operands of vqa_occl_curves with orders int32
 *     [M][P] in place of order [B][P], a workspace of vqa_occl_curves_orders_workspace_bytes(B, M, P, G, hid) bytes (M times
 *     vqa_occl_curves'), and deletion / insertion [B][M][P + 1].  The same three kernels, whose tasks are the pairs t = b * M + m
 *     (one place maps a task to its question row, its order row and its output row); row (b, m) holds, bit for bit, what
 *     vqa_occl_curves gives question b with orders[m] as its order.  Slot window, columns outside [0, A) (+0.0 rows), entries
 *     outside [0, P), limits and refusals are vqa_occl_curves'; in addition M >= 1 and B * M < 2^31 and the grids of B * M
 *     tasks must fit, else VQA_ERR_INVALID before any HIP call.  No atomics; LDS as vqa_occl_curves.
 *   vqa_shapley_accumulate: the curves of one group of Mg orders (deletion, insertion [B][Mg][P + 1]) into the running state.
 *     rank int32 [Mg][P] is the inverse of each order of the group (rank[m][orders[m][k]] = k; an entry outside [0, P) is no
 *     address and gives e = 0).  One thread owns (b, p) and folds the group in ascending m by Welford's update in fp32,
 *       d = e - mean;  mean += d / (m0 + m + 1);  M2 = fma(d, e - mean, M2)
 *     on mean, M2 [B][P]; m0 is the number of orders folded before this group (m0 == 0 starts from zero and reads no state).
 *     One sequence of roundings per (b, p): the bits do not depend on how the orders are grouped into launches.  total == 0:
 *     the state alone is written.  total == m0 + Mg (the last group): also maps = mean and err = stderr as above.  empty
 *     (optional, [B]) with m0 == 0: empty[b] = ins_0[b][0] of the group's first order, the logit of the empty image.  A question
 *     whose slot is outside [slot0, slot0 + R) is left alone; a column a_b outside [0, A) gives state, maps, err and empty of +0.0.
 *     Null pointers (maps, err may be NULL when total == 0), Mg < 1, m0 < 0, another total, P outside 1..2^20, R, A < 1 or a
 *     grid that does not fit: VQA_ERR_INVALID before any HIP call.  B == 0 returns without a launch.  No LDS, no atomics. */
int64_t vqa_occl_curves_orders_workspace_bytes(int B, int M, int P, int G, int hid);
int vqa_occl_curves_orders(const float* base, const float* U, const int32_t* slot, int slot0, const float* probs,
                           const float* score, const float* cnull, const float* W2, int64_t w2_ld, const float* b2,
                           const int32_t* answers, const int32_t* orders, float* workspace, int64_t workspace_bytes,
                           float* deletion, float* insertion, int R, int B, int M, int P, int hid, int G, int A,
                           vqa_stream_t stream);
int vqa_shapley_accumulate(const float* deletion, const float* insertion, const int32_t* rank, const int32_t* slot, int slot0,
                           const int32_t* answers, float* mean, float* m2, float* maps, float* err, float* empty, int R, int B,
                           int P, int Mg, int m0, int total, int A, vqa_stream_t stream);

/* ---- probability curves: the curve walk that keeps its hidden rows (inference, VqaNet.explain_faithfulness_probs;
 * csrc/faithfulness.hip) ----
 * vqa_occl_curves collapses every kept set's hidden row onto ONE row of W2, so it can follow one logit.  A probability, or the
 * arg-max, of a kept set needs every column: this entry point stops one step earlier and writes the hidden rows themselves,
 *   H[b][0][k][:] = relu(base[b] + sum_g alpha[b][g] * acc[b][g])   of the kept set order[b][k .. P)   (deletion)
 *   H[b][1][k][:] = the same                                         of the kept set order[b][0 .. k)   (insertion)   k = 0 .. P
 * with m, acc and alpha as vqa_occl_curves defines them, so that H . W2^T + b2 (one GEMM over the 2 (P + 1) rows of every
 * question) holds every column's logit of every step.  The hidden rows do not depend on the explained column.
 *   vqa_occl_curves_hidden: the operands of vqa_occl_curves without W2, w2_ld, b2, answers and A, a workspace of
 *     vqa_occl_curves_workspace_bytes(B, P, G, hid) bytes (the same layout), and hidden fp32 [B][2][P + 1][hid] in place of
 *     deletion / insertion.  The same three launches: (1) and (2) are vqa_occl_curves' kernels as they are; (3) is its walk
 *     under a compile-time flag -- the same chunks of L steps, alphas, forward / backward accumulation and fmaf chain, but
 *     the head loads no W2, there is no dot product and no wave butterfly: after the chain lane l stores max(pre, 0) as one
 *     float4 per state per quad (64 lanes write 1 KiB contiguous).  Every element of a listed question is written once:
 *     insertion state 0 by chunk 0 alone, deletion state P by the last chunk alone.  One summation order per (b, k), that of
 *     vqa_occl_curves: W2[a] . H[b][0][k] + b2[a] differs from its deletion[b][k] by the rounding of the dot product alone.
 *     H[b][0][P] and H[b][1][0] (the empty image) are bit-equal.  Permuting the questions permutes the rows bit for bit; it
 *     does not depend on the grid, the batch or the chunking of the images.  No atomics, no scratch.
 *     An order entry outside [0, P) adds nothing and is never an address; a question whose row slot[b] - slot0 is outside
 *     [0, R) is LEFT ALONE.
 *     Limits: hid % 4 == 0, hid * 4 + 80 <= 65536 bytes of LDS, G in 1..4, P <= 2^20, base, U, the workspace and hidden 16-byte
 *     aligned, the workspace large enough, no null pointer; anything else is VQA_ERR_INVALID before any HIP call.  B == 0
 *     returns without a launch and needs no workspace. */
int vqa_occl_curves_hidden(const float* base, const float* U, const int32_t* slot, int slot0, const float* probs,
                           const float* score, const float* cnull, const int32_t* order, float* workspace, int64_t workspace_bytes,
                           float* hidden, int R, int B, int P, int hid, int G, vqa_stream_t stream);

/* ---- integrated gradients from cached image features (inference, VqaNet.explain_integrated; csrc/att_score.hip) ----
 * The gradient x input map above, averaged along the straight path from the zero cache to the real one (eval mode, the
 * question held fixed, zero baseline).  For question b about image n, column a_b and S step positions alpha_s in (0, 1]:
 *   G_s[b][p] = sum_c vn[n][p][c] * d logit[b][a_b] / d x[p][c]   at x = alpha_s * vn[n]
 *   IG[b][p]  = scale * sum_s G_s[b][p]                            scale = 1 / S
 * v_conv has no bias, so x = alpha_s * vn[n] means v' = alpha_s * v'[n].  With the symbols of the attribution section at
 * step s (probs_s the softmax of score_s; dwv_s from h1_s = relu(lin1([alpha_s * sum_p probs_s vn, qf])); t_s = vn . dwv_s):
 *   r1_s[b][p]        = sum_g probs_s[b][g][p] * t_s[b][g][p]
 *   dscore_s[b][g][p] = probs_s * (t_s - sum_p' probs_s * t_s)      (vqa_att_attr_apply_gather on vn, without the factor alpha_s)
 *   c_s[b][p][m]      = sum_g dscore_s[b][g][p] * wx[g][m]
 *   r2_s[b][p]        = sum_m c_s[b][p][m] * s_s[b][p][m] * (alpha_s * v'[n][p][m])
 *                       '+': s_s = [alpha_s v' + q' > 0]   '*': s_s = [(alpha_s v') q' > 0] * q'   '|': s_s = [alpha_s v' > 0]
 *   G_s = r1_s + r2_s
 * The step-rows (b, s) are laid out as a batch of B*S questions -- score and dscore [B][S][G][P], r1 [B][S][P] -- so the
 * apply-gather entry points run between the two walks with the image index repeated S times.
 *   vqa_att_path_score_grouped / _pairs / _f16 / _pairs_f16: the grouped forward at every step,
 *       score[b][s][g][p] = bx[g] + sum_m wx[g][m] * relu((alpha_s * v'[n*P+p][m]) (+|*) q'[b][m])
 *       '|': score[b][s][g][p] = (bx[g] + sum_m wx[g][m] * relu(alpha_s * v'[n*P+p][m])) + sum_m wx[g][mid+m] * relu(q'[b][m])
 *   vqa_att_path_attr_grouped / _pairs / _f16 / _pairs_f16: the path sum of the grouped attribution,
 *       out[b][p] = scale * sum_s (r1[b][s][p] + r2_s[b][p])       from r1 [B][S][P] and dscore [B][S][G][P]
 * alphas: device float [S], 1 <= S <= VQA_ATT_PATH_MAX_STEPS.  Evaluation order: x = alpha_s * v' is rounded to fp32 first, then
 * the element math of vqa_att_score_grouped_fwd / vqa_att_attr_score_grouped runs on x, so both walks see the same
 * pre-activation bits; per (b, s, p) the summation order is theirs (a lane's channel quads lane*4 + 256*i in ascending i, x,
 * y, z, w inside a quad, then the wave butterfly); the path sum adds r1 + r2_s in ascending s and multiplies by scale last.
 * Ownership, argument checks, limits and path choice are vqa_att_score_grouped_fwd's / vqa_att_attr_score_grouped's
 * (vqa_att_attr_score_grouped_path): a workgroup stages a tile of positions of ONE image in LDS once and walks that image's
 * questions, and per question its S steps -- v' is read from memory once per walk whatever S is.  No atomics; every (b, s, p)
 * / (b, p) of a listed question is written exactly once, so permuting or splitting the batch permutes the rows bit for bit;
 * rows of questions that are not listed are left alone.  The pairs forms equal the plain forms on qp[qrow], the half forms the
 * fp32 forms on the widened v', bit for bit.  '|' reads no q' in the attribution forms (qp may be NULL there).  A null
 * alphas or an S outside the range is VQA_ERR_INVALID before any HIP call; B == 0 returns without a launch.
 *   vqa_att_path_scale_rows: x[r*ld + c] *= alphas[r % S] for r < rows, c < cols (ld >= cols >= 1): the image half of the
 *     classifier input of the step-rows r = b*S + s, between the two walks (the weighted sum of alpha_s * vn is alpha_s times
 *     the weighted sum of vn, rounded once).  rows == 0 returns without a launch. */
#define VQA_ATT_PATH_MAX_STEPS 64
int vqa_att_path_scale_rows(float* x, int64_t ld, const float* alphas, int S, int64_t rows, int cols, vqa_stream_t stream);
int vqa_att_path_score_grouped(const float* vprime, const float* qp, const float* wx, int wx_ld, const float* bx,
                               const float* alphas, const int32_t* order, const int32_t* offsets, float* score, int N, int B,
                               int S, int P, int mid, int G, int mode, vqa_stream_t stream);
int vqa_att_path_score_grouped_pairs(const float* vprime, const float* qp, const int32_t* qrow, const float* wx, int wx_ld,
                                     const float* bx, const float* alphas, const int32_t* order, const int32_t* offsets,
                                     float* score, int N, int B, int M, int S, int P, int mid, int G, int mode,
                                     vqa_stream_t stream);
int vqa_att_path_score_grouped_f16(const void* vprime_f16, const float* qp, const float* wx, int wx_ld, const float* bx,
                                   const float* alphas, const int32_t* order, const int32_t* offsets, float* score, int N, int B,
                                   int S, int P, int mid, int G, int mode, vqa_stream_t stream);
int vqa_att_path_score_grouped_pairs_f16(const void* vprime_f16, const float* qp, const int32_t* qrow, const float* wx, int wx_ld,
                                         const float* bx, const float* alphas, const int32_t* order, const int32_t* offsets,
                                         float* score, int N, int B, int M, int S, int P, int mid, int G, int mode,
                                         vqa_stream_t stream);
int vqa_att_path_attr_grouped(const float* r1, const float* dscore, const float* vprime, const float* qp, const float* wx,
                              int wx_ld, const float* alphas, float scale, const int32_t* order, const int32_t* offsets,
                              float* out, int N, int B, int S, int P, int mid, int G, int mode, vqa_stream_t stream);
int vqa_att_path_attr_grouped_pairs(const float* r1, const float* dscore, const float* vprime, const float* qp,
                                    const int32_t* qrow, const float* wx, int wx_ld, const float* alphas, float scale,
                                    const int32_t* order, const int32_t* offsets, float* out, int N, int B, int M, int S, int P,
                                    int mid, int G, int mode, vqa_stream_t stream);
int vqa_att_path_attr_grouped_f16(const float* r1, const float* dscore, const void* vprime_f16, const float* qp, const float* wx,
                                  int wx_ld, const float* alphas, float scale, const int32_t* order, const int32_t* offsets,
                                  float* out, int N, int B, int S, int P, int mid, int G, int mode, vqa_stream_t stream);
int vqa_att_path_attr_grouped_pairs_f16(const float* r1, const float* dscore, const void* vprime_f16, const float* qp,
                                        const int32_t* qrow, const float* wx, int wx_ld, const float* alphas, float scale,
                                        const int32_t* order, const int32_t* offsets, float* out, int N, int B, int M, int S,
                                        int P, int mid, int G, int mode, vqa_stream_t stream);

/* ---- loss head (train.py:190-207, utils/train_utils.py:12-25) -------------------------------
 * loss_rows[b] = sum_k -log_softmax(logits[b])[a_idx[b][k]-1] * a_val[b][k]/10 * inv_batch
 * score_rows[b] = min(1, 0.3 * a_val of the arg-max answer)
 * dlogits (optional) = d(sum_b loss_rows)/dlogits. a_idx is 1-based, 0 = padding. */
int vqa_softce_fwd_bwd(const float* logits, int64_t ld, const int64_t* a_idx, const int64_t* a_val,
                       int kmax, int B, int A, float inv_batch, float* loss_rows, float* score_rows,
                       float* dlogits, int64_t dld, vqa_stream_t stream);

/* ---- the answers themselves (csrc/topk.hip; VqaNet.predict, dl_vqa_amd.topk_answers; the reference leaves this to
 * torch.max in utils/train_utils.py:12-25 and to the caller) -- the k best columns of every logits row with their softmax
 * probabilities, one launch.  idx[b][0..k) are the first k columns of row b under ONE total order:
 *   larger value first; equal values: smaller column first;
 *   -0.0 and +0.0 are equal; NaN ranks above +inf (torch.topk's order), several NaNs by column.
 * idx[b][0] is therefore exactly the arg-max vqa_softce_fwd_bwd takes the score at (torch.max: the first maximum).
 * Columns are 0-based positions in the row; the loss head's a_idx is 1-based, so a_idx - 1 names the same column.
 *   prob[b][j] = exp(x[idx[b][j]] - max) / sum_i exp(x[i] - max)   fp32, expf (not the fast intrinsic); the sum runs in a
 *                fixed order (per lane, then the wave butterfly; no atomics): the same input gives the same bits
 *   lse[b]     = max + log(sum)   (optional, NULL: not written)
 * A row that contains NaN gets NaN probabilities and a NaN lse (its idx are still the order above).  Infinities follow the
 * arithmetic: -inf entries beside finite ones get probability 0; a row whose maximum is +inf, or that is all -inf, gets
 * NaN probabilities (inf - inf) and a NaN lse.
 * 1 <= k <= 64, k <= A, A >= 1, ld >= A (elements); no alignment demand on logits or ld.  B == 0 returns without a launch.
 * Nothing outside idx[B][k], prob[B][k] and lse[B] is written. */
int vqa_softmax_topk(const float* logits, int64_t ld, int B, int A, int k, int32_t* idx /* [B][k] */, float* prob /* [B][k] */,
                     float* lse /* [B], optional */, vqa_stream_t stream);

/* ---- the probability of a GIVEN column beside the best one (csrc/topk.hip; VqaNet.explain_faithfulness_probs)
 * One launch over `rows` logits rows, one wave per row, the row read once into the wave's registers (A <= 3072; beyond that
 * through the cache, as vqa_softmax_topk).  Row r belongs to question b = r / rows_per_question, whose column is answers[b]:
 *   top[r], top_prob[r]  = idx[r][0], prob[r][0] of vqa_softmax_topk(k = 1) on the same rows, bit for bit: the same device code
 *                          (csrc/topk.hip softmax_topk_row), hence the same total order -- larger value first, equal values by the
 *                          smaller column, -0.0 equal to +0.0, NaN above +inf -- and the same fixed-order sum
 *   prob_at[r]           = exp(x[r][answers[b]] - max_r) / sum_r   top_prob's own expression with the row's own max and sum, so a
 *                          row whose given column is its arg-max holds the same bits in both; +0.0 for a column outside [0, A)
 *                          (never an address); NaN for a row that holds a NaN, as vqa_softmax_topk
 * rows >= 0, A >= 1, ld >= A (elements), rows_per_question >= 1 and a divisor of rows (answers holds rows / rows_per_question
 * int32 entries); anything else, or a null pointer with rows > 0, is VQA_ERR_INVALID before any HIP call.  rows == 0 returns
 * without a launch.  No alignment demand, no LDS, no atomics; nothing outside top[rows], top_prob[rows], prob_at[rows] is written. */
int vqa_softmax_pick(const float* logits, int64_t ld, int rows, int A, const int32_t* answers, int rows_per_question,
                     int32_t* top /* [rows] */, float* top_prob /* [rows] */, float* prob_at /* [rows] */, vqa_stream_t stream);

/* ---- reductions / pointwise helpers -------------------------------------------------------- */
/* out[n] (+)= sum_m x[m*ld + n]; if mask != NULL rows of x where mask[m*cols+n] == 4 are skipped
 * (conv bias gradient over dead pool windows). workspace: vqa_colsum_workspace_bytes(rows, cols). */
int64_t vqa_colsum_workspace_bytes(int64_t rows, int cols);
int vqa_colsum(const float* x, int64_t ld, const uint8_t* mask, int64_t rows, int cols, float* out,
               int accumulate, float* workspace, int64_t workspace_bytes, vqa_stream_t stream);
/* out[g] = sum_{b,p} x[b][g][p] */
int vqa_sum_bgp(const float* x, float* out, int B, int G, int P, vqa_stream_t stream);
/* out[b][n] = sum_r part[(b*parts + r)*cols + n] */
int vqa_sum_parts(const float* part, float* out, int batch, int parts, int cols, vqa_stream_t stream);
/* dx = dy * dropmask * (y > 0): backward of dropout(relu(.)) given y = relu output (model.py:201-204) */
int vqa_relu_drop_bwd(const float* y, const float* dy, float* dx, int64_t n, float p, uint64_t seed,
                      vqa_stream_t stream);
/* y[r*ldy + c] = a[r*lda + c] + (b ? b[r*ldb + c] : 0) for r < rows, c < cols (strided add / copy;
 * in-place allowed): gradient joins such as d(combined) = d(cat[v, q]) (models/model.py:64). */
int vqa_add2d(const float* a, int64_t lda, const float* b, int64_t ldb, float* y, int64_t ldy,
              int64_t rows, int cols, vqa_stream_t stream);

/* x[i] *= *scalar (scalar is a DEVICE pointer): chains an upstream loss gradient without a host sync */
int vqa_scale_by(float* x, int64_t n, const float* scalar, vqa_stream_t stream);

/* ---- input pipeline ----------------------------------------------------- */
/* y[i] = (float)x[i] for n IEEE half values: the dataset stores image features as fp16 [N,3,S,S]
 * (preprocessing/preprocess_images.py:39-53) and the reference casts them to fp32 on the HOST per sample
 * (preprocessing/data_preprocessing.py:167-176); here the fp16 batch is uploaded as is (half the PCIe bytes)
 * and widened on the device.  x and y 16-byte aligned or n small; layout unchanged (NCHW). */
int vqa_half_to_float(const void* x_f16, float* y, int64_t n, vqa_stream_t stream);

/* ---- image preprocessing (csrc/preprocess.hip; dl_vqa_amd.preprocess_images) -------------------------------------------
 * Raw RGB bytes -> the image tensor v [N,3,S,S] the entry points above start from, in ONE launch for a batch of images
 * of different sizes, bit for bit what the reference computes per image on the host through PIL and torchvision
 * (preprocessing/preprocess_images.py:8-15 _get_transformations, 50-52; evaluate_vqa.py:45-51 runs it when the processed
 * file is missing).  For one RGB uint8 image [H][W][3], target size S and central_fraction cf in (0, 1]:
 *   1. resize size: R = int(S / cf); the short side becomes R: W <= H ? (ow, oh) = (R, int(R * H / W))
 *                                                                       : (oh, ow) = (R, int(R * W / H))   (double division)
 *   2. resample: PIL's bilinear filter with antialiasing, separable, the horizontal pass first, the intermediate rounded
 *      and clipped to uint8; a pass whose output size equals its input size is skipped.  For an axis of n input and m
 *      output samples: scale = n / m, fs = max(scale, 1), support = fs, ss = 1 / fs; per output index i
 *        center = (i + 0.5) * scale, lo = max((int)(center - support + 0.5), 0), hi = min((int)(center + support + 0.5), n)
 *        w_x = max(0, 1 - |(x + lo - center + 0.5) * ss|) for x in [0, hi - lo), summed in that order in double and each
 *        divided by the sum; k_x = (int)(0.5 + w_x * 2^22);
 *        out[i] = clip((2^21 + sum_x in[lo + x] * k_x) >> 22, 0, 255)
 *      The tables are computed on the HOST in double exactly so (dl_vqa_amd/preprocess.py, cached per (n, m)); the
 *      kernel does integer arithmetic only.  A skipped pass is the table lo = i, len = 1, k = 2^22, which returns the byte.
 *   3. centre crop to S x S: top = round((oh - S) / 2.0), left = round((ow - S) / 2.0), halves to the EVEN integer
 *      (Python's round).  Only the window's rows and columns are computed: the tables hold its S entries per axis.
 *   4. float tail: x = (byte / 255 - mean[c]) / std[c] in fp32, mean = {0.485, 0.456, 0.406}, std = {0.229, 0.224, 0.225},
 *      then rounded to fp16: a function of (c, byte) alone, read from a 3 x 256 table `lut` the caller builds with the
 *      reference's own operations (fp16 entries, or fp32 entries without the last rounding when out_is_f32).
 *   5. out[n][c][y][x], NCHW, fp16 (the dataset's storage format) or fp32.
 * Coefficient table of one axis of one image, at int32 offset *_off of `coef`: lo[S], len[S], k[S][*_taps] (k is 0 past
 * len).  Images may share tables.  A workgroup owns a band of output rows of one image: it runs the horizontal pass for
 * the source rows that band needs into an LDS tile of uint8 [rows][S][3], then the vertical pass out of LDS, the table
 * look-up and the stores of the three channel planes.  No atomics, no floating point, no branch on a pixel value. */
typedef struct {
  int64_t src_offset;     /* byte offset of pixel (0, 0) in the packed source buffer */
  int64_t pitch;          /* bytes from one source row to the next, >= 3 * W */
  int32_t H, W;           /* source size */
  int32_t oh, ow;         /* resized size (step 1); both >= S */
  int32_t top, left;      /* origin of the crop window in the resized image (step 3) */
  int32_t h_off, h_taps;  /* horizontal table (ow from W, columns left .. left + S) */
  int32_t v_off, v_taps;  /* vertical table (oh from H, rows top .. top + S) */
} vqa_pre_image_t;        /* 56 bytes */

/* Band height (output rows per workgroup, > 0) the kernel would use for this batch, or 0 when it does not cover it
 * (vqa_last_error says why): a descriptor or table that is out of range (any lo + len > n, len < 1, len > taps, a window
 * outside the resized image, a resized side < S), or a scale so large that the source rows of ONE output row do not fit
 * the LDS tile.  Pure host code: images and coef are HOST pointers, no HIP call is made.  src_offset / pitch are not read. */
int vqa_preprocess_supported(const vqa_pre_image_t* images, const int32_t* coef, int64_t coef_len, int N, int S);

/* images_host / coef_host: the HOST copies of the DEVICE arrays images_dev / coef_dev (the same bytes): every check --
 * null pointers, N < 0, S < 1, what vqa_preprocess_supported checks, and every image's bytes inside [0, src_bytes) --
 * runs on them before any launch, so the kernel never reads outside src, coef or its LDS tile.  N == 0 returns VQA_OK
 * without a launch.  src, lut and out are device pointers; lut is [3][256] fp16 (out_is_f32: fp32), out [N][3][S][S]. */
int vqa_preprocess_images(const uint8_t* src, int64_t src_bytes, const vqa_pre_image_t* images_host, const int32_t* coef_host,
                          int64_t coef_len, const vqa_pre_image_t* images_dev, const int32_t* coef_dev, int N, int S,
                          const void* lut, int out_is_f32, void* out, vqa_stream_t stream);

/* ---- bf16 path (BASELINE configs[3]: bf16 MFMA conv / FC, fp32 accumulate, fp32 LSTM) -------------------
 * Opt-in second instantiation of the engine on v_mfma_f32_32x32x16_bf16.  Parameters, Adam state, the LSTM and
 * every reduction stay fp32; bf16 tensors are raw uint16 buffers (IEEE bfloat16, round to nearest even).
 * The fp32 entry points above remain the parity path. */
/* y = bf16(x) / y = float(x) element-wise; y[c][r] = bf16(x[r][c]) (a weight's bf16 copy in the other orientation) */
int vqa_f32_to_bf16(const float* x, void* y_bf16, int64_t n, vqa_stream_t stream);
int vqa_bf16_to_f32(const void* x_bf16, float* y, int64_t n, vqa_stream_t stream);
int vqa_f32_to_bf16_transpose(const float* x, void* y_bf16, int rows, int cols, vqa_stream_t stream);
/* y = bf16(x * keep(seed, i) / (1-p)): nn.Dropout fused with the bf16 copy (attention.drop on v, model.py:185) */
int vqa_dropout_to_bf16(const float* x, void* y_bf16, int64_t n, float p, uint64_t seed, vqa_stream_t stream);
/* vqa_gemm with bf16 A and B (same layouts / trans flags; leading dimensions in ELEMENTS, multiples of 8; K % 8 == 0;
 * a reduction-major operand needs its row length % 8 == 0), fp32 accumulation, the same fused epilogue; C is fp32,
 * or bf16 when c_is_bf16 (then no accumulate).  bias / rowgroup / aux stay fp32. */
int64_t vqa_gemm_bf16_workspace_bytes(int M, int N, int K);
int vqa_gemm_bf16(const void* A, int64_t lda, int transA, const void* B, int64_t ldb, int transB, void* C,
                  int64_t ldc, int c_is_bf16, int M, int N, int K, const float* bias1, const float* bias2,
                  const float* rowgroup, int64_t rg_ld, int rg_div, int rg_op, int relu, int accumulate,
                  float* aux, float* workspace, int64_t workspace_bytes, int tag, vqa_stream_t stream);

/* The plan the three entry points above run for a shape, as their launchers compute it under the VQA_* knobs in force; no HIP
 * call is made.  engine: 0 vqa_gemm, 1 vqa_gemm_x3, 2 vqa_gemm_bf16.  workspace_bytes: what the caller would pass (it only
 * decides whether vqa_gemm_bf16 admits its 128 x 256 plan).  out[0..9] = BM, BN, tiles_m, tiles_n, nk (K-steps), splits,
 * ks_per_split, order (0: tiles row-major, 1: column-major), persistent, wide; n_out >= 10. */
int vqa_gemm_plan(int engine, int M, int N, int K, int transA, int transB, int64_t workspace_bytes, int32_t* out, int n_out);

/* Tall bf16 GEMM with a short reduction (csrc/gemm_tall_bf16.hip): C[M][N] = act(A[M][K] . W[N][K]^T (+|*) rowgroup), bf16
 * result -- the v_conv forward of the bf16 path (models/model.py:173,187-193: M = B * positions, N = mid, K = image
 * features).  Persistent 256 x 128 tiles (128 x 128 under VQA_TALL_BM=128, a knob that vqa_reload_knobs re-reads), stages
 * prefetched through registers across tile boundaries, 16-byte stores.  Operands as vqa_gemm_bf16 with transA = 0,
 * transB = 1; rowgroup (optional) [ceil(M / rg_div)][N] fp32, rg_op 0 = add, 1 = multiply.  The row-group table is read 16
 * bytes at a time: with a rowgroup, rg_ld >= N, rg_ld % 4 == 0 and a 16-byte aligned rowgroup pointer are required
 * (VQA_ERR_INVALID otherwise).
 * vqa_gemm_tall_bf16_plan: the launch geometry for a shape (N % 128 == 0, K % 64 == 0) under the knob in force, as the launcher
 * computes it (it calls this query); no HIP call is made.  out[0..4] = tile height, tiles_m, tiles_n, grid (workgroups), nk
 * (k-stages of 64); n_out >= 5. */
int vqa_gemm_tall_bf16_supported(int M, int N, int K, int rg_div, int has_rowgroup);
int vqa_gemm_tall_bf16_plan(int M, int N, int K, int32_t* out, int n_out);
int vqa_gemm_tall_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int M, int N, int K,
                       const float* rowgroup, int64_t rg_ld, int rg_div, int rg_op, int relu, int tag, vqa_stream_t stream);

/* Convolution blocks of the bf16 path (models/model.py:80-82 and their autograd): activations NHWC bf16, weights
 * re-packed per step to bf16 as wfT [Co][9*CiP] and wdT [CiP][9*Co] (K index = (tap, channel)), arg-max bytes and
 * semantics as in the fp32 entry points, fp32 accumulation, fp32 weight / bias gradients.
 *   forward: CiP % 64 == 0; pooled is bf16, or fp32 when pooled_is_bf16 == 0 (the last block feeds the fp32 L2 norm);
 *   dgrad:   Co % 64 == 0; dx is bf16, or fp32 when dx_is_bf16 == 0;
 *   wgrad:   CiP, Co multiples of 8; both operands reach the MFMAs through ds_read_b64_tr_b16 (reduction-major). */
int vqa_conv_pack_weights_bf16(const float* w, void* wfT, void* wdT /* may be NULL */, int Co, int Ci, int CiP,
                               vqa_stream_t stream);
int vqa_conv3x3_relu_pool_fwd_bf16(const void* x, const void* wfT, const float* bias, void* pooled,
                                   int pooled_is_bf16, uint8_t* argmax, int B, int H, int W, int CiP, int Co,
                                   int stride, int tag, vqa_stream_t stream);
int vqa_conv3x3_dgrad_bf16(const void* dpooled, const uint8_t* argmax, const void* wdT, void* dx, int dx_is_bf16,
                           int B, int H, int W, int CiP, int Co, int stride, int tag, vqa_stream_t stream);
int64_t vqa_conv3x3_wgrad_bf16_workspace_bytes(int B, int H, int W, int CiP, int Co, int stride);
int vqa_conv3x3_wgrad_bf16(const void* x, const void* dpooled, const uint8_t* argmax, float* dw, float* dbias,
                           int B, int H, int W, int CiP, int Ci, int Co, int stride, float* workspace,
                           int64_t workspace_bytes, int tag, vqa_stream_t stream);

/* Patch convolutions of the bf16 path (csrc/conv_patch_bf16.hip; models/model.py:80-82 and their autograd), 3x3, stride 1:
 * a persistent workgroup keeps an input patch in LDS and takes the nine taps as shifted fragment reads of it, so every
 * input pixel is fetched once per workgroup instead of once per tap.  Same results contract as the vqa_conv3x3_*_bf16 entry
 * points (bf16 operands, fp32 accumulation, arg-max codes 0-3 / 4 = dead window); what differs:
 *   - every tensor a patch is cut from is channel-blocked "C16": [B][C/16][H][W][16] -- the activations between the blocks
 *     (bf16), the pooled gradients (bf16) AND the arg-max bytes;
 *   - the weights are packed per step into fragment-ordered images (vqa_pconv_pack_weights; wf_img for forward, wd_img =
 *     flipped + transposed for backward-data, vqa_pconv_weights_bytes each);
 *   - forward patches are copied by buffer_load ... lds; backward patches (the pre-pool gradient: dP where the arg-max byte
 *     names the pixel, zero elsewhere and on the border) are ROUTED in the kernel from dP + arg-max -- the pre-pool
 *     gradient, four times the pooled one, never exists in HBM.
 * Shapes: Ci % 16 == 0, Co % 64 == 0 (forward); additionally Ci % 64 == 0 for backward-data (vqa_pconv_supported). */
int vqa_pconv_supported(int H, int W, int Ci, int Co, int stride);
int64_t vqa_pconv_weights_bytes(int Ci, int Co);
int vqa_pconv_pack_weights(const float* w /* [Co][Ci][3][3] */, void* wf_img /* may be NULL */, void* wd_img /* may be NULL */,
                           int Co, int Ci, vqa_stream_t stream);
/* x C16 [B][Ci/16][H][W][16] -> pooled (bf16 C16 [B][Co/16][Hp][Wp][16] or fp32 NHWC [B][Hp][Wp][Co]) and arg-max bytes
 * (always C16 [B][Co/16][Hp][Wp][16]) */
int vqa_pconv_fwd(const void* x, const void* wf_img, const float* bias, void* pooled, int pooled_is_bf16, uint8_t* argmax,
                  int B, int H, int W, int Ci, int Co, int tag, vqa_stream_t stream);
/* dX of the block whose INPUT map is H x W x Ci, from the pooled gradient and arg-max bytes (both C16, [B][Co/16][Hp][Wp][16]).
 * dx_mode: 0 fp32 NHWC, 1 bf16 NHWC (feeds vqa_conv0_wgrad_bf16), 2 bf16 C16 (the pooled gradient of the block below) */
int vqa_pconv_dgrad(const void* dpooled, const uint8_t* argmax, const void* wd_img, void* dx, int dx_mode, int B, int H, int W,
                    int Ci, int Co, int tag, vqa_stream_t stream);
/* weight + bias gradient: dw [Co][Ci][3][3], dbias [Co] fp32.  A workgroup holds a whole [9 taps x 64 ci] x [128 co] block of
 * dW in its accumulators and streams 4 x 32-pixel tiles of x (C16; LDS patch, nine shifted transpose-reads) and of the routed
 * pre-pool gradient through LDS; one fp32 slab per workgroup, summed by a reduce kernel (deterministic).  Ci % 64 == 0,
 * Co % 128 == 0, and (Ci / 64) * (Co / 128) in {1, 2, 4, 8}; dbias is the masked sum of dpooled (arg-max != 4), summed by the
 * same kernel as the pieces of dpooled pass through it. */
int vqa_pconv_wgrad_supported(int H, int W, int Ci, int Co);
int64_t vqa_pconv_wgrad_workspace_bytes(int B, int H, int W, int Ci, int Co);
int vqa_pconv_wgrad(const void* x, const void* dpooled, const uint8_t* argmax, float* dw, float* dbias, int B, int H, int W,
                    int Ci, int Co, float* workspace, int64_t workspace_bytes, int tag, vqa_stream_t stream);

/* fp32 patch backward-data (csrc/conv_patch_f32.hip; the autograd of models/model.py:80-82 on the fp32 headline path): the same
 * dX as vqa_conv3x3_dgrad (stride 1) up to fp32 summation order, from the same operands (dpooled fp32 NHWC, argmax NHWC) --
 * a persistent workgroup builds the pre-pool gradient of an 8-channel slice in LDS once (routed from dpooled + argmax) and
 * takes the nine taps as shifted fragment reads over a FLATTENED segment of the padded map (no 2-D edge waste at 111- and
 * 54-pixel maps), exact fp32 MFMA.  wd_img = vqa_pconvf_pack_weights(w) (flipped, transposed, fragment order),
 * vqa_pconvf_weights_bytes.  Ci % 64 == 0, Co % 8 == 0, W <= 256 (vqa_pconvf_supported). */
int vqa_pconvf_supported(int H, int W, int Ci, int Co, int stride);
int64_t vqa_pconvf_weights_bytes(int Ci, int Co);
int vqa_pconvf_pack_weights(const float* w /* [Co][Ci][3][3] */, float* wd_img, int Co, int Ci, vqa_stream_t stream);
int vqa_pconvf_dgrad(const float* dpooled, const uint8_t* argmax, const float* wd_img, float* dx, int B, int H, int W, int Ci,
                     int Co, int tag, vqa_stream_t stream);

/* ---- fp32 on the bf16 matrix cores ("fp32x3": csrc/x3_core.hpp) -------------------------------
 * The same fp32 tensors, layouts and results contract as the fp32 entry points above; inside the K loop every
 * fp32 operand element is split exactly into three bf16 terms (8 + 8 + 8 significand bits) and a product is
 * accumulated in fp32 from its six partial products of weight >= 2^-16 (the dropped ones are below 2^-24 of the
 * product, less than one fp32 rounding): six v_mfma_f32_32x32x16_bf16 instead of eight v_mfma_f32_32x32x2_f32 per
 * 32x32x16 block, 2.67x the fp32 MFMA rate at fp32 accuracy.  Arguments as vqa_conv3x3_relu_pool_fwd /
 * vqa_conv3x3_dgrad / vqa_conv3x3_wgrad (models/model.py:72-84), except that the packed weights wf / wd are handed over
 * already split: three bf16 planes (hi, mid, lo), each in the layout of vqa_conv_pack_weights and one after the other
 * (vqa_x3_split of the fp32 packing, once per step); shapes: CiP, Co multiples of 32 and a conv output
 * row of at least 32 pixels (vqa_conv3x3_x3_supported), other layers keep the fp32 MFMA entry points. */
int vqa_conv3x3_x3_supported(int H, int W, int CiP, int Co, int stride);
/* the operand split of those kernels on its own (the packed weights, once per step; tests): x[n] -> three planes of n
 * bf16, x == hi + mid + lo exactly */
int vqa_x3_split(const float* x, void* hi, void* mid, void* lo, int64_t n /* multiple of 4 */, vqa_stream_t stream);
/* x3-packed activations: a tensor [pixels][C] (C % 4 == 0) split once per tensor instead of by every workgroup that
 * reads it: every four consecutive channels are 24 bytes hi[4] mid[4] lo[4] bf16 (6 bytes per element, same order).
 * The forward and wgrad entry points take their input x either as fp32 (x_packed = 0) or in this form (1). */
int vqa_x3_pack(const float* x, void* out /* 6 bytes per element */, int64_t n /* multiple of 4 */, vqa_stream_t stream);
int vqa_conv3x3_relu_pool_fwd_x3(const void* x, int x_packed, const void* wf_planes, const float* bias, void* pooled,
                                 int pooled_packed /* 1: the output is written x3-packed, for the next block */,
                                 uint8_t* argmax, int B, int H, int W, int CiP, int Co, int stride, int tag,
                                 vqa_stream_t stream);
/* dpooled: fp32 (dp_packed = 0) or x3-packed (1): the arg-max routing then is a mask on the packed halves */
int vqa_conv3x3_dgrad_x3(const void* dpooled, int dp_packed, const uint8_t* argmax, const void* wd_planes, float* dx, int B,
                         int H, int W, int CiP, int Co, int stride, int tag, vqa_stream_t stream);
int64_t vqa_conv3x3_wgrad_x3_workspace_bytes(int B, int H, int W, int CiP, int Co, int stride);
/* One pass over a pooled gradient [windows][Co] for its two needs in the fp32x3 backward: the x3-packed copy (read by
 * dgrad and wgrad) and the bias gradient (sum over the windows whose ReLU was alive, arg-max byte != 4). */
int64_t vqa_x3_pack_pooled_grad_workspace_bytes(int Co);
int vqa_x3_pack_pooled_grad(const float* dpooled, const uint8_t* argmax, void* packed, float* dbias, int64_t windows, int Co,
                            float* workspace, int64_t workspace_bytes, vqa_stream_t stream);
/* dpooled (fp32): the bias gradient is summed from it unless dbias is NULL (the caller has it from
 * vqa_x3_pack_pooled_grad); dpooled_packed (optional): the same gradient x3-packed, read by the contraction instead */
int vqa_conv3x3_wgrad_x3(const void* x, int x_packed, const float* dpooled, const void* dpooled_packed,
                         const uint8_t* argmax, float* dw, float* dbias, int B, int H, int W, int CiP, int Ci, int Co,
                         int stride, float* workspace, int64_t workspace_bytes, int tag, vqa_stream_t stream);

/* vqa_gemm on the split kernels: the same arguments and results contract (large contractions: the attention stage's
 * v_conv forward / dW / dX); 192 x 128 tiles, split-K slabs in `workspace` when the output has few tiles. */
int64_t vqa_gemm_x3_workspace_bytes(int M, int N, int K);
int vqa_gemm_x3(const float* A, int64_t lda, int transA, const float* B, int64_t ldb, int transB, float* C, int64_t ldc,
                int M, int N, int K, const float* bias1, const float* bias2, const float* rowgroup, int64_t rg_ld,
                int rg_div, int rg_op, int relu, int accumulate, float* aux, float* workspace, int64_t workspace_bytes,
                int tag, vqa_stream_t stream);

/* ---- optimiser: torch.optim.Adam defaults over one flat buffer (train.py:55,80) ------------- */
int vqa_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
             float beta1, float beta2, float eps, int step, float grad_scale, vqa_stream_t stream);

/* ---- optimiser with parameter groups: Adam / AdamW over a table of segments of the flat buffer ----
 * One launch updates every listed range [begin, end) with that segment's own step number (bias correction), learning
 * rate, betas, eps and weight decay; elements outside every segment are neither read nor written.  `segs` is a HOST
 * array: it travels to the kernel by value in the launch arguments (no allocation, no upload, no sync).
 *   weight_decay == 0: the arithmetic of vqa_adam expression for expression -- the segment holds the bits vqa_adam
 *     gives on that slice with that lr and step; no decay term is evaluated (0 * p would change signed zeros and
 *     non-finite values);
 *   weight_decay > 0, decoupled == 0 (torch.optim.Adam): the gradient is grad * grad_scale + weight_decay * param;
 *   weight_decay > 0, decoupled == 1 (torch.optim.AdamW): param is first multiplied by 1 - lr * weight_decay.
 * VQA_ERR_INVALID, before any HIP call, for: a null or not 16-byte aligned pointer, n < 1, n_segs outside
 * 1..VQA_ADAM_MAX_SEGMENTS, a segment with begin or end no multiple of 4, begin < 0, begin >= end or end > n, segments that are
 * not sorted and disjoint (begin below the previous end), step < 1, weight_decay < 0 (or NaN), decoupled outside 0/1.
 * The grid is capped at VQA_ADAM_SEGMENTS_MAX_BLOCKS workgroups of 256 lanes, one float4 per lane: a longer walk
 * (more than VQA_ADAM_SEGMENTS_MAX_BLOCKS * 1024 floats from the first begin to the last end) strides. */
#define VQA_ADAM_MAX_SEGMENTS 64
#define VQA_ADAM_SEGMENTS_MAX_BLOCKS 2048
typedef struct {
  int64_t begin, end;   /* [begin, end) in elements of the flat buffer; both multiples of 4 */
  float lr, beta1, beta2, eps, weight_decay;
  int step;             /* >= 1: this segment's own step number (bias correction) */
  int decoupled;        /* 0: L2 as torch.optim.Adam; 1: torch.optim.AdamW */
} vqa_adam_segment;
int vqa_adam_segments(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                      const vqa_adam_segment* segs /* HOST array */, int n_segs, float grad_scale,
                      vqa_stream_t stream);

/* ---- the plan of the fp32x3 conv entry points ------------------------------------------------
 * What vqa_conv3x3_relu_pool_fwd_x3 (pass 0), vqa_conv3x3_dgrad_x3 (pass 1) and vqa_conv3x3_wgrad_x3 (pass 2) run for a layer
 * and batch under the VQA_* knobs in force, from the host functions their launchers call; no HIP call is made.  A batch is
 * walked in launches of `chunk` images; the tiles are those of the first launch (min(B, chunk) images).
 * out[0..10] = BM, BN, waves per workgroup, tiles_m, tiles_n, persistent (0: one workgroup per tile, 1: 256 workgroups walk the
 * tiles; always 0 for pass 2), chunk, launches, nk (K-steps of 32), splits, ks_per_split (pass 0 and 1: 1 and nk); n_out >= 11.
 * VQA_ERR_INVALID for a pass outside 0..2, a null out, a short n_out and every layer vqa_conv3x3_x3_supported refuses. */
int vqa_conv3x3_x3_plan(int pass, int B, int H, int W, int CiP, int Co, int stride, int32_t* out, int n_out);

/* ---- float16 image-feature caches ---------------------------------------------------------------
 * The cached image features (vn, and v' = v_conv(vn)) may be stored as IEEE half: the fp32 tensor rounded ONCE, to nearest
 * even, overflow to +-inf, NaN kept, subnormals kept (vqa_float_to_half).  Each reader below is the device code of the entry
 * point it is named after with the cache operand's load widened on the fly (exact), so it returns, bit for bit, what the fp32
 * entry point returns on an fp32 tensor holding the same values; every other operand is fp32 and checked as there.
 * A quad of halves is one 8-byte load, so the half operand needs 8-byte alignment where the fp32 form needs 16.
 *   vqa_float_to_half: y[i] = half(x[i]); x and y 16-byte aligned; n == 0 returns VQA_OK without a launch.
 *   vqa_gather_rows_drop_f16: src is a half bank [M][row_len], dst fp32.  The quad path (8-byte loads, 16-byte stores) needs
 *     row_len % 4 == 0, src 8-byte and dst 16-byte aligned; anything else takes the scalar path, same bits.
 *   vqa_att_apply_gather_fwd_f16: vn is half [N][P][C].  C % 4 != 0 or a vn that is not 8-byte aligned runs the scalar kernel.
 *   vqa_att_apply_gather_dscore_f16: vn is half; C % 4 == 0, dout_ld % 4 == 0, dout 16-byte and vn 8-byte aligned
 *     (VQA_ERR_INVALID otherwise, as the fp32 form refuses what it cannot read as quads).
 *   vqa_att_score_grouped_fwd_f16 / vqa_att_score_grouped_pairs_fwd_f16: v' is half [N*P][mid], 8-byte aligned; it is widened
 *     while its tile is staged in LDS (the tile stays fp32).  Inference forms only: training recomputes v' in fp32. */
int vqa_float_to_half(const float* x, void* y_f16, int64_t n, vqa_stream_t stream);
int vqa_gather_rows_drop_f16(const void* src_f16, const int32_t* rows, float* dst, int n, int M, int64_t row_len, float p,
                             uint64_t seed, vqa_stream_t stream);
int vqa_att_apply_gather_fwd_f16(const float* score, const void* vn_f16, const int32_t* img, float* probs, float* out,
                                 int64_t out_ld, int N, int B, int P, int C, int G, vqa_stream_t stream);
int vqa_att_apply_gather_dscore_f16(const float* dout, int64_t dout_ld, const float* probs, const void* vn_f16,
                                    const int32_t* img, float* dscore, float* dscore_rowsum, int N, int B, int P, int C, int G,
                                    vqa_stream_t stream);
int vqa_att_score_grouped_fwd_f16(const void* vprime_f16, const float* qp, const float* wx, int wx_ld, const float* bx,
                                  const int32_t* order, const int32_t* offsets, float* score, int N, int B, int P, int mid, int G,
                                  int mode, vqa_stream_t stream);
int vqa_att_score_grouped_pairs_fwd_f16(const void* vprime_f16, const float* qp, const int32_t* qrow, const float* wx, int wx_ld,
                                        const float* bx, const int32_t* order, const int32_t* offsets, float* score, int N, int B,
                                        int M, int P, int mid, int G, int mode, vqa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VQA_HIP_H */
