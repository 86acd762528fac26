/* mega_hip.h -- C ABI of libmega_hip.so: the MI355X (gfx950) native kernels behind MEGA's
 * per-key-frame inference hot path.
 *
 * Boundary rules
 *   - extern "C", plain device pointers + sizes, no torch / ATen types.
 *   - every entry point returns int: 0 = MEGA_OK, 1 = bad argument, 2 = launch failure,
 *     3 = workspace too small, 4 = a kernel's loop bound was exceeded (mega_seq_nms, mega_link_tracks).  Nothing is
 *     allocated inside: the caller owns outputs and workspaces.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).  All work is
 *     enqueued on that stream; no call synchronises the device or copies to the host, except mega_seq_nms and
 *     mega_link_tracks, which read their status word back.
 *   - mega_jpeg_probe and mega_jpeg_entropy_decode are the exception to both rules above: they take HOST pointers and no
 *     stream, run entirely on the calling thread and touch no device (lengths are long long, everything else a pointer).
 *   - dtype codes: MEGA_F32 = 0 (exact-f32 MFMA path, parity mode), MEGA_BF16 = 1, MEGA_F16 = 2 (IEEE half: the same
 *     kernels instantiated for _Float16 operands -- the bf16 MFMA rate and bytes with 11 significant bits instead of 8,
 *     values bounded by 65 504; accumulation is f32 in every mode).  Wherever an entry point takes a dtype code, MEGA_F16
 *     is accepted where MEGA_BF16 is, unless its comment says otherwise (the split-precision plane kernels are bf16 only).
 *   - activations are NHWC; GEMM weights are OHWI ([Cout][R][S][Cin]) so both operands are K-contiguous.
 *   - this header is the ONE declaration of the ABI.  The kernels' sources include it, so the compiler checks every
 *     definition against its prototype, and the Python binding parses it (comments stripped) into its ctypes signatures
 *     and structures.  The parser's grammar is deliberately tiny; keep every declaration inside it:
 *       prototype   `RET mega_name(PARAMS);` -- RET is int, size_t, void or const char*; PARAMS is `void` or a comma list
 *                   of named parameters, each int, float, long long, size_t or a pointer (anything with a `*`).
 *       descriptor  `typedef struct { FIELDS } mega_name;` -- semicolon-ended fields of the parameter types, several
 *                   names of one type separated by commas (`int ldq, ldk;`).
 *     Anything else (a double or unsigned parameter, an array field, a struct by value) makes the binding raise, naming
 *     the line.
 *
 * Each prototype cites the reference interface it replaces (paths relative to the reference tree
 * Scalsol/mega.pytorch).
 */
#ifndef MEGA_HIP_H
#define MEGA_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MEGA_F32 0
#define MEGA_BF16 1
#define MEGA_F16 2
#define MEGA_F8 3     /* OCP e4m3fn codes, one byte each: mega_conv2d_nhwc_f8 only */

#define MEGA_OK 0
#define MEGA_ERR_ARG 1
#define MEGA_ERR_LAUNCH 2
#define MEGA_ERR_WS 3
#define MEGA_ERR_LIMIT 4   /* a kernel's loop bound was exceeded (mega_seq_nms, mega_link_tracks) */

/* Conv2d (+ FrozenBatchNorm2d scale/bias) (+ residual add) (+ ReLU), implicit GEMM on MFMA.
 * Replaces torch Conv2d->cuDNN + the unfused FrozenBatchNorm2d / relu_ / += of
 * mega_core/modeling/backbone/resnet.py:324-344 (Bottleneck.forward), :155-204 (ResNetHead),
 * mega_core/layers/batch_norm.py:19-31, modeling/rpn/rpn.py:99-106 (RPNHead), and every nn.Linear
 * of the box head (H = W = R = S = 1, N = rows): roi_box_feature_extractors.py:894,:907,:826,
 * roi_box_predictors.py:50-57.
 *   in  [N][H][W][Cin]      (in_dtype)        w [Cout][R][S][Cin] (in_dtype)
 *   out [N*Ho*Wo][ldo]      (out_dtype)       y = act(acc*scale[c] + bias[c] (+ residual[m][c]))
 *   relu: 0 = identity, 1 = ReLU, 2 = LeakyReLU(0.1) (FlowNetS)
 *   scale / bias: f32 [Cout] or NULL (1 / 0); residual [M][ldr] in_dtype or NULL; ldo/ldr <= 0 -> Cout.
 *   Cin must be a multiple of 64 (bf16) / 32 (f32).  out_dtype may be MEGA_F32 with bf16 inputs. */
int mega_conv2d_nhwc(const void* in, const void* w, const float* scale, const float* bias, const void* residual,
                     void* out, int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dil,
                     int relu, int ldo, int ldr, int in_dtype, int out_dtype, void* stream);
/* Which block tile (BM * 1000 + BN, i.e. which igemm_kernel<.., BM, BN> instantiation) mega_conv2d_nhwc launches for
 * a GEMM of M = N*Ho*Wo rows, Cout columns, K = R*S*Cin: lets a profiler attribute time to the kernel symbol
 * rocprofv3 reports.  No device work. */
int mega_conv2d_nhwc_tile(int M, int Cout, int K);
/* Same, for a given operand dtype (MEGA_F32 / MEGA_BF16): kind * 1000000 + BM * 1000 + BN with kind 0 =
 * igemm_kernel<.., BM, BN> (register-staged tiles) and kind 8 = igemm8_kernel (bf16 only: LDS-DMA staging, 8 waves,
 * BM x 256 tiles, BM = 256 or 192).  Every kernel accumulates an output element over K in the same order with the
 * same MFMA instruction, so the choice never changes a result bit. */
int mega_conv2d_nhwc_plan(int M, int Cout, int K, int in_dtype);
/* The shape-complete form: which kernel mega_conv2d_nhwc[_ws] really dispatches THIS layer to (same predicates as the
 * launch path: one function decides for both): kind 6 = conv3x3_c64_kernel (layer1's 3x3 64 -> 64 conv: 3x3, stride 1, pad 1,
 * 16-bit out, no residual, enough tiles), 7 = igemm8 streaming class (1x1, K <= 512), 8 = igemm8 matrix class, 0 = igemm_kernel.
 * -1: bad shape.  The split count is the one of mega_conv2d_nhwc_ws (a function of K alone).  (Kinds 1-4 were round 6's three
 * opt-in GEMM kernels: measured at or below igemm8, profiles/r06_streaming_class_experiments.txt, and removed.) */
int mega_conv2d_nhwc_plan_ex(int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dil, int ldo,
                             int has_residual, int in_dtype, int out_dtype);

/* mega_conv2d_nhwc with a caller-owned workspace of mega_conv2d_nhwc_workspace_bytes(M, Cout, K) bytes (M = N*Ho*Wo,
 * K = R*S*Cin; 0 for most layers).  With it, layers with K >= 32768 (the box head's first FC, K = 100352) run
 * split-K: three K ranges per output tile write f32 partial sums into the workspace and a second kernel adds them in a
 * fixed order and applies scale / bias / residual / activation.  The split depends on K only, never on M, so a
 * row's result does not depend on the batch it is computed in.  mega_conv2d_nhwc (no workspace) never splits. */
size_t mega_conv2d_nhwc_workspace_bytes(int M, int Cout, int K);
int mega_conv2d_nhwc_ws(const void* in, const void* w, const float* scale, const float* bias, const void* residual,
                        void* out, int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dil,
                        int relu, int ldo, int ldr, int in_dtype, int out_dtype, void* ws, size_t ws_bytes, void* stream);

/* mega_conv2d_nhwc for a 1x1 / stride 1 / unpadded conv whose residual is read at a pixel stride: output pixel (t, y, x) adds
 * pixel (res_stride y, res_stride x) of the NHWC tensor residual [N][res_H][res_W][ldr], i.e. residual[:, ::s, ::s, :] read in
 * place (a bottleneck's conv3 run at the even pixels only, the identity taken from the block's dense input).  dtype MEGA_BF16 /
 * MEGA_F16 = operands and output; Cin % 64 == 0, Cin <= 512, Cout % 256 == 0, (H - 1) res_stride < res_H, (W - 1) res_stride <
 * res_W.  Same bits as mega_conv2d_nhwc on the gathered residual. */
int mega_conv2d_nhwc_rs(const void* in, const void* w, const float* scale, const float* bias, const void* residual, void* out,
                        int N, int H, int W, int Cin, int Cout, int relu, int ldo, int ldr, int res_H, int res_W, int res_stride,
                        int dtype, void* stream);

/* ResNet stem: 7x7 stride-2 pad-3 conv (3->64) + FrozenBN + ReLU  (resnet.py:347-366 BaseStem.forward,
 * without the max-pool).  in: NCHW f32 [N][3][H][W]; w_tap64: [147][64] f32 with tap = (c*7+r)*7+s;
 * out: NHWC [N][Ho][Wo][64], Ho = (H-1)/2+1. */
int mega_stem_conv_bn_relu(const float* in, const float* w_tap64, const float* scale, const float* bias, void* out,
                           int N, int H, int W, int out_dtype, void* stream);
/* The same stem on the matrix cores (bf16 path): w_n176_bf16 = bf16 [64][176], row n = output channel, column
 * k = (c*7+r)*8+s for the 7 taps s of kernel row (c, r), zero for s = 7 and for the 8 pad columns; out: NHWC bf16.
 * Image pixels and weights are rounded to bf16, accumulation is f32. */
int mega_stem_conv_bn_relu_bf16(const float* in, const void* w_n176_bf16, const float* scale, const float* bias,
                                void* out, int N, int H, int W, void* stream);
/* The bf16 stem fed by the uint8 frames themselves, [N][H][W][3] RGB: the preprocessing of mega_preprocess_frames
 * (data/transforms/transforms.py:83-129: ToTensor, to_bgr255, Normalize with std 1) is applied on the patch load --
 * (float)byte - mean[c] for output channel c -- so the f32 image never exists in HBM.  Same bits as
 * mega_preprocess_frames followed by mega_stem_conv_bn_relu_bf16. */
int mega_stem_conv_bn_relu_bf16_u8(const void* frames_u8, const void* w_n176_bf16, const float* scale, const float* bias,
                                   void* out, int N, int H, int W, float mean0, float mean1, float mean2, int to_bgr,
                                   void* stream);

/* The whole stem of resnet.py:355-366 in one kernel (16-bit types): conv 7x7/2 + FrozenBN + ReLU + F.max_pool2d(3, 2, 1); `in` =
 * the preprocessed f32 NCHW image (u8 = 0) or the uint8 RGB frames [N][H][W][3] with the preprocessing on the patch load
 * (u8 = 1; mean / to_bgr as above); out NHWC bf16 [N][Hp][Wp][64], Hp = ((H - 1) / 2 + 1 - 1) / 2 + 1.  The stem's own
 * 64-channel map is never written.  Same bits as mega_stem_conv_bn_relu_bf16[_u8] + mega_maxpool3x3s2_nhwc. */
/* dtype = MEGA_BF16 or MEGA_F16 is the type of w_n176 and of `out`. */
int mega_stem_pool_dt(const void* in, int u8, const void* w_n176, const float* scale, const float* bias, void* out, int N,
                      int H, int W, float mean0, float mean1, float mean2, int to_bgr, int dtype, void* stream);
/* The pooled tile (rows x columns) that is one unit of mega_stem_pool_dt's work. */
void mega_stem_pool_tile(int* rows, int* cols);

/* F.max_pool2d(kernel 3, stride 2, padding 1) on NHWC (resnet.py:365). */
int mega_maxpool3x3s2_nhwc(const void* in, void* out, int N, int H, int W, int C, int dtype, void* stream);

/* nn.AvgPool2d(2, stride 2, ceil_mode=True) on NHWC (FlowNetS, mega_core/modeling/backbone/flownet.py:52,:56,:112). */
int mega_avgpool2x2_ceil_nhwc(const void* in, void* out, int N, int H, int W, int C, int dtype, void* stream);

/* ROIAlign forward.  Replaces mega_core._C.roi_align_forward (csrc/ROIAlign.h:11-25,
 * cuda/ROIAlign_cuda.cu:64-122, cpu/ROIAlign_cpu.cpp:113-219).  rois [K][5] f32 = (batch, x1, y1, x2, y2).
 *   in_nhwc : feat is [B][H][W][C] (1) or the reference's [B][C][H][W] (0)
 *   out_nhwc: out is bin-major [K][ph*pw][C] (1) or the reference's [K][C][ph][pw] (0) */
int mega_roi_align_fwd(const void* feat, const float* rois, void* out, int K, int C, int H, int W,
                       float spatial_scale, int pooled_h, int pooled_w, int sampling_ratio, int in_nhwc,
                       int out_nhwc, int dtype, int out_dtype, void* stream);

/* Greedy NMS.  Replaces mega_core._C.nms (csrc/nms.h:10-28): unsorted dets [n][4] + scores [n] ->
 * kept ORIGINAL indices, ascending, int64 (cuda/nms.cu:127-130, cpu/nms_cpu.cpp:64); *keep_cnt is a device int.
 * strict_gt = 1: suppress when IoU > thr (cuda/nms.cu:60); 0: IoU >= thr (cpu/nms_cpu.cpp:60).  n <= 8192. */
size_t mega_nms_full_workspace_bytes(int n);
int mega_nms(const float* dets, const float* scores, int n, float thr, int strict_gt, long long* keep_out,
             int* keep_cnt, void* ws, size_t ws_bytes, void* stream);

/* Batched NMS over P independent, already score-sorted problems (device-side counts, no host sync).
 *   boxes [P][nmax][4]; counts [P]; valid [P][nmax] u8 or NULL; order [P][nmax] or NULL
 *   keep_pos [P][max_keep] positions in sorted order (ascending); keep_cnt [P]
 *   flags [P][nmax] (pre-zeroed) or NULL: flags[order[pos]] = 1 for every kept box. */
size_t mega_nms_workspace_bytes(int P, int nmax);
int mega_nms_sorted(const float* boxes, const int* counts, const unsigned char* valid, const int* order, int P,
                    int nmax, float thr, int strict_gt, int max_keep, int* keep_pos, int* keep_cnt,
                    unsigned char* flags, void* ws, size_t ws_bytes, void* stream);

/* RPN proposal selection for B frames in one call.  Replaces RPNPostProcessor.forward_for_single_feature_map
 * (modeling/rpn/inference.py:76-123) incl. AnchorGenerator.grid_anchors (rpn/anchor_generator.py:73-95),
 * BoxCoder.decode (box_coder.py:52-95), clip_to_image (structures/bounding_box.py:214-219),
 * remove_small_boxes + boxlist_nms (structures/boxlist_ops.py:9-50).
 *   rpn_out [B][Hf*Wf][ldc] f32: channel a = objectness logit of anchor a, channel A + 4a + j = delta j
 *   outputs: proposals [B][post_nms_top_n][4], prop_scores [B][post_nms_top_n], prop_cnt [B] (device) */
size_t mega_rpn_select_workspace_bytes(int B, int pre_nms_top_n);
/* prop_index [B][post_nms_top_n] (NULL allowed): the flat anchor index (y * Wf + x) * A + a of every
 * kept proposal (-1 in unused rows) = the reference's index into permute_and_flatten's (N, H*W*A) order
 * (rpn/utils.py:10-14, rpn/inference.py:93-104) after NMS: what "bit-exact proposal indices" is checked on. */
int mega_rpn_select_idx(const float* rpn_out, const float* cell_anchors, int B, int Hf, int Wf, int A, int ldc,
                        int anchor_stride, int pre_nms_top_n, int post_nms_top_n, float nms_thresh, int strict_gt,
                        float min_size, float im_w, float im_h, float* proposals, float* prop_scores, int* prop_cnt,
                        int* prop_index, void* ws, size_t ws_bytes, void* stream);

/* Box-head post-processor for one image.  Replaces PostProcessor.forward / filter_results
 * (modeling/roi_heads/box_head/inference.py:45-149): softmax, per-class decode with (wx,wy,ww,wh), clip,
 * score > score_thresh, per-class NMS, detections_per_img k-th value cut (>= kth, ties kept).
 *   logits [R][NC], deltas [R][NC*4], props [R][4], nprop device int or NULL (= R); R <= 1024
 *   outputs have capacity (NC-1)*R rows; out_cnt is a device int; probs_out [R][NC] optional. */
size_t mega_postprocess_workspace_bytes(int R, int NC);
int mega_postprocess(const float* logits, const float* deltas, const float* props, const int* nprop, int R, int NC,
                     float wx, float wy, float ww, float wh, float im_w, float im_h, float score_thresh,
                     float nms_thresh, int strict_gt, int max_det, float* out_boxes, float* out_scores,
                     long long* out_labels, int* out_cnt, float* probs_out, void* ws, size_t ws_bytes,
                     void* stream);

/* The same post-processor for B images of R rows each in one launch chain (the key frames of a step-batch: the
 * reference calls PostProcessor.forward once per key frame, tools/test_net.py -> engine/inference.py:23-46).
 *   logits [B][R][NC], deltas [B][R][NC*4], props [B][R][4], nprop device int[B] or NULL; outputs [B][(NC-1)*R]...,
 *   out_cnt device int[B].  Image b's results have the bits of mega_postprocess on image b alone (same kernels,
 *   the image is a grid dimension). */
size_t mega_postprocess_batched_workspace_bytes(int B, int R, int NC);
int mega_postprocess_batched(const float* logits, const float* deltas, const float* props, const int* nprop, int B,
                             int R, int NC, float wx, float wy, float ww, float wh, float im_w, float im_h,
                             float score_thresh, float nms_thresh, int strict_gt, int max_det, float* out_boxes,
                             float* out_scores, long long* out_labels, int* out_cnt, float* probs_out, void* ws,
                             size_t ws_bytes, void* stream);

/* The first phase of the post-processor alone: the candidates that the reference's PostProcessor returns when
 * TEST.BBOX_AUG is enabled (box_head/inference.py:79-86: prepare_boxlist + clip_to_image(remove_empty=False)),
 * without the background class and with the score threshold applied.  No workspace.
 *   cboxes [B][NC-1][R][4] (class j + 1, proposal row r), cscores [B][NC-1][R]: the softmax score, -1 when it is not
 *   > score_thresh or r >= nprop[b]. */
int mega_postprocess_candidates_batched(const float* logits, const float* deltas, const float* props, const int* nprop,
                                        int B, int R, int NC, float wx, float wy, float ww, float wh, float im_w,
                                        float im_h, float score_thresh, float* cboxes, float* cscores, void* stream);

/* Test-time box augmentation merge (engine/bbox_aug.py:53-66) for F frames x K views (K <= 16, K * R <= 8192, else
 * MEGA_ERR_LIMIT before any launch).  cboxes [K][F][NC-1][R][4] / cscores [K][F][NC-1][R] as the candidate entries
 * write them, view k's boxes in its own image of view_w[k] x view_h[k] (host int arrays [K]), view_flip[k] (host) = 1
 * if the view's frames were mirrored.  Each box is un-flipped (BoxList.transpose), scaled into view 0's image
 * (BoxList.resize), then filter_results runs on the (view, row)-ordered concatenation: the outputs are those of
 * mega_postprocess, per frame, with capacity (NC-1)*K*R rows: out_boxes [F][cap][4], out_scores [F][cap],
 * out_labels [F][cap] i64, out_cnt device int[F]. */
size_t mega_bbox_aug_merge_workspace_bytes(int F, int K, int R, int NC);
int mega_bbox_aug_merge(const float* cboxes, const float* cscores, int F, int K, int R, int NC, const int* view_w,
                        const int* view_h, const int* view_flip, float score_thresh, float nms_thresh, int strict_gt,
                        int max_det, float* out_boxes, float* out_scores, long long* out_labels, int* out_cnt, void* ws,
                        size_t ws_bytes, void* stream);

/* The same merge with another final filter: soft-NMS (TEST.SOFT_NMS) and / or box voting (TEST.BBOX_VOTE), as
 * mega/pytorch_amd/soft_nms.py defines them.  Inputs, view mapping, row order, outputs and limits are those of
 * mega_bbox_aug_merge (K <= 16, K * R <= 8192, else MEGA_ERR_LIMIT; MEGA_ERR_ARG, MEGA_ERR_WS: all before any launch,
 * the outputs untouched).  Per (frame, class), on the rows with score > score_thresh:
 *   soft_method 0  the greedy NMS of mega_bbox_aug_merge (nms_thresh, strict_gt);
 *               1  linear soft-NMS: repeatedly keep the highest score (ties: lowest row) with its current score and
 *                  multiply every remaining row's score by 1 - iou where iou > nms_thresh (>= with strict_gt = 0);
 *               2  gaussian: by expf(-(iou * iou) / sigma), every row;
 *                  a row whose score is no longer > score_thresh leaves unkept.  f32 throughout, +1-area IoU.
 *   vote 1         every kept box becomes sum(s_j * b_j) / sum(s_j) over the live rows j of its (frame, class) with
 *                  iou(kept, j) >= vote_thresh -- original boxes and scores, f64 sums, rounded once to f32; the kept
 *                  row always votes.  vote_scoring 0 ("ID"): the score stays; 1 ("AVG"): the f64 mean of the voters'
 *                  original scores, rounded to f32.
 * then the class-major compaction and the max_det k-th value cut on the final scores.  A NaN IoU neither decays nor
 * votes.  soft_method 0 with vote 0 is mega_bbox_aug_merge, bit for bit.  MEGA_ERR_ARG for soft_method outside 0..2,
 * sigma <= 0, vote / vote_scoring outside 0..1, vote_thresh outside (0, 1]. */
size_t mega_soft_merge_workspace_bytes(int F, int K, int R, int NC);
int mega_soft_merge(const float* cboxes, const float* cscores, int F, int K, int R, int NC, const int* view_w,
                    const int* view_h, const int* view_flip, float score_thresh, float nms_thresh, int strict_gt,
                    int soft_method, float sigma, int vote, float vote_thresh, int vote_scoring, int max_det,
                    float* out_boxes, float* out_scores, long long* out_labels, int* out_cnt, void* ws, size_t ws_bytes,
                    void* stream);

/* Position-embedding logits of the relation module: log(relu(Wg . pe(q,k) + bg) + 1e-6).
 * Replaces extract_position_matrix + extract_position_embedding + the Wgs 1x1 conv + relu + log
 * (roi_box_feature_extractors.py:147-176,:126-144,:593-597,:630) without materialising the
 * [64][Nq][Nk] embedding.  wg_t [64][16] (Wg transposed), bg [16], dim_mat [8] = 1000^(i/8);
 * out [16][Nq][ldp] f32, ldp >= Nk (attention wants ldp % 32 == 0).  precise != 0: libm-accurate sincosf
 * (f32 parity mode); 0: two-constant range reduction + hardware sin/cos (abs error ~1e-6). */
int mega_position_logits(const float* rois_q, const float* rois_k, const float* wg_t, const float* bg,
                         const float* dim_mat, float* out, int Nq, int Nk, int ldp, int precise, void* stream);

/* Relation-attention core (roi_box_feature_extractors.py:599-646): per head h (64-wide)
 *   out[q][h*64+j] = resid[q][h*64+j] + bias_v[h*64+j]
 *                    + sum_k softmax_k( scale * q[q][h,:] . k[k][h,:] + pos[h][q][k] ) * vt[h*64+j][k]
 * q already contains the learned u vector (folded into the Wq bias), vt is V projected by Wv and stored
 * key-contiguous ([groups*64][ldv], pad columns zero).  pos / resid / bias_v may be NULL. */
int mega_relation_attention(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldv,
                            const float* pos, int ldp, const void* resid, int ldr, const float* bias_v, void* out,
                            int ldo, int Nq, int Nk, int groups, float scale, int dtype, void* ws, size_t ws_bytes,
                            void* stream);
/* The key range of one call is split over mega_relation_attention_splits() block groups (flash-decoding style:
 * partial max / sum / output per split, merged by a second kernel) when ws holds at least
 * mega_relation_attention_workspace_bytes(); with ws == NULL the call runs unsplit. */
/* The 16-bit pair of the two calls above (mega_position_logits_tiled_dt, mega_relation_attention_tiled_pos_dt below) keeps the
 * logits in 16 bits and in the attention kernel's own tile order:
 * out16 / pos_tiled16 = [16][ceil(Nk/32)][Nq][32] bf16 (16 * ceil(Nk/32) * Nq * 64 bytes, 16-byte aligned), the
 * 32 keys of a tile stored as (h2, rq, e) with key = 8 rq + 4 h2 + e.  Half the bytes of the f32 form, written by the
 * matrix-core position kernel and read by the attention kernel in fully coalesced 2 KiB blocks one tile pair ahead. */
int mega_relation_attention_splits(int Nq, int Nk, int groups);
size_t mega_relation_attention_workspace_bytes(int Nq, int Nk, int groups);

/* Test-time frame transform on device: uint8 HWC RGB [N][H][W][3] -> f32 CHW [N][3][H][W],
 * ToTensor -> (BGR*255 if to_bgr) -> minus mean, std 1.  Replaces the CPU chain
 * mega_core/data/transforms/transforms.py:83-129 for frames already at the target size. */
int mega_preprocess_frames(const unsigned char* in, float* out, int N, int H, int W, float mean0, float mean1,
                           float mean2, int to_bgr, void* stream);

/* Test-time Resize on device: PIL / torchvision F.resize(BILINEAR) of uint8 HWC frames,
 * [N][Hi][Wi][3] -> [N][Ho][Wo][3], bit-identical to Pillow's 8-bit resampler (libImaging/Resample.c): horizontal
 * pass to uint8 (tmp [N][Hi][Wo][3], needed only when both dimensions change), then vertical.  bounds_* = int
 * [out][2] (first tap, tap count), coef_* = int [out][ksize] fixed-point (<<22) taps, both prepared on the host
 * (mega.pytorch_amd.feed.pil_bilinear_coeffs).  A pass whose size is unchanged is skipped, as in PIL.  Replaces
 * mega_core/data/transforms/transforms.py:27-66 (Resize.__call__ -> F.resize). */
int mega_resize_bilinear_u8(const unsigned char* in, unsigned char* out, unsigned char* tmp, int N, int Hi, int Wi,
                            int Ho, int Wo, const int* bounds_h, const int* coef_h, int ksize_h, const int* bounds_v,
                            const int* coef_v, int ksize_v, void* stream);
/* The same resize followed by Image.transpose(FLIP_LEFT_RIGHT) (TT.RandomHorizontalFlip(1.0) after T.Resize,
 * engine/bbox_aug.py:92-96), the mirror written by the last pass; hflip = 0 is mega_resize_bilinear_u8.  With no
 * resize at all and hflip = 1 the frames are mirrored.  out must not alias in. */
int mega_resize_bilinear_u8_flip(const unsigned char* in, unsigned char* out, unsigned char* tmp, int N, int Hi, int Wi,
                                 int Ho, int Wo, const int* bounds_h, const int* coef_h, int ksize_h,
                                 const int* bounds_v, const int* coef_v, int ksize_v, int hflip, void* stream);

/* FGFA flow-guided aggregation (BASELINE configs[4]): bilinear warp of T frames' [features | embeddings] by their
 * flow fields (F.grid_sample bilinear / border / align_corners=False), cosine-similarity weights of the embeddings
 * against the key frame's, softmax over frames, weighted feature sum -- one fused kernel.  Replaces
 * GeneralizedRCNNFGFA.get_grid / resample / compute_weight + the softmax / sum of _forward_test
 * (mega_core/modeling/detector/generalized_rcnn_fgfa.py:45-76,:201-211).
 *   feats [T][H][W][Cf+Ce] NHWC, flow [T][2][H][W] f32, out [H][W][Cf], weights_out [T][H][W] f32 or NULL.
 * Shape limits, shared by the four mega_fgfa_warp_aggregate* entry points (ve = 8 elements per 16-byte vector in bf16, 4 in
 * f32): Cf / ve <= 256 and 256 % (Cf / ve) == 0, T < 63, H * W * (Cf + Ce) < 2^31.  Any other shape returns MEGA_ERR_ARG
 * before any launch (until the one-pass kernel was removed, such a shape silently ran on that slower kernel). */
int mega_fgfa_warp_aggregate(const void* feats, const float* flow, void* out, float* weights_out, int T, int H,
                             int W, int Cf, int Ce, int key, int dtype, void* stream);
/* The same with the T maps and flow fields held in a ring of T slots (the window's deques of
 * generalized_rcnn_fgfa.py:166-176 without the per-step torch.cat of 21 x 3072-channel maps): order = 1 + T device ints,
 * order[0] = slot of the key frame, order[1 + t] = slot of window position t.  Frames are visited in window order, so the
 * result has the bits of the contiguous call; one hipGraph serves every step (only the ints change). */
int mega_fgfa_warp_aggregate_ring(const void* feats, const float* flow, void* out, float* weights_out, int T, int H,
                                  int W, int Cf, int Ce, const int* order, int dtype, void* stream);

/* FlowNetS input in one kernel (round 6): the T image pairs cat([cur, frame_t]) of generalized_rcnn_fgfa.py:196-198 (the
 * "/ 255" lives in the first conv's weights), average-pooled 2 x 2 with ceil_mode (backbone/flownet.py:52,:56), written as
 * the operand of flow_conv1 with its seven horizontal taps gathered into the channel dimension:
 *   out[t][3 + h][w][s * 8 + c] = pool(pair)[t][h][w - 3 + s][c]  (c < 6; zeros for c = 6, 7, channels 56..63, taps outside
 *   the row and the three rows above / below), dtype MEGA_BF16 / MEGA_F16, [T][ceil(H/2) + 6][ceil(W/2)][64]:
 * flow_conv1 (7 x 7, stride 2, pad 3, 6 -> 64) then IS a 7 x 1 conv, stride 2, pad 0, over 64 channels (K = 448 instead of
 * the 49 x 64 of a channel-padded operand).  ring: f32 [T][3][H][W]; cur: the key frame(s), or NULL = ring slot order[0]. */
int mega_fgfa_pair_taps(const float* ring, long long ring_stride, const float* cur, long long cur_stride, const int* order,
                        void* out, int T, int H, int W, int dtype, void* stream);

/* DFF feature propagation: out[H][W][C] = bilinear warp (same grid convention as above) of the
 * key frame's NHWC feature map by flow [2][H][W], times the per-element scale map [H][W][C].  Replaces
 * GeneralizedRCNNDFF.get_grid / resample and the scale multiply (detector/generalized_rcnn_dff.py:41-60,:132-135). */
int mega_dff_warp_scale(const void* feats, const float* flow, const void* scale, void* out, int H, int W, int C,
                        int dtype, void* stream);

/* Pool / key-set assembly of the batched relation aggregation: n block copies (rows x row_bytes bytes, independent
 * source / destination row strides) in one launch -- replaces the reference's per-key-frame torch.cat of its pools
 * (roi_box_feature_extractors.py:676,:687-688,:812-814; generalized_rcnn_mega.py:213-216).  segs = mega_copy_seg[n], host
 * memory; strides in bytes.  Destinations must not overlap; addresses / strides / row lengths 2-byte aligned at least.
 * Bit-exact data movement. */
typedef struct { const void* src; void* dst; long long src_stride, dst_stride; int rows, row_bytes; } mega_copy_seg;
int mega_copy_segments(const mega_copy_seg* segs, int n, void* stream);

/* The identity bottleneck of the backbone's full-resolution stage -- layer1 blocks 1, 2 of ResNet-50/101-C4
 * (backbone/resnet.py:324-344: 256 -> 64 (1x1) -> 64 (3x3, pad 1) -> 256 (1x1) channels, stride 1, FrozenBN as f32
 * scale / bias vectors (layers/batch_norm.py:19-31), residual = the block's input) -- in ONE persistent kernel:
 *   out = relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1 x))))))) + x),   x, out: NHWC bf16 [N][H][W][256],
 * w1 [64][256], w2 [64][3][3][64], w3 [256][64] bf16 (OHWI).  The 64-channel intermediates never leave the CU.  Same MFMA,
 * K order, roundings and epilogue arithmetic as the three mega_conv2d_nhwc launches it replaces: bit-identical.
 * dtype = MEGA_BF16 / MEGA_F16: the 16-bit type of x, every w and out (both fused bottlenecks). */
int mega_bottleneck64_fwd_dt(const void* x, const void* w1, const float* s1, const float* b1, const void* w2, const float* s2,
                             const float* b2, const void* w3, const float* s3, const float* b3, void* out, int N, int H, int W,
                             int dtype, void* stream);

/* mega_bottleneck64_fwd_dt at the even pixels only: out = y[:, ::2, ::2, :] as a contiguous [N][ceil(H/2)][ceil(W/2)][256]
 * tensor, for a block whose only reader is a stride-2 1x1 conv.  conv1 runs on every pixel (the 3x3 windows need it); conv2,
 * conv3, the residual and the stores on a quarter of them.  Bit-identical to the dense form at those pixels. */
int mega_bottleneck64_even_fwd_dt(const void* x, const void* w1, const float* s1, const float* b1, const void* w2, const float* s2,
                                  const float* b2, const void* w3, const float* s3, const float* b3, void* out, int N, int H, int W,
                                  int dtype, void* stream);

/* The stage's first block with the 1x1 downsample branch on the residual (layer1 block 0: 64 -> 64 -> 64 (3x3) -> 256,
 * backbone/resnet.py:266-276,:324-344), one persistent kernel:
 *   out = relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1 x))))))) + bnd(convd(x))),  x NHWC bf16 [N][H][W][64], out [N][H][W][256];
 * w1 [64][64], w2 [64][3][3][64], w3 / wd [256][64].  The identity branch is computed from the x patch already in LDS and
 * rounded to bf16 before the add (as the separate launch would): bit-identical to the four mega_conv2d_nhwc launches. */
int mega_bottleneck64_ds_fwd_dt(const void* x, const void* w1, const float* s1, const float* b1, const void* w2, const float* s2,
                                const float* b2, const void* w3, const float* s3, const float* b3, const void* wd, const float* sd,
                                const float* bd, void* out, int N, int H, int W, int dtype, void* stream);

/* dst [rows][3K] bf16 = [hi | lo | hi] of src [rows][K] f32 (hi = bf16(v), lo = bf16(v - hi); K % 8 == 0): the A operand
 * of a split-precision GEMM on the bf16 matrix cores against weight rows [Wh | Wh | Wl] -- v.W to ~2^-16.  Used for the
 * stage FCs of the aggregation head (roi_box_feature_extractors.py:826-827) when the activation stream is f32. */
int mega_split_f32_to_bf16x3(const float* src, void* dst_bf16, int rows, int K, void* stream);

/* ---- split-precision activation PLANES (round 5): the parity mode of the frame stage at bf16 matrix-core rates, and the
 * wide residual stream of the bf16 mode.  The reference computes these layers in fp32 (mega_core/config/defaults.py:541;
 * backbone/resnet.py:324-344 `out += identity`, rpn/rpn.py:99-106, roi_box_feature_extractors.py:894,:907).  An f32
 * activation x [M][C] lives in HBM as bf16 [M][2C] = [hi | lo], hi = bf16(x), lo = bf16(x - hi): x = hi + lo to ~2^-17. */

/* dst [rows][2K] bf16 = [hi | lo] of src [rows][K] f32 (K % 8 == 0, both 16-byte aligned). */
int mega_split_f32_to_planes_dt(const float* src, void* dst, int rows, int K, int dtype, void* stream);

/* mega_roi_align_fwd on f32 NHWC features with the pooled rows leaving as planes: out bf16 [K][2 PH PW C] = [hi | lo] of the
 * f32 row [PH PW C] (same term order as the f32 kernel, ROIAlign_cuda.cu:64-122).  C % 4 == 0. */
int mega_roi_align_fwd_planes_dt(const float* feat, const float* rois, void* out_planes, int K, int C, int H, int W,
                                 float spatial_scale, int pooled_h, int pooled_w, int sampling_ratio, int dtype, void* stream);

/* conv + FrozenBN (+ split residual) + activation on plane tensors, bf16 matrix cores, f32 accumulation (igemm8 SP kernels):
 *   in       bf16 [N][H][W][ldi]; the contraction runs over Cin channels per tap, SOURCE channel k < kwrap ? k : k - kwrap
 *            (kwrap = 0: no wrap).  Split precision: ldi = 2C, Cin = 3C, kwrap = 2C reads [hi | lo | hi]; with weights
 *            packed [Wh | Wh | Wl] per tap ([Cout][R][S][3C]) the contraction is x_hi.Wh + x_lo.Wh + x_hi.Wl = x.W to ~2^-16.
 *            bf16 compute on a wide residual stream: ldi = 2C, Cin = C, kwrap = 0, plain weights (only hi is read).
 *   residual split planes [M][ldr] (ldr >= 2 Cout; 0 = 2 Cout) or NULL: hi + lo is added in f32 before the activation
 *   out_mode 0: bf16 [M][ldo];  1: split planes [M][ldo] (ldo >= 2 Cout);  2: f32 [M][ldo]     (ldo 0 = the natural width)
 *   relu     0 none, 1 ReLU, 2 LeakyReLU(0.1)
 * Cin % 64 == 0, kwrap % 64 == 0, Cout % 8 == 0, every tensor below 2 GiB (MEGA_ERR_ARG otherwise).  ws / ws_bytes: the
 * split-K workspace of mega_conv2d_nhwc_workspace_bytes(M, Cout, R S Cin) (long-K layers: f32 output without residual). */
int mega_conv2d_nhwc_sp_dt(const void* in, int ldi, int kwrap, const void* w, const float* scale, const float* bias,
                           const void* residual, int ldr, void* out, int ldo, int out_mode, int N, int H, int W, int Cin,
                           int Cout, int R, int S, int stride, int pad, int dil, int relu, int dtype, void* ws, size_t ws_bytes,
                           void* stream);

/* Which SP kernel a mega_conv2d_nhwc_sp_dt launch of GEMM shape M x Cout x K (K = R S Cin, Cin the wrapped depth of one tap)
 * with taps = R S runs on: kind * 1000000 + rows * 1000 + 256, encoded as mega_conv2d_nhwc_plan_ex (kind 7 streaming class,
 * 8 matrix class; rows 192 or 256).  has_ws: the call passes a split-K workspace.  Computed by the function the launch itself
 * uses; launches nothing.  -1: not a launchable combination (bad sizes, a split-K launch that is not out_mode 2). */
int mega_conv2d_nhwc_sp_plan(int M, int Cout, int K, int taps, int out_mode, int has_ws);

/* The three plane entry points above take either 16-bit type (dtype = MEGA_BF16 / MEGA_F16: the type of the [hi | lo] pairs and of
 * the weights; the text above describes MEGA_BF16).  MEGA_F16 carries the TWO-PASS form of the fp16 mode (conv_mode "h2"): ldi = 2C, Cin = 2C, kwrap = 0 reads the planes
 * as [hi | lo] against weights packed [W | W] per tap, W rounded to fp16 once -- x_hi.W + x_lo.W: exact activations (to ~2^-22)
 * against single-rounded weights, f32 accumulation, twice the matrix-core work of the one-pass fp16 mode. */

/* mega_copy_segments with an f32 -> 16-bit conversion on the way (source blocks f32, destination blocks dtype = MEGA_BF16 /
 * MEGA_F16; row_bytes =
 * SOURCE bytes per row, a multiple of 32; 16-byte aligned on both sides): a concatenation of f32 row blocks delivered as the
 * rounded copy the bf16 projections read (roi_box_feature_extractors.py:812-814 pools with an f32 activation stream). */
int mega_copy_cast_segments_dt(const mega_copy_seg* segs, int n, int dtype, void* stream);

/* dst[i] = half(src[i]) (round to nearest even; dtype = MEGA_BF16 / MEGA_F16), n contiguous elements, both pointers 16-byte
 * aligned: the rounded copy of the head's f32 activation stream that the 16-bit Wq / Wk / Wv projections read
 * (roi_box_feature_extractors.py:584-597 run in one dtype; this is the mixed-precision seam of the 16-bit modes). */
int mega_cast_f32_to_half(const float* src, void* dst, size_t n, int dtype, void* stream);

/* hipGetErrorString of the last launch failure any entry point of this library reported (MEGA_ERR_LAUNCH). */
const char* mega_last_error_string(void);

/* Several independent relation-attention problems (the key frames of one engine step-batch at the same stage) in ONE
 * launch (+ one combine launch).  A problem's key-range split is a function of the problem alone, so its bits do not depend
 * on what it is batched with; mega_relation_attention / mega_relation_attention_tiled_pos_dt launch a batch of one.  n <= 20;
 * all problems share groups, scale, dtype and the kind of position term (none / f32 rows `pos` with ldp / tile-ordered 16-bit
 * `pos_tiled`). */
typedef struct {
  const void* q; const void* k; const void* vt; const float* pos; const void* pos_tiled; const void* resid;
  const float* bias_v; void* out; void* ws; size_t ws_bytes;
  int ldq, ldk, ldv, ldp, ldr, ldo, Nq, Nk;
  int io_f32;      /* != 0 with dtype bf16: resid and out are f32 rows (the head's f32 activation stream, cfg.HEAD_STREAM:
                    * x + attention is never rounded to bf16 between the stages of roi_box_feature_extractors.py:806-829) */
  int nk1;         /* keys 0 .. nk1-1 come from (k, vt), keys nk1 .. Nk-1 from (k2, vt2): the [local window ; memory] key set of a
                    * MEGA stage (roi_box_feature_extractors.py:676,:687-688,:812-814 concatenate it per key frame) read in
                    * place.  0 or Nk: one segment, k2 / vt2 ignored.  Same keys in the same order: same bits. */
  const void* k2;  /* [Nk - nk1][ldk] */
  const void* vt2; /* [groups*64][ldv2]; its columns may start at any element (2-byte) address */
  int ldv2;
  int reserved;
} mega_attn_desc;
int mega_relation_attention_batched(const mega_attn_desc* descs /* [n], host memory */, int n, int groups,
                                    float scale, int dtype, void* stream);

/* mega_position_logits_tiled_dt for n <= 20 (query boxes, key boxes) problems in one launch (mega_position_logits_tiled_batched_dt);
 * the single entry point launches a batch of one. */
typedef struct { const float* rois_q; const float* rois_k; void* out; int Nq, Nk; } mega_pos_desc;

/* Round 6: the head on IEEE-half operands (cfg.HEAD_DTYPE "float16": Q K^T, P V and the position term on
 * v_mfma_f32_32x32x16_f16 / 16x16x32_f16 -- the bf16 rate and bytes, 11 significant bits instead of 8).  The three
 * tile-ordered-logit entry points take the 16-bit type as an argument: dtype = MEGA_BF16 or MEGA_F16; the logits / Q / K /
 * V^T are that type.  mega_relation_attention and mega_relation_attention_batched take
 * MEGA_F16 through their own dtype argument.  Replaces the same reference code as the bf16 forms:
 * roi_box_feature_extractors.py:126-176 (position embedding), :567-646 (attention_module_multi_head). */
int mega_position_logits_tiled_dt(const float* rois_q, const float* rois_k, const float* wg_t, const float* bg,
                                  const float* dim_mat, void* out16, int Nq, int Nk, int dtype, void* stream);
int mega_position_logits_tiled_batched_dt(const mega_pos_desc* descs /* [n], host memory */, int n, const float* wg_t,
                                          const float* bg, const float* dim_mat, int dtype, void* stream);
int mega_relation_attention_tiled_pos_dt(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldv,
                                         const void* pos_tiled16, const void* resid, int ldr, const float* bias_v,
                                         void* out, int ldo, int Nq, int Nk, int groups, float scale, int dtype, void* ws,
                                         size_t ws_bytes, void* stream);

/* Round 6, FGFA / DFF (BASELINE configs[4]): FlowNetS's refinement levels, mega_core/modeling/backbone/flownet.py:40-52,:94-111.
 *
 * mega_conv2d_nhwc_ws with the split count chosen by the CALLER (small-M, long-K layers whose tiles would not fill the chip:
 * FlowNetS's coarse levels on 21 pairs, the FGFA box head's fc6 on 300 rows -- roi_box_feature_extractors.py:55-118).
 * ksplit >= 1 K ranges (clamped so that every range holds a K-tile), f32 partial sums in a workspace of
 * mega_conv2d_nhwc_ks_workspace_bytes(M, Cout, K, in_dtype, ksplit) bytes, added in a fixed order by a second kernel.
 * The result depends on ksplit (summation order), never on M. */
size_t mega_conv2d_nhwc_ks_workspace_bytes(int M, int Cout, int K, int in_dtype, int ksplit);
int mega_conv2d_nhwc_ks(const void* in, const void* w, const float* scale, const float* bias, const void* residual,
                        void* out, int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dil,
                        int relu, int ldo, int ldr, int in_dtype, int out_dtype, int ksplit, void* ws, size_t ws_bytes,
                        void* stream);
/* nn.ConvTranspose2d(Cin, C, 4, stride=2) + bias + activation + crop_like + its slice of the torch.cat (flownet.py:9-13,:40-52,
 * :94-111), as ONE sub-pixel GEMM: the four output phases (a, b) of a stride-2 transposed conv are a 2 x 2 / pad 1 convolution
 * with 4 C output columns (a, b, co); GEMM row (t, m, n), column (a, b, co) is written to
 *   out[t][2 m + a - crop][2 n + b - crop][coff + co]   of an NHWC tensor [N][out_H][out_W][ldo] (dropped outside it).
 * in [N][H][W][Cin]; w4 [4 C][2][2][Cin] with w4[(a*2 + b)*C + co][r][s][ci] = Wt[ci][co][a + 2 (1 - r)][b + 2 (1 - s)]
 * (Wt = the ConvTranspose2d weight [Cin][C][4][4]); bias4 f32 [4 C] (the bias once per phase) or NULL; relu as
 * mega_conv2d_nhwc; dtype = operand AND output type (MEGA_BF16 / MEGA_F16: Cin % 64 == 0; MEGA_F32: Cin % 32 == 0);
 * C a multiple of 16 (4 C = whole 64-column tiles), ldo, coff multiples of the 16-byte vector.  ksplit / ws as mega_conv2d_nhwc_ks with M = N (H+1) (W+1), Cout = 4 C,
 * K = 4 Cin.  A quarter of the matrix work of the zero-stuffed form, no zero-stuffing / crop / cat copies. */
int mega_conv2d_nhwc_subpixel(const void* in, const void* w4, const float* bias4, void* out, int N, int H, int W, int Cin,
                              int C, int relu, int out_H, int out_W, int crop, int ldo, int coff, int dtype, int ksplit,
                              void* ws, size_t ws_bytes, void* stream);
/* The rest of a refinement level's concatenation in one pass (flownet.py:94-111): out[..., 0:Cs] = skip,
 * out[..., Cs+C : Cs+C+2] = crop(ConvTranspose2d(2, 2, 4, stride=2)(flow)) computed in f32 from the f32 weights
 * w_up [2][2][4][4] / b_up [2], out[..., Cs+C+2 : ldo] = 0.  skip [N][H2][W2][Cs], flow [N][h][w][2], out [N][H2][W2][ldo] of
 * `dtype`; crop: rows / columns of the full (2h+2) x (2w+2) map dropped at the top / left. */
int mega_flow_level_assemble(const void* skip, const void* flow, const float* w_up, const float* b_up, void* out, int N,
                             int H2, int W2, int Cs, int C, int ldo, int h, int w, int crop, int dtype, void* stream);

/* FlowNetS flow prediction (flownet.py:40-52 Convolution1..5 = nn.Conv2d(Cin, 2, 3, padding=1)), second half: by linearity the
 * 3 x 3 conv with two output channels is a 1 x 1 conv with 18 columns z[p][(r*3 + s)*2 + c] = sum_ci x[p][ci] w[c][ci][r][s]
 * (mega_conv2d_nhwc, f32 output: one pass over x, K = Cin instead of 9 Cin on 64-wide tiles) followed by
 *   out[t][y][x][c] = (sum_{r,s} z[t][y+r-1][x+s-1][(r*3+s)*2 + c]) * scale + bias[c]     (f32, taps outside the map skipped).
 * z f32 [N][H][W][ldz], ldz >= 18 and even; bias f32 [2]; out [N][H][W][2] of out_dtype (MEGA_F32 / MEGA_BF16 / MEGA_F16). */
int mega_flow_pred_finish(const float* z, int ldz, const float* bias, float scale, void* out, int N, int H, int W,
                          int out_dtype, void* stream);

/* FlowNetS flow_conv1 (flownet.py:52,:56: Conv2d(6, 64, 7, stride 2) + LeakyReLU(0.1) on cat([key, frame_t]) / 255) per FRAME
 * instead of per pair: the conv is linear before its activation, so conv(pair) = conv_key(key frame) + conv_ref(frame_t); both
 * halves [A | B] of a frame are computed once, when it enters the window (mega_conv2d_nhwc with 128 output channels over that
 * frame's tap operand, f32 out), and a key frame's 21 pairs are  out[t][p][c] = leaky(A[key][p][c] + B[t][p][c] + bias[c]).
 * ab f32 [S][P][128]; bias f32 [64]; order (device int; NULL: use `key`): order[0] = slot of the key frame; out [T][P][64] of
 * dtype (MEGA_BF16 / MEGA_F16), pair t = (key frame, the frame in slot t).  nwin > 0: order holds G rows [key slot, slot of
 * window position 0 .. nwin-1], T = G nwin, pair g nwin + t = (key frame of row g, window position t): exactly the pairs of G
 * key frames, in window order. */
int mega_flow_conv1_combine(const float* ab, const float* bias, const int* order, int key, void* out, int T, long long P,
                            int nwin, int dtype, void* stream);
/* mega_fgfa_warp_aggregate_ring with the flow fields in WINDOW order: flow [T][2][H][W] = the T pairs (key frame, window
 * position t) and nothing else; key_pos = the key frame's window position (cfg KEY_FRAME_LOCATION).  What a FlowNetS pass over
 * the exact pairs of several key frames (mega_flow_conv1_combine with nwin > 0) hands to the warp.  Shape limits: see
 * mega_fgfa_warp_aggregate. */
int mega_fgfa_warp_aggregate_ring_pos(const void* feats, const float* flow, void* out, float* weights_out, int T, int H,
                                      int W, int Cf, int Ce, const int* order, int key_pos, int dtype, void* stream);
/* ... for G key frames in one launch: order [G][1 + T], flow [G][T][2][H][W], out [G][H][W][Cf], weights_out [G][T][H][W] or
 * NULL; the feature ring `feats` is shared.  Same bits per key frame as G separate calls. */
int mega_fgfa_warp_aggregate_ring_pos_batched(const void* feats, const float* flow, void* out, float* weights_out, int T,
                                              int H, int W, int Cf, int Ce, const int* order, int key_pos, int G, int dtype,
                                              void* stream);

/* ImageNet VID evaluation (AP50 and motion-specific AP).  Replaces the Python loops of
 * mega_core/data/datasets/evaluation/vid/vid_eval.py:156-285 (calc_detection_vid_prec_rec) and :288-343
 * (calc_detection_vid_ap, use_07_metric=False), for F frames, R motion ranges and C classes (labels 0 .. C-1).
 * Matching: one wave per (frame, range).  Inputs, flat over frames:
 *   det_box [N][4] f32 in the prediction's frame size, det_label [N] i32, det_off [F+1] i64 (frame f's detections are
 *   det_off[f] .. det_off[f+1]), order [N] i32: detection indices, each frame's run ordered by label, then score
 *   descending, then position descending; ratio [F][2] f32 = (annotation width / prediction width, height / height) as in
 *   BoxList.resize (bounding_box.py:91-125); gt_box [G][4] f32, gt_label [G] i32, gt_off [F+1] i64; gt_motion [G] f64 or
 *   NULL (NaN: the frame has no motion list, nothing is ignored); ranges [R][3] f64 = (lo, hi, empty_weight); max_gt = the
 *   largest GT count of a frame (<= 4096).
 * Outputs: match [R][N] u8, pred_ignore [R][N] f64 (indexed by detection), n_pos [R][C] i32 (non-ignored GT per class). */
int mega_vid_eval_match(const float* det_box, const int* det_label, const long long* det_off, const int* order,
                        const float* ratio, const float* gt_box, const int* gt_label, const double* gt_motion,
                        const long long* gt_off, const double* ranges, int F, int R, int C, long long N, int max_gt,
                        unsigned char* match, double* pred_ignore, int* n_pos, void* stream);
/* Precision / recall / AP: one workgroup per (class, range) sweeps the class's detections in global order
 * gorder[seg_off[l] .. seg_off[l+1]) (score descending, equal scores by descending position in the frame-by-frame
 * concatenation): inclusive tp (integer) / fp (f64) scans, prec = tp / (fp + tp + 2^-52), rec = tp / n_pos, the
 * precision envelope (suffix max) and AP = sum of (rec_j - rec_j-1) * envelope_j where recall changes.  ap [R][C] f64,
 * NaN where n_pos is 0.  Workspace: mega_vid_eval_workspace_bytes(N, C, R) bytes. */
size_t mega_vid_eval_workspace_bytes(long long N, int C, int R);
int mega_vid_eval_ap(const unsigned char* match, const double* pred_ignore, const int* gorder, const long long* seg_off,
                     const int* n_pos, int C, int R, long long N, double* ap, void* ws, size_t ws_bytes, void* stream);

/* ImageNet VID proposal recall: the greedy one-to-one matching of
 * mega_core/data/datasets/evaluation/vid/vid_eval.py:72-119 (eval_proposals_vid), for F frames and nL proposal limits in
 * one launch, one wave per (frame, limit).  Inputs, flat over frames:
 *   box [N][4] f32 in the prediction's frame size, off [F+1] i64 (frame f's proposals are off[f] .. off[f+1]), order [N]
 *   i32: proposal indices, each frame's run in the order the evaluation takes them (objectness descending, equal values by
 *   ascending position); only the first min(limits[l], off[f+1] - off[f]) of a run are used; ratio [F][2] f32 as for
 *   mega_vid_eval_match; gt_box [G][4] f32, gt_off [F+1] i64; limits [nL] i32, each <= max_limit <= 1024; max_gt = the
 *   largest GT count of a frame (<= 4096).
 * Per (frame, limit), min(proposals, GT boxes) rounds: the live (proposal, GT) pair of largest IoU (boxlist_iou: +1
 * convention, f32; ties: the lower GT index, then the lower position in the frame's order) is recorded and both are
 * removed.  A NaN IoU is never chosen.
 * Outputs, indexed by the GT box's own position in gt_box: gt_overlap [nL][G] f32 (0 for a GT box that is never matched),
 * gt_prop [nL][G] i32: the matched proposal's position in its frame's order, or -1. */
int mega_proposal_recall_match(const float* box, const long long* off, const int* order, const float* ratio,
                               const float* gt_box, const long long* gt_off, const int* limits, int F, int nL, long long N,
                               long long G, int max_limit, int max_gt, float* gt_overlap, int* gt_prop, void* stream);

/* Seq-NMS video-level rescoring (mega/pytorch_amd/seq_nms.py defines it; the reference has no counterpart).  One
 * workgroup per (video, class) task; per task, until no box is alive: forward DP in f64 over the frames (S = score + the
 * best S of an alive box of the previous frame with IoU > link_iou, arg-max P: smallest position on equal S), the best
 * end box (largest S, then earliest frame, then smallest position), backtrack, rescore the path (rescore_max = 0: f32(S /
 * path length), 1: the largest score on the path), remove the path boxes and every alive box with IoU > nms_iou to them.
 * IoU: the +1 convention in f32.  The DP is recomputed incrementally after each removal (bit-identical to a full pass).
 * Inputs, sorted class-major then frame, positions kept within each (class, frame) run:
 *   box [N][4] f32, score [N] f32 (>= 0), seg_off [C * F + 1] i64 (class c, frame f: seg_off[c F + f] .. seg_off[c F + f
 *   + 1]), tasks [T][3] i32 = (class, first frame, frame count) of each task, longest first.
 * Outputs (same order): keep [N] u8 (1: on a path), new_score [N] f32 (set where keep is 1), stats [T][2] i64 or NULL =
 * (iterations, DP frame steps) per task.  Thresholds in [0, 1].  Workspace: mega_seq_nms_workspace_bytes(N, C * F).
 * Synchronises the stream: returns MEGA_ERR_LIMIT if a task ran past its loop bound (its box count). */
size_t mega_seq_nms_workspace_bytes(long long N, long long segs);
int mega_seq_nms(const float* box, const float* score, const long long* seg_off, const int* tasks, int T, int F, int C,
                 long long N, float link_iou, float nms_iou, int rescore_max, unsigned char* keep, float* new_score,
                 long long* stats, void* ws, size_t ws_bytes, void* stream);

/* Linking detections into tracks (mega/pytorch_amd/tracks.py defines it; the reference has no counterpart).  One
 * workgroup per (video, class) task; per task, frames t ascending: close every open track whose last frame is
 * < t - max_gap - 1; then the frame's boxes with score >= score_thresh, in descending score (equal scores: ascending
 * position), each join the open track with last frame < t of the largest iou(track's last box, box) > link_iou (strict; on
 * equal IoU the track whose root has the smallest pos), or open a new track with themselves as the root.  A track extended
 * or born in frame t is not available in frame t; a NaN IoU never links.  IoU: the +1 convention in f32, as mega_seq_nms.
 * Inputs, sorted class-major then frame, and within each (class, frame) run by descending score, equal scores by
 * ascending position:
 *   box [N][4] f32, score [N] f32 (>= 0), pos [N] i32 (the box's position in the frame-by-frame concatenation: the tie
 *   key), seg_off [C * F + 1] i64 and tasks [T][3] i32 as for mega_seq_nms.
 * Outputs (same order): root [N] i64 = the index (in this order) of the first box of the box's track, -1 for a box below
 * score_thresh; and at each root's index cnt i32 = the track's box count, sum f64 = its members' scores added in frame
 * order, mx f32 = the largest of them (other elements are not written).
 * max_open: the caller's bound on the open tracks of a task (e.g. the most boxes of one class in max_gap + 2 consecutive
 * frames); tracks beyond the 1024 kept in LDS live in the workspace, mega_link_tracks_workspace_bytes(T, max_open).
 * link_iou in [0, 1], score_thresh not NaN, max_gap >= 0; negative sizes: MEGA_ERR_ARG; N = 0 or T = 0 is a no-op.
 * Synchronises the stream: returns MEGA_ERR_LIMIT if a task would have opened more than max_open tracks. */
size_t mega_link_tracks_workspace_bytes(int T, int max_open);
int mega_link_tracks(const float* box, const float* score, const int* pos, const long long* seg_off, const int* tasks,
                     int T, int F, int C, long long N, float score_thresh, float link_iou, int max_gap, int max_open,
                     long long* root, int* cnt, double* sum, float* mx, void* ws, size_t ws_bytes, void* stream);

/* Refining linked tracks: gap frames filled by interpolation, boxes smoothed along the track
 * (mega/pytorch_amd/tracks.py defines it; the reference has no counterpart).  One 256-thread workgroup per tile of 256
 * output slots, plus a halo of r slots on each side held in LDS; one launch, no atomics, no status word.  Inputs:
 *   m_box [M][4] f32, m_score [M] f32 (>= 0), m_frame [M] i32 (dataset frame): the members (boxes with a track id) sorted
 *   by (video, track id, frame); m_off [K + 1] i64: track k's members are m_off[k] .. m_off[k + 1] (at least one, frames
 *   strictly ascending); o_off [K + 1] i64, o_off[0] = 0, o_off[K] = S: track k's output slots, with fill = 1 one per frame
 *   from its first member's frame to its last member's, with fill = 0 one per member.
 * A slot that is a member copies it; any other slot f between the members a, b that bracket it gets, per coordinate in
 * f32 without contraction, a.c + (b.c - a.c) * (f32(f - fa) / f32(fb - fa)) and the score min(a.score, b.score) *
 * fill_scale.  With r > 0 every slot's box is then the mean of the unsmoothed boxes of its own track's slots within r
 * frames: f64 sum in ascending frame order starting from the first term, / count, rounded once to f32.
 * Outputs, per slot: out_box [S][4] f32, out_score [S] f32, out_frame [S] i32, out_track [S] i32 (k), out_src [S] i32 (the
 * member's index, -1 for a filled slot), out_filled [S] u8 (1 for a filled slot).
 * Negative sizes, M or S above 2^31 - 1, a NULL pointer with a non-zero size, S > 0 with K = 0 or M = 0, fill outside
 * 0..1, r outside 0..64, fill_scale outside (0, 1]: MEGA_ERR_ARG; a workspace below
 * mega_refine_tracks_workspace_bytes(S, r) (0: a tile and its halos live in LDS): MEGA_ERR_WS; both before any launch.
 * S = 0 launches nothing.  Does not synchronise. */
size_t mega_refine_tracks_workspace_bytes(long long S, int r);
int mega_refine_tracks(const float* m_box, const float* m_score, const int* m_frame, const long long* m_off,
                       const long long* o_off, int K, long long M, long long S, int fill, int r, float fill_scale,
                       float* out_box, float* out_score, int* out_frame, int* out_track, int* out_src,
                       unsigned char* out_filled, void* ws, size_t ws_bytes, void* stream);

/* Tubelet AP: matching linked tracks (tubelets) against ground-truth tracks by temporal IoU
 * (mega/pytorch_amd/track_eval.py defines it; the reference has no counterpart).  One workgroup per (video, label) task
 * with P tubelets and G GT tracks (G <= 4096).  Phase 1 counts, per pair, both = frames where both have a box and hits =
 * those where the box IoU (mega_vid_eval_match's: prediction rescaled by ratio in f32, +1 on x2 / y2, boxlist_iou) is
 * >= 0.5f; the two i32 tables live in LDS when P * G <= 4096, else in the workspace.  Phase 2, per threshold num / den: the
 * tubelets in rank order each take the untaken GT track with hits > 0 and hits * den >= num * union (union = tubelet
 * length + GT length - both) of the largest hits / union, compared cross-multiplied in 64-bit integers; on an equal value
 * the lowest GT track.  Inputs (device unless noted):
 *   box [M][4] f32, frame [M] i32 (dataset frame), rank [M] i32 (the box's tubelet: its rank within its task): the tubelet
 *   boxes sorted class-major then frame, seg_off [C * F + 1] i64 as for mega_seq_nms; ratio [F][2] f32;
 *   gt_box [Gb][4] f32, gt_track [Gb] i32 (the box's GT track: its index within its task), sorted the same way,
 *   gt_seg_off [C * F + 1] i64;
 *   tasks [T][8] i32 = (class, first frame, frames, p0, P, g0, G, 0), the most boxes first; offs [T][2] i64 = (offset of the
 *   task's P x G table in hits / both, offset of its table in the workspace or -1);
 *   tubelet [slots] i32: the tubelet index u of task slot p0 + rank; tub_len [U] i32; gt_len [J] i32 by GT slot g0 + index;
 *   thresholds: HOST int [R][2] = (num, den), 0 < num <= den <= 1024, R <= 8.
 * Outputs: match [R][U] u8 and matched_gt [R][U] i32 (GT slot g0 + index, -1: none), written for the tubelets of the T
 * tasks only (the caller presets 0 / -1); hits / both [n_pairs] i32 or both NULL: the pair tables, task by task.
 * Negative sizes, a threshold outside the range, R outside 1..8: MEGA_ERR_ARG; workspace below
 * mega_tubelet_match_workspace_bytes(ws_pairs) (ws_pairs = the pairs of the tasks with P * G > 4096): MEGA_ERR_WS; both
 * before any launch.  T = 0 is a no-op.  A task whose table entries do not fit the sizes is skipped.  Does not
 * synchronise. */
size_t mega_tubelet_match_workspace_bytes(long long ws_pairs);
int mega_tubelet_match(const float* box, const int* frame, const int* rank, const long long* seg_off, const float* ratio,
                       const float* gt_box, const int* gt_track, const long long* gt_seg_off, const int* tasks,
                       const long long* offs, const int* tubelet, const int* tub_len, const int* gt_len,
                       const int* thresholds, int T, int F, int C, int R, long long M, long long Gb, long long U,
                       long long J, long long slots, long long n_pairs, long long ws_pairs, unsigned char* match,
                       int* matched_gt, int* hits, int* both, void* ws, size_t ws_bytes, void* stream);
/* The tubelet score of track_eval.py: out[u] f64 = the f32 scores score[off[u] .. off[u+1]) (a tubelet's members in frame
 * order) added in f64 in that order, divided by their count; with use_max = 1 the largest of them.  One thread per
 * tubelet.  U = 0 is a no-op. */
int mega_tubelet_scores(const float* score, const long long* off, long long U, long long M, int use_max, double* out,
                        void* stream);

/* Motion IoU of every GT box (mega/pytorch_amd/motion_iou.py defines it; the reference reads such values from a file):
 * the mean IoU of a box with the boxes of its own track in the +-W neighbouring frames of its video.  One wave64 per
 * frame: its lanes stride over the frame's (box, offset) pairs, each scanning the neighbour frame's track ids; the pair
 * IoUs (the box with +1 on x2 / y2 against the neighbour: mega_vid_eval_match's IoU of a detection that coincides with
 * the box) are kept per box in offset order (-W .. -1, +1 .. +W), in LDS while a frame's boxes x 2W <= 2048, else in the
 * workspace; one lane per box then adds the found ones in that order in f64 and divides by their count.  No atomics: the
 * same bits on every run.
 *   gt_box [G][4] f32, gt_track [G] i64 (unique within a frame), gt_off [F + 1] i64 (frame f's boxes), video_start /
 *   video_end [F] i32: the frame range [start, end) of frame f's video; W in 1..64; max_gt: the most boxes of a frame
 *   (<= 4096).
 * Outputs: values [G] f64 (0.0 without a neighbour, the quiet NaN 0x7ff8000000000000 if a pair IoU is NaN), counts [G] i32
 * (the neighbours found).  A frame whose offsets do not fit G or that holds more than max_gt boxes is skipped.
 * NULL pointers (gt_box / gt_track / values / counts may be NULL only when G = 0, video_start / video_end only when F = 0),
 * F < 0, G < 0, W outside 1..64, max_gt outside 0..4096: MEGA_ERR_ARG; a workspace below mega_motion_iou_workspace_bytes(G, W, max_gt) (0 when max_gt * 2W <=
 * 2048, else the slots of all G boxes): MEGA_ERR_WS; both before any launch.  F = 0 or G = 0 launches nothing.  Does not
 * synchronise. */
size_t mega_motion_iou_workspace_bytes(long long G, int W, int max_gt);
int mega_motion_iou(const float* gt_box, const long long* gt_track, const long long* gt_off, const int* video_start,
                    const int* video_end, int F, long long G, int W, int max_gt, double* values, int* counts, void* ws,
                    size_t ws_bytes, void* stream);

/* Detection error diagnosis (mega/pytorch_amd/diagnose.py defines it; the reference has no counterpart): the kind of every
 * detection and the detections that found or nearly found every GT box, for F frames and labels 0 .. C-1.  One wave per
 * frame.  The IoU is mega_vid_eval_match's throughout (prediction rescaled by ratio in f32, +1 on x2 / y2, boxlist_iou, no
 * contraction); a NaN IoU satisfies no comparison; tf = 0.5f and tb = bg_thresh are compared in f32 with >=.
 *   Matching: mega_vid_eval_match's for one range and no motion list -- per frame, in the frame's run of `order` (label,
 *   then score descending, then position descending), each detection takes the not yet taken GT box of its label with the
 *   largest IoU >= tf, the lowest GT index among equals: a TP.
 *   Every other detection, with a / ga = the largest IoU with a GT box of its label and that box (lowest index on a tie),
 *   b / gb the same over the boxes of other labels ("none" meets no threshold), by the first rule that holds:
 *   DUPE a >= tf (ga), LOC tb <= a < tf (ga), CLS b >= tf (gb), BOTH tb <= b < tf (gb), else BKG (no box).
 * Inputs, flat over frames: det_box [N][4] f32, det_label [N] i32, det_score [N] f32 (no NaN), det_off [F+1] i64, order [N]
 * i32 and ratio [F][2] f32 as for mega_vid_eval_match; gt_box [G][4] f32, gt_label [G] i32, gt_off [F+1] i64; max_gt = the
 * largest GT count of a frame (<= 4096).
 * Outputs, every element written: det_kind [N] u8 (0 TP, 1 DUPE, 2 LOC, 3 CLS, 4 BOTH, 5 BKG), det_gt [N] i32 (the matched
 * or attributed box's index in gt_box, -1 for BKG), det_iou [N] f32 (the IoU with that box, 0 for BKG); gt_det [3][G] i32,
 * per GT box the index of the TP that took it, of the best LOC and of the best CLS detection attributed to it (-1: none;
 * best = the highest score, on equal scores the higher position in its frame).
 * No workspace, no atomics.  A NULL pointer with a non-zero size, negative sizes, C <= 0, max_gt > 4096, N > 2^31 - 1,
 * bg_thresh outside (0, 0.5): MEGA_ERR_ARG before any launch.  F = 0 launches nothing.  Does not synchronise. */
int mega_diagnose_match(const float* det_box, const int* det_label, const float* det_score, const long long* det_off,
                        const int* order, const float* ratio, const float* gt_box, const int* gt_label,
                        const long long* gt_off, int F, int C, long long N, long long G, int max_gt, float bg_thresh,
                        unsigned char* det_kind, int* det_gt, float* det_iou, int* gt_det, void* stream);

/* Detection overlay of the demo (mega/pytorch_amd/demo.py defines it), in place on F original-size frames, no host round
 * trip.  Per frame: rows i < counts[f] with score > thr (strict), drawn in descending score order (equal scores: ascending
 * row); box -> original frame by ONE f32 multiply per coordinate (x * sx, y * sy; sx = f32(W / resized width) computed by
 * the caller) and truncation toward zero; degenerate boxes, boxes wholly outside the image and classes outside [0, NC)
 * are dropped.  All outlines (thickness odd: the pixels within Chebyshev distance (thickness - 1) / 2 of the 1-pixel
 * rectangle, colour palette[class]) are drawn in that order, then all labels "<name>: D.DD" on top: the rectangle (sum of
 * the glyph advances wide, gh high, its bottom on the box's top edge, moved inside the box at the image's top, clamped
 * horizontally) filled with the class colour c and blended with white by glyph coverage a: (c (255 - a) + 255 a + 127) /
 * 255.  D.DD are the digits of "%.2f" for scores in [0, 1] (rint of the exact f64 product score * 100).
 *   frames [F][H][W][3] u8 (in / out); boxes [F][R][4] f32 xyxy; scores [F][R] f32; labels [F][R] i64 (labels_i64 = 1) or
 *   i32; counts [F] i32; palette [NC][3] u8; class_glyphs [NC][ML] i32: the glyphs of each class name, ended by a value
 *   outside [0, G) (ML <= 18); fmt_glyphs [13] i32: the glyphs of '0'..'9', ':', ' ', '.'; cov [G][gh][gw] u8 coverage,
 *   adv [G] i32 advances (a glyph shows its first min(adv, gw) columns); G <= 256.
 * select_only = 1 stops after the selection pass (timing).  thickness even or < 1: MEGA_ERR_ARG; R > 512:
 * MEGA_ERR_LIMIT, both before any launch.  R = 0 is a no-op.  Workspace: mega_overlay_detections_workspace_bytes(F, R). */
size_t mega_overlay_detections_workspace_bytes(int F, int R);
int mega_overlay_detections(unsigned char* frames, int F, int H, int W, const float* boxes, const float* scores,
                            const void* labels, int labels_i64, const int* counts, int R, float sx, float sy, float thr,
                            int thickness, const unsigned char* palette, int NC, const int* class_glyphs, int ML,
                            const int* fmt_glyphs, const unsigned char* cov, const int* adv, int G, int gh, int gw,
                            int select_only, void* ws, size_t ws_bytes, void* stream);

/* Conv2d + FrozenBatchNorm2d scale / bias + ReLU on FP8 operands (OCP e4m3fn: bias 7, largest finite value 448, no infinities;
 * not MI300's fnuz), f32 accumulation on the block-scaled MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, unit block scales): the
 * opt-in FP8 path of layer3's conv1 / conv2 (cfg FP8_CONV; backbone/resnet.py:324-344).  mega/pytorch_amd/f8.py defines the
 * quantisation  quantize(v, inv) = e4m3(clamp(f32(v) * inv, -448, 448)), round to nearest even.
 *   in    [N][H][W][Cin]: in_dtype MEGA_F8 (the producer's codes; in_inv_scale is not read) or MEGA_BF16 (quantised on the load
 *         path with in_inv_scale = 1 / s_in: no fp8 copy of the tensor is ever written)
 *   w_f8  [Cout][R][S][Cin] codes (OHWI), one scale sw[c] per output channel
 *   out   [N*H*W][Cout]: out_dtype MEGA_BF16, y rounded once, or MEGA_F8, quantize(y, out_inv_scale)
 *   y = act(acc * scale[c] + bias[c]), acc = the f32 sum of code products; the caller folds s_in * sw[c] * bn_scale[c] into
 *   scale.  scale / bias: f32 [Cout] or NULL (1 / 0).  relu 0 / 1.  No residual operand, no workspace, no synchronisation.
 * Admitted: 1x1 / stride 1 / pad 0 and 3x3 / stride 1 / pad 1 / dil 1, Cin % 128 == 0, Cout % 64 == 0, N H W < 2^30; anything
 * else returns MEGA_ERR_ARG before any launch, the output untouched.  A padding tap contributes +0. */
int mega_conv2d_nhwc_f8(const void* in, int in_dtype, float in_inv_scale, const void* w_f8, const float* scale,
                        const float* bias, void* out, int out_dtype, float out_inv_scale, int N, int H, int W, int Cin,
                        int Cout, int R, int S, int stride, int pad, int dil, int relu, void* stream);
/* < 0: mega_conv2d_nhwc_f8 does not admit the layer; else its tile class, the columns of the 128-row block tile (256 when
 * Cout % 256 == 0, else 64).  Computed by the function the launch itself uses; launches nothing. */
int mega_conv2d_nhwc_f8_plan(int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dil, int in_dtype,
                             int out_dtype);

/* JPEG decode, host entropy stage + device pixel stages (mega/pytorch_amd/jpeg.py defines the accepted streams, the layout and
 * the arithmetic; replaces the PIL.Image.open(...).convert("RGB") of the reference's loader, mega_core/data/datasets/vid.py
 * __getitem__ / vid_mega.py:95-142, bit for bit).
 * mega_jpeg_probe: parse the markers of the JPEG at data[0, nbytes) (host memory) and fill info[MEGA_JPEG_INFO_INTS]:
 *   0 width, 1 height, 2 components, 3 sampling code (0 gray, 1 4:4:4, 2 4:2:2, 3 4:2:0), 4 + 2c / 5 + 2c blocks per row /
 *   column of component c over the MCU-padded grid, 10 restart interval, 11 int16 elements mega_jpeg_entropy_decode writes.
 *   MEGA_ERR_ARG for anything outside the accepted set (or not a JPEG); info is then untouched.
 * mega_jpeg_entropy_decode: Huffman-decode the same bytes into out (host memory, out_elems >= info[11] int16 elements):
 *   qt[3][64], the quantisation table of each component in natural order, then the coefficient planes of Y, Cb, Cr,
 *   [block row][block col][64] in natural order, not dequantised.  info: a probe's result the stream must agree with in entries
 *   0 to 3.  Every element of out[0, info[11]) is written.  MEGA_ERR_ARG for a refused, mismatching, truncated or corrupt
 *   stream; never reads outside data or writes outside out. */
#define MEGA_JPEG_INFO_INTS 12
int mega_jpeg_probe(const unsigned char* data, long long nbytes, int* info);
int mega_jpeg_entropy_decode(const unsigned char* data, long long nbytes, const int* info, short* out, long long out_elems);
/* mega_jpeg_reconstruct: N frames of one size and sampling code, frame n's coefficients (the layout above) at coef + n * stride
 * (device, int16 elements; stride % 8 == 0 and coef 16-byte aligned) -> rgb [N][H][W][3] uint8.  Two launches: dequantise +
 * integer IDCT + clamp into component planes in ws, then chroma upsampling + YCbCr -> RGB.  MEGA_ERR_ARG before any launch
 * for N outside [1, 65535], H or W outside [1, 65535], an unknown sampling code, a stride below the frame's element count or
 * not a multiple of 8, a NULL pointer, ws off an 8-byte boundary, rgb off a 4-byte boundary when W % 4 == 0 (other widths are
 * stored byte by byte, so a slice of a batch of odd-sized frames is accepted); MEGA_ERR_WS for a workspace below
 * mega_jpeg_reconstruct_workspace_bytes(N, H, W, sampling) (0 for arguments the launch would refuse). */
size_t mega_jpeg_reconstruct_workspace_bytes(int N, int H, int W, int sampling);
int mega_jpeg_reconstruct(const short* coef, long long stride, int N, int H, int W, int sampling, unsigned char* rgb, void* ws,
                          size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MEGA_HIP_H */
