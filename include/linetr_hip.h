/*
 * linetr_hip.h -- C ABI of the MI355X-native (gfx950) Line-Transformer descriptor + matcher.
 *
 * This is the drop-in boundary for the hot path of yosungho/LineTR: every entry point names the
 * reference interface it replaces (paths relative to the reference checkout).  Plain pointers and
 * sizes only -- no torch/ATen types.  All `d_*` pointers are DEVICE pointers (HIP), `h_*` are HOST
 * pointers.  `stream` is a hipStream_t passed as void* (NULL = default stream).  Every function
 * returns 0 on success or a negative LINETR_E_* code; linetr_last_error() returns a message for the
 * calling thread.  Nothing here ever falls back to a CPU implementation: if no HIP device is
 * usable, linetr_create() fails.
 *
 * Host-side contract of every entry point.  No C++ exception leaves this interface because of an argument's value: a count, an offset
 * table, a capacity or a name that cannot be served is refused with a LINETR_E_* code and a message (running out of memory has no
 * code and is the one thing left out).  A size query (`*_workspace_bytes`, `*_output_bytes`, `*_pack_bytes`) never returns a wrapped
 * number: its byte count is formed in int64_t behind a range check, and a shape whose size cannot be formed (beyond 2^56 bytes, far
 * beyond any device) answers 0, as does a shape the query's own text says its entry point refuses; the entry point refuses such a
 * shape whatever workspace it is given.  Where a query's text says nothing else, a negative count counts as 0.  The answer for every
 * shape an entry point serves is the exact number of bytes it asks for.
 *
 * Call sequence for one batch of B images (one image = B=1):
 *     linetr_prefilter / linetr_pack_lines   (host, O(K) per image)  -> line records
 *     linetr_tokenize                         (device)                -> the tensors of `preprocess`
 *     linetr_forward                          (device)                -> line_desc
 *     linetr_match                            (device)                -> Dk, match indices
 * or, for throughput:  linetr_prefilter_batch -> linetr_describe (tokenise + forward fused, var-len batch) -> linetr_match;
 * streams of batches:  linetr_describe_submit / linetr_describe_join (the same call as a software pipeline over consecutive batches).
 * ABI version 5 (r06): + linetr_describe_submit, linetr_describe_join, linetr_pipeline_max_slots.
 * ABI version 6: + linetr_debug_sig_attention (one chosen signature-attention kernel alone, for the unit tests).
 *                + linetr_debug_gemm_case (one chosen GEMM tile alone on a full problem description, for the unit tests): an added
 *                diagnostics symbol, nothing existing changes, so the version stays.
 *                + linetr_debug_tok_mlp, linetr_debug_cls_pool (the descriptive layer's front-end kernels alone, for the unit
 *                tests): added diagnostics symbols again, the version stays.
 *                + linetr_debug_match (one chosen path of the matcher alone, for the unit tests): an added diagnostics symbol, the
 *                version stays.
 *                + linetr_debug_bn_train, linetr_debug_bn_train_workspace_bytes (the train-mode BatchNorm kernels alone, for the
 *                unit tests): added diagnostics symbols, the version stays.
 *                + linetr_bn_forward, linetr_bn_backward and their _workspace_bytes (BatchNorm on batch statistics with a backward): added
 *                symbols, nothing existing changes, the version stays.
 *                + linetr_cls_pool_train_forward / _backward, linetr_layer_norm_forward / _backward / _backward_workspace_bytes,
 *                linetr_gelu_forward / _backward (the descriptive layer's training kernels): added symbols, the version stays.
 *                + linetr_input_layer_forward / _backward / _backward_workspace_bytes / _chunk_rows, linetr_token_assemble_forward /
 *                _backward / _backward_workspace_bytes (the positional encoders' first layer and the token assembly): added symbols,
 *                the version stays.
 *                + LinetrDropout, linetr_cls_pool_dropout_forward / _backward, linetr_layer_norm_dropout_forward / _backward,
 *                linetr_dropout_factors (training-time dropout of the descriptive layer, masks generated in the kernels): added
 *                symbols, the version stays.
 *                + LinetrAdamTensor, LinetrAdamHyper, linetr_adam_step, linetr_grad_norm and their _workspace_bytes (the optimizer
 *                step over a table of tensors and the gradient norm that can feed it): added symbols, the version stays.
 *                + linetr_debug_stage, linetr_debug_stage_workspace_bytes (the descriptive layer's tail or the signature network
 *                alone, through the forward pass's own host functions, for the unit tests): added diagnostics symbols, the version stays.
 *                + LinetrPreparedEntry, linetr_debug_prepare (linetr_create's weight preparation alone, on the host, for the unit
 *                tests): an added diagnostics symbol, the version stays.
 *                + linetr_hardnet_loss_grad, linetr_hardnet_loss_grad_workspace_bytes (the HardNet criterion, value and gradient):
 *                added symbols, nothing existing changes, the version stays.
 */
#ifndef LINETR_HIP_H
#define LINETR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LINETR_ABI_VERSION 6

enum {
  LINETR_OK = 0,
  LINETR_E_ARG = -1,       /* bad argument / unsupported configuration            */
  LINETR_E_HIP = -2,       /* a HIP runtime call failed                            */
  LINETR_E_WEIGHTS = -3,   /* state_dict tensor missing / wrong size               */
  LINETR_E_ASSERT = -4,    /* reference AssertionError: token beyond the line end  */
  LINETR_E_WORKSPACE = -5, /* workspace too small                                  */
  LINETR_E_CAPACITY = -6   /* caller-provided output capacity too small            */
};

typedef struct LinetrHandle LinetrHandle;

/* Model hyper-parameters: LineTransformer.default_config, models/line_transformer.py:187-201. */
typedef struct {
  int32_t d_model;          /* descriptor_dim, must be 256                                  */
  int32_t n_heads;          /* must be 4                                                    */
  int32_t d_inner;          /* FFN width, multiple of 128 (default 1024)                    */
  int32_t n_sig_layers;     /* line-signature layers (7)                                    */
  int32_t n_desc_layers;    /* n_line_descriptive_layers; only the LAST one reaches the     */
                            /* output (models/line_transformer.py:123-125)                  */
  int32_t enc_channels[4];  /* keyline_encoder = {32,64,128,256}                            */
  int32_t norm_height;      /* constructor-time image_shape used by normalize_keylines      */
  int32_t norm_width;       /* (models/line_transformer.py:206,:238)                        */
  int32_t bn_batch_stats;   /* 0: BatchNorm(eval) folded into the convolutions (inference).  1: a TRAINING-mode handle      */
                            /* (train.py:127 -> model.train()): the convolutions stay unfolded and only                      */
                            /* linetr_forward_train may run on it                                                            */
} LinetrModelConfig;

/* One key-line after pre-filtering (float64 geometry exactly as the reference keeps it in NumPy). */
typedef struct {
  double sp[2];        /* start point (x,y), post remove_borders clip                           */
  double ep[2];        /* end point                                                            */
  double length;       /* lineLength * 2^octave (models/line_process.py:220) -- NOT geometric   */
  double angle[2];     /* (cos 2theta, sin 2theta), models/line_process.py:28-41                */
  int32_t first_sub;   /* index of this line's first sub-line inside the whole batch           */
  int32_t n_tok;       /* ceil(length / token_distance), models/line_process.py:109            */
  int32_t n_sub;       /* ceil(n_tok / max_tokens), models/line_process.py:121                 */
  int32_t image;       /* image index inside the batch                                         */
  int32_t line_local;  /* index of this key-line inside its image                              */
  int32_t first_tok;   /* index of this line's first REAL token in the batch-wide compact list  */
} LinetrLineRec;       /* 80 bytes */

/* Device outputs of the tokeniser == the tensor entries LineTransformer.preprocess returns
 * (models/line_process.py:182-193), leading batch-1 axis dropped, images concatenated.
 * K = total key-lines, N = total sub-lines, T = max_tokens, S = T+1.  All float32. */
typedef struct {
  float* klines;      /* [K,2,2]                                                    */
  float* length;      /* [K]                                                        */
  float* angles;      /* [K,2]                                                      */
  float* sublines;    /* [N,2,2]                                                    */
  float* pnt;         /* [N,T,2]   pnt_sublines                                     */
  float* mask;        /* [N,S]     mask_sublines (trailing 1-axis dropped)          */
  float* resp;        /* [N]       resp_sublines                                    */
  float* angle_sub;   /* [N,2]     angle_sublines                                   */
  float* desc;        /* [N,T,256] desc_sublines                                    */
  float* score;       /* [N,T]     score_sublines                                   */
  float* mat;         /* mat_klines2sublines (models/line_process.py:160-165): per image a [K_i,N_i] block, 1/num_sublines  */
                      /*           over a key-line's own sub-lines and 0 elsewhere, the blocks back to back (image i at float     */
                      /*           offset sum_{j<i} K_j N_j).  Optional (NULL = not written); calls of up to 8 images -- the rows   */
                      /*           are written by extra blocks of the tokeniser's own launch                                  */
  const int32_t* h_cu_klines; /* HOST prefix sums [n_images+1] of key-lines per image; needed with `mat` when n_images > 1     */
} LinetrTokens;

/* ---- lifetime ------------------------------------------------------------------------------ */

int linetr_abi_version(void);
const char* linetr_last_error(void);

/* Replaces LineTransformer.__init__ + load_state_dict (models/line_transformer.py:203-223).
 * `names[i]` are state_dict keys, `h_data[i]` host float32 arrays of
 * `numel[i]` elements; integer buffers (num_batches_tracked) may be omitted or passed as NULL.
 * BatchNorm folding, head permutation and the CLS-query constants are derived here in float64
 * and uploaded once (weights stay resident in HBM/Infinity Cache). */
int linetr_create(const LinetrModelConfig* cfg, int32_t n_tensors, const char* const* names,
                  const float* const* h_data, const int64_t* numel, int32_t device,
                  LinetrHandle** out);
void linetr_destroy(LinetrHandle* h);

/* ---- host pre-filter ------------------------------------------------------------------------ */

/* change_cv2_T_np + remove_borders + filter_by_length (models/line_process.py:203-231, :59-84,
 * :6-21) on one image.  h_lines6 = [K,6] rows (startX,startY,endX,endY,lineLength,octave).
 * h_valid_mask: NULL (== the reference's non-ndarray mask, i.e. ignored) or [height,width] float64.
 * max_keylines follows the reference's slice semantics ([:max_keylines], so -1 drops the shortest).
 * Ties in length are ordered by descending original index (== a stable ascending argsort, reversed); linetr_prefilter_tied_images
 * reports them, for hosts that want NumPy's order instead.
 * Writes up to `capacity` records (first_sub/n_tok/n_sub/image filled as by linetr_pack_lines;
 * `sub_base` / `tok_base` = number of sub-lines / real tokens of the images that precede this one in the batch) and
 * returns K' in *k_out, the number of sub-lines of this image in *n_out.  LINETR_E_ASSERT if a token distance
 * exceeds the geometric line length (the reference's AssertionError, line_process.py:44-45).
 * Survivors are written straight into h_recs: on ANY error return the contents of h_recs are unspecified (the same holds
 * for linetr_prefilter_batch).
 * LINETR_E_ARG, before a line is read: K < 0, h_lines6 NULL with K > 0, a NULL k_out / n_out, a negative height, width, border,
 * capacity, sub_base or tok_base, h_recs NULL with capacity > 0, token_distance that is not > 0 (NaN included), max_tokens < 1.
 * A line with a NaN or infinite coordinate, length or octave fails remove_borders' / filter_by_length's comparisons the way it does
 * in the reference and is dropped; one whose length comes out infinite (an infinite lineLength, an octave beyond the exponent range)
 * and survives them is refused with LINETR_E_ARG (its token count is absurd), as is a batch of more than 2^31 - 1 sub-lines or tokens.
 * max_keylines may be any int32 (INT32_MIN: the slice [:-2^31], nothing survives). */
int linetr_prefilter(const double* h_lines6, int32_t K, int32_t height, int32_t width, int32_t border,
                     double min_length, int32_t max_keylines, const double* h_valid_mask,
                     double token_distance, int32_t max_tokens, int32_t image_index, int32_t sub_base,
                     int32_t tok_base, LinetrLineRec* h_recs, int32_t capacity, int32_t* k_out, int32_t* n_out);

/* linetr_prefilter for a whole batch in one call (images processed by up to `n_threads` host threads,
 * 0 = library default).  h_lines6 holds the [K_i,6] blocks of all images back to back, h_line_off [B+1]
 * their row offsets; h_valid_masks is NULL or an array of B (nullable) [height,width] float64 pointers.
 * Writes the records image-major into h_recs (may be pinned memory) and the prefix sums of surviving
 * key-lines / sub-lines into h_cu_k / h_cu_n [B+1].
 * LINETR_E_ARG as linetr_prefilter, and: n_images < 0, n_threads < 0, a NULL offset table or prefix-sum array, an offset table that
 * starts below 0 or decreases anywhere (image i owns rows h_line_off[i] .. h_line_off[i+1] of h_lines6; overlapping images cannot be
 * written in this form).  The table's last entry is the number of rows the call reads: the interface carries no other count of the
 * rows given, so a table that ends beyond the caller's array is the caller's to avoid, like any length. */
int linetr_prefilter_batch(const double* h_lines6, const int32_t* h_line_off, int32_t n_images, int32_t height,
                           int32_t width, int32_t border, double min_length, int32_t max_keylines,
                           const double* const* h_valid_masks, double token_distance, int32_t max_tokens,
                           int32_t n_threads, LinetrLineRec* h_recs, int32_t capacity, int32_t* h_cu_k,
                           int32_t* h_cu_n);

/* One image's settings for linetr_prefilter_ragged: what linetr_prefilter_batch takes once for the whole batch. */
typedef struct {
  int32_t height, width;       /* the image's own size in pixels                                                  */
  double min_length;           /* filter_by_length's bound for THIS image (auto_min_length: max(16, max(shape) / 40))   */
  double token_distance;       /* > 0; auto_min_length: max(8, max(shape) / 80)                                    */
  const double* valid_mask;    /* NULL, or this image's own [height][width] float64                                */
} LinetrPrefilterImage;        /* 32 bytes */

/* linetr_prefilter_batch for images of DIFFERENT sizes (the reference runs every image at its own size with --resize -1, and with
 * auto_min_length recomputes min_length and token_distance from each image's shape, models/matching.py:29-32,45-48): h_images [B]
 * gives every image its height, width, min_length, token_distance and valid mask; border, max_keylines, max_tokens, n_threads, the
 * outputs and the worker pool are linetr_prefilter_batch's.  Both entry points run the same per-image code: a table of B equal
 * entries gives linetr_prefilter_batch's bytes.
 * LINETR_E_ARG as linetr_prefilter_batch, with every table entry checked before a line is read, and: a NULL table with B > 0. */
int linetr_prefilter_ragged(const double* h_lines6, const int32_t* h_line_off, int32_t n_images,
                            const LinetrPrefilterImage* h_images, int32_t border, int32_t max_keylines, int32_t max_tokens,
                            int32_t n_threads, LinetrLineRec* h_recs, int32_t capacity, int32_t* h_cu_k, int32_t* h_cu_n);

/* Which images of the LAST linetr_prefilter / linetr_prefilter_batch / linetr_prefilter_ragged call on the calling thread had two candidates of EQUAL
 * length in front of the length sort (models/line_process.py:15-16): there the reference's order -- np.argsort, an unstable,
 * CPU-dispatched sort -- is whatever NumPy does on the host, and a tie across the [:max_keylines] cut even changes the set.
 * Writes up to `capacity` image indices (ascending; 0 for linetr_prefilter) and returns their number.  A host that has NumPy
 * re-orders exactly those images with it and re-packs them through linetr_pack_lines (linetr_amd/engine.py prefilter,
 * tie_order="numpy"), which makes the batched path identical by index to the reference on that machine; every other image
 * has a unique order. */
int32_t linetr_prefilter_tied_images(int32_t* h_images, int32_t capacity);

/* Same record packing for lines that were already filtered/sorted by the caller (the Python shim
 * keeps NumPy's own argsort so that tie order is the reference's on the same machine).
 * h_klines [K,2,2], h_length [K], h_angles [K,2] float64.
 * LINETR_E_ARG: K < 0, a NULL array with K > 0, a negative base, token_distance not > 0 (NaN included) or max_tokens < 1 (lines or no
 * lines), a length that is NaN, infinite or not positive, more than 2^31 - 1 sub-lines or tokens; LINETR_E_ASSERT as linetr_prefilter
 * (a NaN end point fails that comparison too). */
int linetr_pack_lines(const double* h_klines, const double* h_length, const double* h_angles, int32_t K,
                      double token_distance, int32_t max_tokens, int32_t image_index, int32_t sub_base,
                      int32_t tok_base, LinetrLineRec* h_recs, int32_t* n_out);

/* ---- device: tokenise ----------------------------------------------------------------------- */

/* Element type of a dense descriptor map, OR-ed into an entry point's `dense_is_nhwc` argument.  Without these bits the argument means
 * what it always meant: 0 = NCHW float32, any other value below 0x100 (a negative one too) = NHWC float32, with the alignment rules each
 * entry point states (a float32 NCHW map may lie anywhere).  LINETR_DENSE_F16: the map holds IEEE float16,
 * LINETR_DENSE_BF16: bfloat16; both bits together, or any higher bit, are refused with LINETR_E_ARG before anything is launched.  A half
 * map is read in place (no float32 copy): every element is converted exactly at the load (fp16 subnormals are kept) and all arithmetic
 * is the float32 call's, so the results equal those of the same call on the map's float32 upcast.  One call has ONE element type for all
 * its images.  A half NHWC map must be 8-byte aligned (a lane owns 4 channels); a half NCHW map may lie at any 2-byte address, its layout
 * pass transposes halves into a half scratch.  dense_score, token outputs and line descriptors are float32 always.
 * The bits are accepted by linetr_tokenize, linetr_sample_descriptors, linetr_point_descriptors, linetr_describe,
 * linetr_describe_ragged, linetr_describe_submit and linetr_debug_cls_pool (and by the size queries that take dense_is_nhwc: a half
 * format may need less, never more; a refused format gives the query's own "refused" answer).  Every other entry point that takes a
 * dense map (linetr_fixed_size) refuses them. */
#define LINETR_DENSE_F16 0x100
#define LINETR_DENSE_BF16 0x200

/* Bytes of scratch linetr_tokenize needs (NHWC copy of the dense descriptor maps + index maps). */
int64_t linetr_tokenize_workspace_bytes(int32_t n_images, int32_t height, int32_t width, int32_t N);

/* line_tokenizer + sample_descriptors + score gather (models/line_process.py:100-196, :86-98).
 * d_recs: [K] records of all images (image-major, per-image order preserved); h_recs the same
 * array on the host (used only to size launches).  d_dense_desc [B,256,height/8,width/8] NCHW
 * (dense_is_nhwc = 0, the reference's 'dense_descriptor') or [B,height/8,width/8,256] (dense_is_nhwc != 0, what
 * linetr_superpoint_heads emits: no layout pass), d_dense_score [B,height,width].  The end-point clip of line_process.py:114-116 is applied, and
 * the clipped end points are what `out.klines` holds (reference quirk: it mutates through a view).
 * d_sub2line [N] int32 (key-line index of every sub-line INSIDE ITS IMAGE, non-decreasing per image)
 * is written for linetr_match.  `out.desc` may be NULL to skip descriptor sampling.  `h` may be NULL (no weights are
 * involved; the current HIP device is used).  clip_height / clip_width: the `image_shape` ARGUMENT of line_tokenizer
 * (models/line_process.py:101), which only sets the end-point clip (:115-116) and need not be the maps' shape -- the dataset
 * builder passes (640, 480) for 480 x 640 images (dataloaders/utils/util_lines.py:682,703); <= 0 = height / width.
 * A channel-last d_dense_desc, out.desc and d_workspace are accessed with 16-byte vectors: one that is not 16-byte aligned is refused
 * with LINETR_E_ARG before anything is launched (linetr_describe / linetr_describe_submit: the same three). */
int linetr_tokenize(LinetrHandle* h, const LinetrLineRec* d_recs, int32_t K, int32_t N,
                    double token_distance, int32_t max_tokens, const void* d_dense_desc,
                    const float* d_dense_score, int32_t n_images, int32_t height, int32_t width,
                    int32_t clip_height, int32_t clip_width, int32_t align_corners, int32_t dense_is_nhwc,
                    LinetrTokens out, int32_t* d_sub2line, void* d_workspace, int64_t workspace_bytes, void* stream);

/* sample_descriptors (models/line_process.py:86-98) on its own, for the module-level function of the shim: n points
 * d_points [n,2] (x,y in pixels) of ONE image sampled bilinearly (zero padding) from its dense descriptor map
 * ([256,Hc,Wc], or [Hc,Wc,256] with dense_is_nhwc) and L2-normalised; d_out [n,256] row-major.  `h` may be NULL.
 * A channel-last map, d_out and d_workspace must be 16-byte aligned (LINETR_E_ARG otherwise; an NCHW map and d_points may lie anywhere). */
int64_t linetr_sample_descriptors_workspace_bytes(int32_t Hc, int32_t Wc, int32_t dense_is_nhwc);
int linetr_sample_descriptors(LinetrHandle* h, const float* d_points, int64_t n, const void* d_dense_desc, int32_t Hc,
                              int32_t Wc, int32_t align_corners, int32_t dense_is_nhwc, float* d_out, void* d_workspace,
                              int64_t workspace_bytes, void* stream);

/* ---- device: descriptor network ------------------------------------------------------------- */

int64_t linetr_forward_workspace_bytes(const LinetrHandle* h, int32_t N, int32_t max_tokens);

/* LineTransformer.forward (models/line_transformer.py:225-249) on a var-len batch.
 * h_cu_sub [B+1]: host prefix sums of sub-lines per image (signature attention is per image).
 * Inputs are the tokeniser tensors; mask is accepted for interface fidelity and ignored, because it
 * masks query rows only and the CLS row is never masked (models/line_attention.py:16).
 * d_cu_sub: the same array already on the device, or NULL (the library then copies h_cu_sub itself).
 * d_line_desc [N,256] row-major (the shim exposes the reference's [1,256,N] as a transposed view). */
int linetr_forward(LinetrHandle* h, const LinetrTokens* tok, const int32_t* h_cu_sub, const int32_t* d_cu_sub,
                   int32_t n_images, int32_t max_tokens, float* d_line_desc, void* d_workspace,
                   int64_t workspace_bytes, void* stream);

/* ---- device: fused tokenise + describe (batched fast path) ---------------------------------------- */

/* Training-time forward (train.py:127,163-164: model.train(); pred = model(data) on a batch of B fixed-size samples): the same
 * network as linetr_forward with every BatchNorm1d of the three MLP stacks (models/line_transformer.py:9-20: 4 in
 * WordPositionalEncoder, 4 in LinePositionalEncoder, 1 per AttentionalPropagation) in TRAINING mode -- normalised with the mean and
 * biased variance of this batch (over all B*N*T token positions / B*N sub-lines), running statistics moved by `momentum` towards
 * the batch mean / UNBIASED variance.  Dropout (models/line_attention.py:11,39,84) is taken at probability 0: the caller has to
 * make sure of that (the Python surface refuses otherwise); no gradients are produced.
 * `h` must have been created with bn_batch_stats = 1.  The images of the batch are the n_images entries of h_cu_sub, as in
 * linetr_forward.  d_bn_running (in/out) and d_bn_batch (out, may be NULL) are packed per BatchNorm layer in THIS order --
 * klenc.word_position_enc.encoder.{1,4,7,10} | klenc.line_position_enc.encoder.{1,4,7,10} | selfattn.layers.l.mlp.1 (l = 0 ..) --
 * (note: the state_dict lists the line encoder first), each layer as mean[C] | var[C]; d_bn_batch
 * receives the batch mean | biased variance.  linetr_bn_stats_floats() = the length of both arrays. */
int64_t linetr_bn_stats_floats(const LinetrHandle* h);
int64_t linetr_forward_train_workspace_bytes(const LinetrHandle* h, int32_t N, int32_t max_tokens);
int linetr_forward_train(LinetrHandle* h, const LinetrTokens* tok, const int32_t* h_cu_sub, const int32_t* d_cu_sub,
                         int32_t n_images, int32_t max_tokens, float momentum, float* d_bn_running, float* d_bn_batch,
                         float* d_line_desc, void* d_workspace, int64_t workspace_bytes, void* stream);

int64_t linetr_describe_workspace_bytes(const LinetrHandle* h, int32_t n_images, int32_t height, int32_t width,
                                        int32_t N, int64_t n_real_tokens);

/* preprocess + forward of LineTransformer (models/line_transformer.py:251-275 + :225-249) for a batch in one
 * call, without materialising the [N,T,256] token descriptors: the word-position MLP runs on the REAL tokens
 * only (n_real_tokens = sum of n_tok over d_recs, plus one shared zero-padding token per image -- every padded
 * slot of an image holds the same coordinate (0,0), hence the same descriptor, score and key/value), and the
 * CLS-row attention pooling samples the NHWC descriptor map on the fly, counting the padding token with its
 * multiplicity.  Results equal linetr_tokenize + linetr_forward up to fp32 rounding.
 * dense_is_nhwc != 0: d_dense_desc is already [B, H/8, W/8, 256] (a producer that emits channel-last, e.g. a fused
 * SuperPoint descriptor head) and the NCHW->NHWC copy is skipped.
 * Small tokeniser outputs (klines, length, angles, sublines, resp, angle_sub) are written when their pointers in
 * `out` are non-NULL; pnt / mask / score / desc are written only if non-NULL (dense [N,T,...] layout). */
int linetr_describe(LinetrHandle* h, const LinetrLineRec* d_recs, int32_t K, int32_t N, int64_t n_real_tokens,
                    const int32_t* h_cu_sub, const int32_t* d_cu_sub, int32_t n_images, double token_distance,
                    int32_t max_tokens, const void* d_dense_desc, const float* d_dense_score, int32_t height,
                    int32_t width, int32_t align_corners, int32_t dense_is_nhwc, LinetrTokens out,
                    int32_t* d_sub2line, float* d_line_desc, void* d_workspace, int64_t workspace_bytes,
                    void* stream);

/* One image of a linetr_describe_ragged batch: its own maps, size and token distance.  The maps are separate allocations; nothing
 * requires the caller to pack them. */
typedef struct {
  const void* d_dense_desc;    /* [256,height/8,width/8] (dense_is_nhwc = 0) or [height/8,width/8,256]; device memory */
  const float* d_dense_score;  /* [height,width]; device memory                                                        */
  int32_t height, width;       /* positive multiples of 8                                                              */
  double token_distance;       /* > 0 (auto_min_length: max(8, max(shape) / 80) of THIS image)                         */
} LinetrImage;                 /* 32 bytes */

/* linetr_describe for a batch whose images differ in size (the reference has no size restriction: match_line_pairs.py --resize -1
 * runs every image at its own size, and models/matching.py:29-32,45-48 recompute token_distance per image).  linetr_describe's
 * arguments with (d_dense_desc, d_dense_score, height, width, token_distance) replaced by the HOST table h_images [n_images], which
 * may be pageable and is not read after the call returns: the library builds its device-side table in the workspace.  The records
 * come from linetr_prefilter_ragged (or linetr_pack_lines per image) with the same token distances; the end-point clip of image i is
 * (width_i - 0.6, height_i - 0.6).  h_recs: the records on the host as well, or NULL -- with it, every record's `image` is checked
 * against the table before anything is launched (the kernels index the table with it; d_recs alone cannot be checked without a
 * device round trip).  NULL means NO check: a record of d_recs whose image is not in 0 .. n_images - 1 then makes the kernels read
 * beyond the table, which is undefined behaviour -- pass NULL only for records whose images the caller vouches for.  All LinetrTokens outputs are supported, `mat` for up to 8 images as in linetr_describe.  Asynchronous on
 * `stream`; no device allocation (the table travels through a pinned staging ring the library keeps).  Everything behind the CLS
 * pooling is linetr_describe's own code: a table of equal entries gives its results bit for bit.
 * LINETR_E_ARG before any launch: a NULL or empty table; a height or width that is not a positive multiple of 8; a NULL map; a
 * channel-last map, out.desc or workspace that is not 16-byte aligned; a token_distance that is not > 0; a record of h_recs whose
 * image lies outside the table; and what linetr_describe refuses.  LINETR_E_WORKSPACE: a workspace below the query's answer.
 * linetr_describe_ragged_workspace_bytes returns -1 for a table the call would refuse. */
int64_t linetr_describe_ragged_workspace_bytes(const LinetrHandle* h, const LinetrImage* h_images, int32_t n_images,
                                               int32_t dense_is_nhwc, int32_t N, int64_t n_real_tokens);
int linetr_describe_ragged(LinetrHandle* h, const LinetrLineRec* d_recs, const LinetrLineRec* h_recs, int32_t K, int32_t N,
                           int64_t n_real_tokens, const int32_t* h_cu_sub, const int32_t* d_cu_sub, const LinetrImage* h_images,
                           int32_t n_images, int32_t max_tokens, int32_t align_corners, int32_t dense_is_nhwc, LinetrTokens out,
                           int32_t* d_sub2line, float* d_line_desc, void* d_workspace, int64_t workspace_bytes, void* stream);

/* linetr_describe as a software pipeline over CONSECUTIVE batches ("batch/varlen plumbing + stream
 * pipelining"; the reference is serial per pair, models/matching.py:34-60).  A batch is cut into stages at fixed points of the network
 * -- e.g. front = layout pass, tokeniser, positional-encoder MLPs, CLS pooling, descriptive-layer tail (HBM-bound for half of its
 * time); back = the line-signature network (MFMA-bound, launches whose tile rounds leave CUs empty) -- and stage k of every batch is
 * queued on the k-th of a set of library-owned streams, so stage k of batch i + 1 runs under stage k + 1 of batch i.  Every GEMM still
 * sees the FULL batch (nothing is split), and the results are bit-identical to linetr_describe's: the same kernels on the same data.
 *   linetr_describe_submit  same arguments as linetr_describe + slot and n_slots: the caller keeps n_slots (2 .. linetr_pipeline_max_slots())
 *                           batches in flight and gives batch i the slot i mod n_slots.  The work starts behind everything already
 *                           queued on `stream` (the upload of d_recs, the producer of the dense maps) and is NOT joined back: `stream`
 *                           does not wait for it.  Every slot needs its OWN d_workspace and output buffers, alive until the slot is
 *                           joined.  Host run-ahead is bounded: a submit first waits (on the host) for the batch previously submitted
 *                           to the same slot.
 *   linetr_describe_join    `stream` waits for the batch last submitted to `slot`; its outputs may be read on `stream` afterwards.
 * A caller pipelines by  submit(i, i mod n);  join(i - n + 1, (i - n + 1) mod n);  -- n - 1 batches of latency for the overlap.
 * Like every entry point that takes a handle, the pair is not re-entrant: one submitting thread per handle.  A failed submit leaves
 * the library's streams idle and the slot free (nothing half-queued survives it). */
int linetr_describe_submit(LinetrHandle* h, const LinetrLineRec* d_recs, int32_t K, int32_t N, int64_t n_real_tokens,
                           const int32_t* h_cu_sub, const int32_t* d_cu_sub, int32_t n_images, double token_distance,
                           int32_t max_tokens, const void* d_dense_desc, const float* d_dense_score, int32_t height,
                           int32_t width, int32_t align_corners, int32_t dense_is_nhwc, LinetrTokens out,
                           int32_t* d_sub2line, float* d_line_desc, void* d_workspace, int64_t workspace_bytes,
                           int32_t slot, int32_t n_slots, void* stream);
int32_t linetr_pipeline_max_slots(void);
int linetr_describe_join(LinetrHandle* h, int32_t slot, void* stream);

/* ---- device: matcher ------------------------------------------------------------------------ */

int64_t linetr_match_workspace_bytes(int32_t n_pairs, int64_t sum_n0n1, int64_t sum_k0k1, int64_t sum_k);

/* get_dist_matrix + subline2keyline + nn_matcher_distmat (models/line_process.py:198-201,
 * models/line_transformer.py:277-282, models/nn_matcher.py:3-31) for P pairs in one launch set.
 * Pair p uses descriptors d_desc0[h_off_n0[p] .. +n0) (rows of 256) and key-line maps
 * d_sub2line0 (LOCAL key-line index per sub-line, non-decreasing), same for side 1.
 * h_dims [P,4] = (n0,k0,n1,k1); offsets are host int64 arrays [P].
 * Outputs: d_dk at h_off_dk[p] holds Dk [k0,k1] float32; d_match01 at h_off_k0[p] holds, per
 * key-line of image 0, the matched key-line of image 1 or -1 (the non-zero of the reference's 0/1
 * matrix; first-index argmin, strict `<`, optional mutual check). */
int linetr_match(LinetrHandle* h, int32_t n_pairs, const int32_t* h_dims, const float* d_desc0,
                 const int64_t* h_off_n0, const int32_t* d_sub2line0, const float* d_desc1,
                 const int64_t* h_off_n1, const int32_t* d_sub2line1, float nn_thresh, int32_t mutual,
                 float* d_dk, const int64_t* h_off_dk, int32_t* d_match01, const int64_t* h_off_k0,
                 void* d_workspace, int64_t workspace_bytes, void* stream);

/* linetr_match with separate offsets for the key-line maps: pair p reads its descriptors at row h_off_n0[p] of d_desc0
 * and its sub-line -> key-line map at element h_off_s0[p] of d_sub2line0 (same for side 1; NULL offsets = h_off_n*).
 * This is the form global matching uses after the multi-GPU all-gather, where descriptors and maps of all ranks sit
 * at different places of ONE gathered buffer (linetr_amd/parallel.py; no reference counterpart, BASELINE.json cfg4). */
int linetr_match_gathered(LinetrHandle* h, int32_t n_pairs, const int32_t* h_dims, const float* d_desc0,
                          const int64_t* h_off_n0, const int32_t* d_sub2line0, const int64_t* h_off_s0,
                          const float* d_desc1, const int64_t* h_off_n1, const int32_t* d_sub2line1,
                          const int64_t* h_off_s1, float nn_thresh, int32_t mutual, float* d_dk,
                          const int64_t* h_off_dk, int32_t* d_match01, const int64_t* h_off_k0, void* d_workspace,
                          int64_t workspace_bytes, void* stream);

/* nn_matcher_distmat (models/nn_matcher.py:3-31) on a distance matrix that already lives on the device:
 * d_dist [n0,n1] float32 -> d_match01 [n0] (index into side 1 or -1).  `h` may be NULL for the three
 * matcher entry points (they need no weights); the current HIP device is used then.
 * Contract: distances are float32 and NaN-free (the reference's cosine distances are clipped to [0,4]); a NaN entry
 * is skipped by the argmin here, whereas np.argmin would return it.  All three matcher entry points are fully
 * asynchronous on `stream` (host tables are staged in a library-owned pinned ring). */
int64_t linetr_match_distmat_workspace_bytes(int32_t n0, int32_t n1);
int linetr_match_distmat(LinetrHandle* h, const float* d_dist, int32_t n0, int32_t n1, float nn_thresh,
                         int32_t mutual, int32_t* d_match01, void* d_workspace, int64_t workspace_bytes,
                         void* stream);

/* nn_matcher_distmat (models/nn_matcher.py:3-31) on a float64 device matrix d_dist [n0,n1], compared in float64 the way NumPy
 * compares a float64 matrix (the reference's own caller passes float32: linetr_match_distmat).  nn_thresh is a double.  `h` may
 * be NULL; asynchronous on `stream`. */
int64_t linetr_match_distmat_f64_workspace_bytes(int32_t n0, int32_t n1);
int linetr_match_distmat_f64(LinetrHandle* h, const double* d_dist, int32_t n0, int32_t n1, double nn_thresh, int32_t mutual,
                             int32_t* d_match01, void* d_workspace, int64_t workspace_bytes, void* stream);

/* LineTransformer.subline2keyline (models/line_transformer.py:277-282) alone: Dk [k0,k1] = A0 D A1^T for a sub-line distance
 * matrix d_dist [n0,n1] that already lives on the device, the two mat_klines2sublines given as the sub-line -> key-line maps
 * linetr_tokenize writes (non-decreasing; rows of A are 1/num_sublines).  `h` may be NULL.  Asynchronous on `stream`. */
int64_t linetr_pool_distmat_workspace_bytes(int32_t k0, int32_t k1);
int linetr_pool_distmat(LinetrHandle* h, const float* d_dist, int32_t n0, int32_t n1, const int32_t* d_sub2line0, int32_t k0,
                        const int32_t* d_sub2line1, int32_t k1, float* d_dk, void* d_workspace, int64_t workspace_bytes,
                        void* stream);

/* LineTransformer.subline2keyline (models/line_transformer.py:277-282) on the two mat_klines2sublines MATRICES, the way the
 * reference's call sites pass them (models/matching.py:80: data['mat_klines2sublines0'][0], [K,N] float32 on the device): a matrix
 * of the form line_tokenizer writes (models/line_process.py:163-167: one non-zero per column, key-lines in order, rows of
 * float32(1 / num_sublines)) is reduced to its sub-line -> key-line map on the device and pooled like linetr_pool_distmat;
 * any other matrix is multiplied out as given, Dk = (A0 D) A1^T in fp32.  The decision is made on the device: asynchronous on
 * `stream`, no host synchronisation.  `h` may be NULL.
 * The verdict: once the call's work on `stream` has completed, the first int32 of d_workspace holds the word the decision was
 * taken by (0: both matrices were pooled by their maps; anything else: multiplied out as given).  Per matrix, with map[n] the
 * LAST row that is non-zero in column n (0 for an empty column; NaN counts as non-zero, -0 as zero) and val[n] that entry, the bits are
 *   1  a column without exactly one non-zero;
 *   2  rows not in order (map[0] != 0, a step of map other than 0 or +1, map[N-1] != K-1: a key-line without sub-lines);
 *   4  a val[n] that is not float32(1 / num_sublines) (a float64 quotient rounded once), num_sublines the length of the run of
 *      equal map values that n belongs to;
 * the bits of A0 and A1 are ORed.  The word is preset to 1 when k0 > n0 or k1 > n1 (nothing is inspected then) and is NOT written
 * when an inner dimension is 0 (the result is a zero matrix) or an outer one is (nothing is done). */
int64_t linetr_pool_distmat_dense_workspace_bytes(int32_t k0, int32_t n0, int32_t k1, int32_t n1);
int linetr_pool_distmat_dense(LinetrHandle* h, const float* d_dist, int32_t n0, int32_t n1, const float* d_A0, int32_t k0,
                              const float* d_A1, int32_t k1, float* d_dk, void* d_workspace, int64_t workspace_bytes,
                              void* stream);

/* nn_matcher (models/nn_matcher.py:33-42): point-descriptor variant, desc given [256,n] column-major
 * like SuperPoint's `descriptors` -- section 8(f) "next" row, same kernels.  `h` may be NULL (the current device is used).
 * d_workspace: linetr_match_points_workspace_bytes(n0, n1) bytes (negative counts count as 0); a smaller one is refused with
 * LINETR_E_WORKSPACE before anything is launched. */
int64_t linetr_match_points_workspace_bytes(int32_t n0, int32_t n1);
int linetr_match_points(LinetrHandle* h, const float* d_desc0_cn, int32_t n0, const float* d_desc1_cn,
                        int32_t n1, float nn_thresh, int32_t mutual, float* d_dist, int32_t* d_match01,
                        void* d_workspace, int64_t workspace_bytes, void* stream);

/* The matching tail of Matching.forward (models/matching.py:67-84) in ONE call: the point matcher on the two [256,n] SuperPoint
 * descriptor sets (nn_matcher, models/nn_matcher.py:33-42), the line matcher on the two images' line descriptors (get_dist_matrix +
 * subline2keyline + nn_matcher_distmat) and the device -> host copies of the four results into ONE caller-provided PINNED host block,
 * everything asynchronous on `stream` (the caller waits for the stream / an event once).  Either branch is skipped when its sizes are
 * 0.  linetr_pair_tail_output_bytes returns the size of the block and the byte offsets of its four segments:
 *   h_offsets[0] point distances [np0][np1] float32, [1] point match01 [np0] int32, [2] Dk [k0][k1] float32, [3] line match01 [k0] int32. */
int64_t linetr_pair_tail_workspace_bytes(int32_t np0, int32_t np1, int32_t n0, int32_t k0, int32_t n1, int32_t k1);
int64_t linetr_pair_tail_output_bytes(int32_t np0, int32_t np1, int32_t k0, int32_t k1, int64_t* h_offsets);
int linetr_pair_tail(LinetrHandle* h, const float* d_pdesc0_cn, int32_t np0, const float* d_pdesc1_cn, int32_t np1, float nn_thresh_points,
                     const float* d_ldesc0, int32_t n0, const int32_t* d_sub2line0, int32_t k0, const float* d_ldesc1, int32_t n1,
                     const int32_t* d_sub2line1, int32_t k1, float nn_thresh_lines, int32_t mutual, void* h_pinned_out,
                     int64_t pinned_bytes, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- validation step (section 8(f) "next" row 4: loss forward + evaluation) ------------------------- */

/* What the reference's `val` epoch computes after the batched forward (train.py:198-240), on the device and forward only:
 *   evaluations/criteria.py:59-124,173-192   descriptor_loss: D = 2 - 2 <d0, d1> (no clip); 2n anchor rows per item (the n rows of D, then
 *       the n rows of D^T); pos = max(0, max of D over the row's entries with assign > 0.3), an anchor where pos > 0; neg = the smallest D
 *       among the row's entries with assign <= 0 that has pos < D < pos + 0.5 (both strict, pos + 0.5 in float32; every other entry counts
 *       as 10000); an anchor without one is dropped; loss = mean over the V anchors left of relu(pos - neg + 1), hardest_positive = max
 *       pos, hardest_negative = min neg.  V == 0 is no error here: loss and both hardest values are NaN, the count 0.
 *   evaluations/matcher.py:51-102            nn_matcher_batches: score = max((|d0|^2 + |d1|^2) - 2 <d0, d1>, 0) in float32 with the norms
 *       recomputed, first-index row argmin, score < nn_thresh (strict, compared in float64), optional mutual check against the
 *       first-index column argmin: match01 [B][n], -1 = no match.
 *   evaluations/evaluate_pr.py:10-35         per item TP, FP, FN, TN (ground truth assign > 0) and precision, recall, f1 in float64.
 * Both formulas read ONE set of dot products (exact-fp32 MFMA); every reduction has a fixed order.  Three launches and one copy.
 *   d_desc0 / d_desc1  [B*n][256] row-major as linetr_forward* writes them: item b owns rows b*n .. b*n + n - 1
 *   d_assign           [B][n+1][n+1] float32, the reference's target['mat_assign_sublines'] (dustbin row / column not read)
 *   d_row_pos / d_row_neg  [B][2n] float32 or NULL: pos of every anchor row; neg, or -1 where the row is no anchor or was dropped.
 *       row_pos is max(0, .): where every column of a row is a match the reference's amax can be slightly negative (n = 1 with
 *       rounding); such a row is no anchor either way, but this array holds 0 there, never a negative value
 *   d_match01          [B][n] int32 or NULL
 *   h_pinned_out       PINNED host block of linetr_val_step_output_bytes(B, h_offsets) bytes, filled by one asynchronous copy:
 *       h_offsets[0] float64 [3] loss, hardest_positive, hardest_negative   [1] int64 [1] V
 *       h_offsets[2] int32 [B][4] TP, FP, FN, TN                            [3] float64 [B][3] precision, recall, f1
 * Asynchronous on `stream`; `h` may be NULL.  n0 != n1 (the criterion concatenates D and D^T), B <= 0, n <= 0, a NULL required pointer,
 * an output block or a workspace smaller than the two functions below say: LINETR_E_ARG, nothing launched. */
int64_t linetr_val_step_workspace_bytes(int32_t B, int32_t n);
int64_t linetr_val_step_output_bytes(int32_t B, int64_t* h_offsets);
int linetr_val_step(LinetrHandle* h, const float* d_desc0, int32_t n0, const float* d_desc1, int32_t n1, const float* d_assign, int32_t B,
                    double nn_thresh, int32_t mutual, float* d_row_pos, float* d_row_neg, int32_t* d_match01, void* h_pinned_out,
                    int64_t pinned_bytes, void* d_workspace, int64_t workspace_bytes, void* stream);

/* train.py:176-183: d_assign [B][n+1][n+1] float32 = 0, then 1 at (d_lmatches[b][m][0], d_lmatches[b][m][1]) for every row m of the
 * loader's int32 [B][M][2] match list whose first entry is not -1 (an index outside 0..n is skipped).  B, n as above, M >= 0 and B * M <= 2^31 * 256, else LINETR_E_ARG.  Asynchronous; `h` may be NULL. */
int linetr_assign_from_matches(LinetrHandle* h, const int32_t* d_lmatches, int32_t B, int32_t M, int32_t n, float* d_assign, void* stream);

/* ---- gradient of the criterion (section 8(f) "next" row 4: the first link of the backward) ---------------- */

/* descriptor_loss above, differentiated as torch autograd differentiates the reference's (evaluations/criteria.py:59-124,173-192): the
 * loss scalars of linetr_val_step (bit-identical on the same inputs) AND d loss / d line_desc0, d loss / d line_desc1, from one selection.
 *   w = upstream / V.  Every surviving anchor row (pos - neg + 1 > 0, which the semi-hard window guarantees) gives dD the weight
 *   +w / ties at each of the `ties` entries with assign > 0.3 whose D equals its pos (amax's backward splits evenly) and -w at its negative,
 *   the FIRST index of the smallest semi-hard entry (argmin, then indexing).  An entry that a row anchor and a column anchor both select
 *   receives the sum.  With D = 2 - 2 <d0[a], d1[c]>:   grad0[a] = -2 sum_c dD[a][c] d1[c],   grad1[c] = -2 sum_a dD[a][c] d0[a].
 * dD is gathered tile by tile on the chip and never stored; no floating-point atomics, every reduction has a fixed order: two calls give
 * the same bits.  Four launches and one copy.
 *   d_desc0 / d_desc1, d_assign   as linetr_val_step reads them (descriptors 16-byte aligned)
 *   d_upstream         one float32 on the device, the gradient arriving at the loss; NULL = 1
 *   d_grad0 / d_grad1  [B*n][256] float32, 16-byte aligned, either may be NULL.  EVERY row is written, zeros included; V == 0: all zero
 *   h_pinned_out       PINNED host block of at least 32 bytes, filled by one asynchronous copy:
 *       float64 [3] loss, hardest_positive, hardest_negative (NaN when V == 0) | int64 [1] V
 * Asynchronous on `stream`; nothing inside allocates or waits; `h` may be NULL.  n0 != n1, B <= 0, n <= 0 (or beyond 65535 items / 32768
 * sub-lines), a NULL required pointer, an output block shorter than 32 bytes or a workspace smaller than
 * linetr_desc_loss_grad_workspace_bytes says: LINETR_E_ARG, nothing launched. */
int64_t linetr_desc_loss_grad_workspace_bytes(int32_t B, int32_t n);
int linetr_desc_loss_grad(LinetrHandle* h, const float* d_desc0, int32_t n0, const float* d_desc1, int32_t n1, const float* d_assign,
                          int32_t B, const float* d_upstream, float* d_grad0, float* d_grad1, void* h_pinned_out, int64_t pinned_bytes,
                          void* d_workspace, int64_t workspace_bytes, void* stream);

/* The reference's second criterion, descriptor_loss.compute_distances_hardnet (evaluations/criteria.py:126-171; its call site is the
 * commented line of forward, :175-176): HardNet mining, value and gradient as torch autograd differentiates it, from one selection.
 * Per item, with D[a][c] = 2 - 2 <d0[a], d1[c]> (float32, not clipped), match = assign > 0.3, unmatch = assign <= 0 on the [n][n] part
 * (an entry in (0, 0.3] is neither; the dustbin row and column are not read) and cand = unmatch ? D : 10000:
 *   rowmin[a] = min_c cand[a][c], colmin[c] = min_a cand[a][c].  There are 2n anchor lines: the n rows of D, then its n columns.
 *   For a line r: pos_r = max(0, largest matched D on the line); it is an anchor iff pos_r > 0; p_r is the FIRST index attaining pos_r
 *   (torch.max(dim)).  neg_r = min(own, cross): a row anchor a has own = rowmin[a], cross = colmin[p]; a column anchor c has
 *   own = colmin[c], cross = rowmin[p].  No anchor is ever dropped: a line without an unmatched entry on either side has neg = 10000.
 *   loss = mean over the V anchors of relu(pos - neg + 1), hardest_positive = max pos, hardest_negative = min neg (may be 10000),
 *   reduced in a fixed order in float64.  V == 0: the three are NaN.  n = 1 with a match: loss 0, hardest_negative 10000, gradients zero.
 * Gradient, w = upstream / V.  An anchor is live iff pos - neg + 1 > 0 (strict: relu'(0) = 0).  A live anchor gives +w to its positive
 * entry at index p_r ONLY (nothing is split over tied positives).  Its -w goes to the own line if own < cross, to the cross line if
 * own > cross, w / 2 to each if they are equal (the element-wise torch.min); on the chosen line the share is divided evenly over every
 * unmatched entry equal to the minimum (amin's backward); entries valued 10000 carry nothing.  An entry of D collects the sum of what
 * row anchors and column anchors give it.  grad0[a] = -2 sum_c G[a][c] d1[c],   grad1[c] = -2 sum_a G[a][c] d0[a].
 * G is gathered tile by tile on the chip and never stored; no floating-point atomics, every reduction has a fixed order: two calls give
 * the same bits.  Five launches and one copy; four when both gradients are NULL (the value-only call: the same scalars, bit for bit).
 *   d_desc0 / d_desc1, d_assign, d_upstream, d_grad0 / d_grad1   as linetr_desc_loss_grad documents them; EVERY gradient row is
 *       written and zeros are +0
 *   d_row_pos / d_row_neg  [B][2n] float32 or NULL: pos of every line; neg, or -1 where the line is no anchor
 *   d_row_arg          [B][2n] int32 or NULL: the positive's index along the line, or -1 where the line is no anchor
 *   h_pinned_out       PINNED host block of at least 40 bytes, filled by one asynchronous copy:
 *       float64 [3] loss, hardest_positive, hardest_negative | int64 [2] V, the number of live anchors
 * Asynchronous on `stream`; nothing inside allocates or waits; `h` may be NULL.  n0 != n1, B <= 0, n <= 0 (or beyond 65535 items / 32768
 * sub-lines), a NULL required pointer, an output block shorter than 40 bytes or a workspace smaller than
 * linetr_hardnet_loss_grad_workspace_bytes says: LINETR_E_ARG, nothing launched. */
int64_t linetr_hardnet_loss_grad_workspace_bytes(int32_t B, int32_t n);
int linetr_hardnet_loss_grad(LinetrHandle* h, const float* d_desc0, int32_t n0, const float* d_desc1, int32_t n1,
                             const float* d_assign, int32_t B, const float* d_upstream, float* d_grad0, float* d_grad1,
                             float* d_row_pos, float* d_row_neg, int32_t* d_row_arg,
                             void* h_pinned_out, int64_t pinned_bytes, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- backward of the 1x1 layers and the descriptor head (section 8(f) "next" row 4: the second link) ---------- */

/* A point-wise linear layer, Conv1d(k=1) or Linear, on the UNFOLDED state_dict weight:  Y = act(X W^T + b)  and its backward, as torch
 * autograd differentiates F.conv1d / F.linear (+ F.relu):
 *   G' = G, zeroed where d_mask <= 0 (d_mask: the layer's own post-ReLU output, handed in by the caller; NULL: no activation)
 *   dX [rows][K] = G' W        dW [N][K] = G'^T X        db [N] = column sums of G'
 * rows = B n positions; activations are row-major [rows][C] with a row stride (the layout linetr_forward* writes).  Every contraction
 * is exact-fp32 MFMA (no split).  dW / db: the rows are cut into chunks of linetr_linear_backward_chunk_rows() rows (a compile-time
 * constant), every (chunk, tile) partial goes to the workspace and the chunks are added in ascending order: no floating-point atomics,
 * every output element written, two calls give the same bits.  Rows beyond `rows` are neither loaded nor stored.
 *   d_x [rows][ldx]   d_W [N][K]   d_b [N] or NULL   d_y [rows][ldy]   act: 0 none, 1 ReLU
 *   d_g, d_mask [rows][ldg] (d_mask may be NULL)   d_dx [rows][ldx], d_dW [N][K], d_db [N]: each may be NULL (not computed then)
 * Asynchronous on `stream`; nothing inside allocates or waits; `h` may be NULL.  LINETR_E_ARG, nothing launched: rows < 1 (or beyond
 * 2^30), N % 64 != 0, K % 32 != 0, N or K beyond 1024, act outside 0 .. 1, a row stride below the width or no multiple of 4 floats, a
 * pointer that is not 16-byte aligned, a NULL required pointer (d_x, d_W, d_y; d_g, the workspace when d_dW or d_db is asked for),
 * a workspace smaller than linetr_linear_backward_workspace_bytes says. */
int32_t linetr_linear_backward_chunk_rows(void);
int64_t linetr_linear_backward_workspace_bytes(int64_t rows, int32_t N, int32_t K);
int linetr_linear_forward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_W, const float* d_b, int64_t rows, int32_t N,
                          int32_t K, int32_t act, float* d_y, int64_t ldy, void* stream);
int linetr_linear_backward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_W, const float* d_g, int64_t ldg,
                           const float* d_mask, int64_t rows, int32_t N, int32_t K, float* d_dx, float* d_dW, float* d_db,
                           void* d_workspace, int64_t workspace_bytes, void* stream);

/* The descriptor head, models/line_transformer.py:245-246:  line_desc = F.normalize(final_proj(x), p=2, dim=1), on rows:
 *   y = x W^T + b (256 -> 256)      d = y / max(|y|_2, 1e-12)
 * and its backward as torch autograd differentiates it:  gy = (g - d (d . g)) / max(|y|, 1e-12) where |y| >= 1e-12, g / 1e-12 elsewhere
 * (clamp_min passes no gradient to the norm there); then dx = gy W, dW = gy^T x, db = column sums of gy as above.  y is recomputed in
 * the backward and never stored; gy [rows][256] lives at the start of the workspace.  Three kernels forward + backward of the layer.
 *   d_x, d_g, d_desc, d_dx [rows][256] contiguous   d_W [256][256]   d_b [256]   d_dx / d_dW / d_db: each may be NULL
 * Asynchronous; `h` may be NULL.  The refusals of the layer above (d_b is required here). */
int64_t linetr_head_backward_workspace_bytes(int64_t rows);
int linetr_head_forward(LinetrHandle* h, const float* d_x, const float* d_W, const float* d_b, int64_t rows, float* d_desc, void* stream);
int linetr_head_backward(LinetrHandle* h, const float* d_x, const float* d_W, const float* d_b, const float* d_g, int64_t rows,
                         float* d_dx, float* d_dW, float* d_db, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- neighbour-line attention for training (section 8(f) "next" row 4: the third link) ---------- */

/* The attention of the signature network, models/line_transformer.py:132-136 of the reference, per image and head on the library's
 * head-major rows (column c = h*64 + d), forward with the softmax statistics and backward as torch autograd differentiates it:
 *   S = (q / 8) k^T      m = row max of S      l = row sum of exp(S - m)      msg = exp(S - m) v / l      lse = m + logf(l)
 *   delta[r][h] = sum_d dO[r][h][d] msg[r][h][d]        P = exp(S - lse)        dV = P^T dO        dP = dO V^T
 *   dS = P * (dP - delta)        dK = dS^T (q / 8)        dQ = (dS K) / 8
 * q is UNSCALED at this interface: the kernels multiply by 1/8 on load (a power of two, exact), and the forward's message has the bits of
 * linetr_debug_sig_attention's kernel 0 on pre-scaled q.  Every contraction is exact-fp32 MFMA (no split), natural-log scores and expf.
 * Flash-style: P is recomputed from q, k and lse and nothing n x n reaches memory; delta [N][4] lives at the start of the workspace.
 *   d_q, d_k, d_v, d_msg, d_g (= dO), d_dq, d_dk, d_dv   [N][256 of ld*] float32, each with a row stride of its own: q | k | v may be three
 *                      column blocks of one [N][768] buffer (ldq = ldk = ldv = 768), the layout the forward pass writes
 *   d_lse              [N][4] float32, contiguous
 *   d_cu_sub           [n_images + 1] int32 ON THE DEVICE, ascending, d_cu_sub[0] = 0 and d_cu_sub[n_images] = N: one image is one softmax
 *                      domain.  Images of 0 sub-lines are legal and cost nothing; image sizes are unbounded; n_images <= 4096 (every
 *                      block finds its image by walking d_cu_sub, so that no size has to be known on the host)
 *   d_dq, d_dk, d_dv   each may be NULL and is then not computed (what is computed has the same bits either way)
 * Deterministic: no floating-point atomics; every output row is written exactly once, by the block that owns it, and every sum has a
 * fixed order (ascending chunks of 32 rows of the other side, each an MFMA chain of its own): two calls give the same bits.  Rows and
 * columns beyond an image are neither loaded into a sum nor stored.  Forward: one launch; backward: three (delta, dK / dV, dQ).
 * Asynchronous on `stream`; nothing inside allocates or waits; `h` may be NULL.  LINETR_E_ARG, nothing launched: a NULL required pointer
 * (forward: all of them; backward: d_q, d_k, d_v, d_msg, d_lse, d_g, d_cu_sub, the workspace), a row stride below 256 or no multiple of 4
 * floats (the stride of a NULL output is not read), a pointer that is not 16-byte aligned, n_images < 1 (or beyond 4096), N < 0 (or beyond 2^31 - 1), a
 * workspace smaller than linetr_sig_attention_backward_workspace_bytes(N) says. */
int64_t linetr_sig_attention_backward_workspace_bytes(int64_t N);
int linetr_sig_attention_forward(LinetrHandle* h, const float* d_q, int64_t ldq, const float* d_k, int64_t ldk, const float* d_v, int64_t ldv,
                                 const int32_t* d_cu_sub, int32_t n_images, int64_t N, float* d_msg, int64_t ldo, float* d_lse, void* stream);
int linetr_sig_attention_backward(LinetrHandle* h, const float* d_q, int64_t ldq, const float* d_k, int64_t ldk, const float* d_v, int64_t ldv,
                                  const float* d_msg, int64_t ldo, const float* d_lse, const float* d_g, int64_t ldg, const int32_t* d_cu_sub,
                                  int32_t n_images, int64_t N, float* d_dq, int64_t lddq, float* d_dk, int64_t lddk, float* d_dv,
                                  int64_t lddv, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- BatchNorm1d (+ ReLU) for training, forward and backward (section 8(f) "next" row 4: the fourth link) ---------- */

/* torch.nn.BatchNorm1d (+ F.relu) on rows z [rows][C] (rows = B n positions, row stride ldz), as the MLP of the signature layer applies
 * it (models/line_transformer.py:9-20, :161), OUT OF PLACE -- z is kept, the backward reads it -- and its backward as torch autograd
 * differentiates it.  4 <= C <= 512, C % 4 == 0; every row stride at least C and a multiple of 4 floats; 16-byte aligned pointers.
 *   forward, mode LINETR_BN_TRAIN:  mean, var = the batch mean and BIASED variance over all rows, float64 sums in row chunks added in
 *     ascending order (the kernels and the chunking of linetr_forward_train);  invstd = 1 / sqrt(var + eps);  alpha = gamma invstd;
 *     beta' = beta - mean alpha (both rounded to float32);  y = max(z alpha + beta', 0), or without the max (relu = 0): the bits of
 *     linetr_forward_train's layer on the same z.  d_running [mean[C] | var[C]] (may be NULL) <- (1 - momentum) running + momentum
 *     (mean | var n / (n - 1)), in place, the same bits too.  rows = 1: var = 0 and the unbiased factor is taken as 1.
 *   forward, mode LINETR_BN_EVAL:  mean | var = d_running (required, only read); nothing is updated.
 *   d_save [2 C] float64 <- mean[C] | invstd[C] (the batch's, or the running ones): what the backward takes.
 *   backward:  g' = g where y > 0, else 0 (d_y: the layer's own output as the forward wrote it, NULL for relu = 0; nothing is recomputed to
 *     decide a sign);  xhat = (z - mean) invstd, z - mean formed in float64;
 *       dbeta[c] = sum_r g'      dgamma[c] = sum_r g' xhat      (float64 sums, the forward's chunks, ascending; rounded to float32)
 *       LINETR_BN_TRAIN:  dz = gamma invstd (g' - dbeta / n - xhat dgamma / n)        LINETR_BN_EVAL:  dz = gamma invstd g'
 *     evaluated as k1 g' - k2 - k3 fl(z - mean) in float32 with per-channel float32 coefficients.  d_dz [rows][lddz], d_dgamma [C],
 *     d_dbeta [C]: each may be NULL and is then not computed.
 * Three launches each way (eval forward: two).  Deterministic: no atomics, fixed summation order, two calls give the same bits.  Columns
 * behind C and rows behind `rows` are neither read nor written.  The caller owns the workspace (linetr_bn_*_workspace_bytes(rows, C); 0
 * for a shape that is refused).  Asynchronous on `stream`; nothing inside allocates or waits; `h` may be NULL (it names the device and
 * collects the profile; no training-mode handle is needed).  rows <= 0: nothing is launched.  LINETR_E_ARG, nothing launched: C outside
 * the above, rows beyond 2^30, a mode or relu outside 0 .. 1, eps <= 0, momentum outside 0 .. 1, a bad row stride (that of a NULL tensor
 * is not read), a pointer that is not 16-byte aligned, a NULL required pointer (forward: d_z, d_gamma, d_beta, d_y, d_save, the
 * workspace, d_running in eval mode; backward: d_z, d_g, d_save, d_gamma, the workspace), a workspace smaller than
 * linetr_bn_*_workspace_bytes says. */
enum { LINETR_BN_TRAIN = 0, LINETR_BN_EVAL = 1 };
int64_t linetr_bn_forward_workspace_bytes(int64_t rows, int32_t C);
int linetr_bn_forward(LinetrHandle* h, const float* d_z, int64_t ldz, int64_t rows, int32_t C, const float* d_gamma, const float* d_beta,
                      float eps, float momentum, float* d_running, int32_t mode, int32_t relu, float* d_y, int64_t ldy, double* d_save,
                      void* d_workspace, int64_t workspace_bytes, void* stream);
int64_t linetr_bn_backward_workspace_bytes(int64_t rows, int32_t C);
int linetr_bn_backward(LinetrHandle* h, const float* d_z, int64_t ldz, const float* d_y, int64_t ldy, const float* d_g, int64_t ldg,
                       const double* d_save, const float* d_gamma, int64_t rows, int32_t C, int32_t mode, float* d_dz, int64_t lddz,
                       float* d_dgamma, float* d_dbeta, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- the line descriptive layer for training (section 8(f) "next" row 4: the fifth link) ---------- */

/* LineDescriptiveEncoder (models/line_transformer.py:75-91 = MultiHeadAttention + FeedForward, models/line_attention.py:23-94) is
 * trained in the folded form of DESIGN 3.1-3.3: KeylineEncoder reads only the CLS row of its output (:128), the CLS query row is never
 * masked, so per segment (sub-line) l of S token rows and head h, with u_lh = Wk_h^T (q_lh / 8) made by the linear layers above,
 *   s_t = u_h . x_t      lse_h = m + logf(l) of the scores      p_t = exp(s_t - lse_h)      pooled_h = sum_t p_t x_t
 * and the value projection is applied to pooled_h afterwards.  The key bias adds one constant per (l, h), which the softmax cancels.
 * Backward, as torch autograd differentiates the above:
 *   delta_h = dpooled_h . pooled_h      dp_t = dpooled_h . x_t      ds_t = p_t (dp_t - delta_h)      (p recomputed from x, u and lse)
 *   dx_t = sum_h (p_t dpooled_h + ds_t u_h)      du_h = sum_t ds_t x_t  (token order)
 *   d_x, d_dx     [L S][256 of ldx / lddx] float32 token rows, segment l = rows l S .. l S + S - 1;  1 <= S <= 256, 0 <= L <= 2^24
 *   d_u, d_du     [L][1024 of ldu / lddu], head h in columns h*256 ..
 *   d_pooled, d_dpooled [L][1024] contiguous      d_lse [L][4] contiguous
 *   d_dx, d_du    each may be NULL and is then not computed (what is computed has the same bits either way)
 * One launch each way, one wave per segment, x read once per direction (the backward writes dx as well): bound by bytes.
 * Deterministic: no atomics, every sum in a fixed order.  Rows behind L S and columns behind the widths are neither read nor written.
 * Asynchronous on `stream`; nothing inside allocates or waits; `h` may be NULL.  L = 0: nothing is launched.  LINETR_E_ARG, nothing
 * launched: S or L outside the above, a row stride below the width or no multiple of 4 floats (that of a NULL output is not read), a
 * pointer that is not 16-byte aligned, a NULL required pointer (every one but d_dx / d_du). */
int linetr_cls_pool_train_forward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_u, int64_t ldu, int64_t L, int32_t S,
                                  float* d_pooled, float* d_lse, void* stream);
int linetr_cls_pool_train_backward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_u, int64_t ldu, const float* d_pooled,
                                   const float* d_lse, const float* d_dpooled, int64_t L, int32_t S, float* d_dx, int64_t lddx,
                                   float* d_du, int64_t lddu, void* stream);

/* torch.nn.LayerNorm(256) on rows with an optional residual, as the reference's `q += residual; q = self.layer_norm(q)`
 * (models/line_attention.py:72-73, :91-92), and its backward:
 *   v = a + r (one float32 add; d_r NULL: v = a)      mean, var (biased) two-pass on the row      rstd = 1 / sqrt(var + eps)
 *   y = (v - mean) rstd gamma + beta      d_stats [rows][2] float32 <- mean | rstd: what the backward takes
 *   backward:  xhat = (v - mean) rstd      gg = g gamma      dx = rstd (gg - mean_c gg - xhat mean_c (gg xhat)): the gradient of a AND of r
 *     dgamma = sum_r g xhat      dbeta = sum_r g      (float32 partial sums per chunk of rows, the chunks added in ascending order in
 *     float64 through the workspace)      d_dx, d_dgamma, d_dbeta: each may be NULL and is then not computed
 * C must be 256; 0 <= rows <= 2^30; every row stride at least 256 and a multiple of 4 floats; 16-byte aligned pointers.  Forward one
 * launch, backward two.  Deterministic.  Asynchronous on `stream`; nothing inside allocates or waits; `h` may be NULL.  rows = 0: no row
 * is touched (dgamma / dbeta, where asked for, are zeros).  LINETR_E_ARG, nothing launched: C != 256, rows outside the above, eps <= 0, a
 * bad row stride (that of a NULL tensor is not read), a pointer that is not 16-byte aligned, a NULL required pointer (forward: d_a,
 * d_gamma, d_beta, d_y, d_stats; backward: d_a, d_stats, d_gamma, d_g, and the workspace when d_dgamma or d_dbeta is asked for), a
 * workspace smaller than linetr_layer_norm_backward_workspace_bytes says (0 for a shape that is refused). */
int64_t linetr_layer_norm_backward_workspace_bytes(int64_t rows, int32_t C);
int linetr_layer_norm_forward(LinetrHandle* h, const float* d_a, int64_t lda, const float* d_r, int64_t ldr, const float* d_gamma,
                              const float* d_beta, float eps, int64_t rows, int32_t C, float* d_y, int64_t ldy, float* d_stats, void* stream);
int linetr_layer_norm_backward(LinetrHandle* h, const float* d_a, int64_t lda, const float* d_r, int64_t ldr, const float* d_stats,
                               const float* d_gamma, const float* d_g, int64_t ldg, int64_t rows, int32_t C, float* d_dx, int64_t lddx,
                               float* d_dgamma, float* d_dbeta, void* d_workspace, int64_t workspace_bytes, void* stream);

/* F.gelu, erf form (models/line_attention.py:89), on rows [rows][C of ld*]:  y = z Phi(z)      dz = g (Phi(z) + z phi(z)) from the saved
 * pre-activation z;  Phi(z) = erfc(-z / sqrt 2) / 2, phi(z) = exp(-z^2 / 2) / sqrt(2 pi).  4 <= C <= 4096, C % 4 == 0, 0 <= rows <= 2^30
 * (rows C / 4 below 2^39).  One launch.  Asynchronous; `h` may be NULL.  LINETR_E_ARG, nothing launched: a shape outside the above, a row
 * stride below C or no multiple of 4 floats, a NULL or misaligned pointer. */
int linetr_gelu_forward(LinetrHandle* h, const float* d_z, int64_t ldz, int64_t rows, int32_t C, float* d_y, int64_t ldy, void* stream);
int linetr_gelu_backward(LinetrHandle* h, const float* d_z, int64_t ldz, const float* d_g, int64_t ldg, int64_t rows, int32_t C, float* d_dz,
                         int64_t lddz, void* stream);

/* ---- training-time dropout of the line descriptive layer ---------- */

/* The reference trains with nn.Dropout(0.1) at three places of every descriptive layer (models/line_attention.py:18 on the attention
 * weights, :70 behind fc, :90 behind w_2).  Here a mask is never stored: it is a pure function of (seed, call, site, row, element) that
 * the forward AND the backward kernels generate, the same bits on every launch geometry.  Generator: Philox4x32-10, multipliers
 * 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85; key = (seed & 0xffffffff, seed >> 32), counter = (inner, row, call,
 * site).  A word w keeps its element iff w >= threshold (= floor(p 2^32), made by the caller in double); the factor r is `scale`
 * (= float(1 / (1 - p))) for a kept element and 0 for a dropped one.  threshold = 0, scale = 1 is p = 0 and gives the bits of the entry
 * points without dropout.
 *   site 0   the CLS query row's attention weights: row = segment l, inner = token t, word h belongs to head h
 *   site 1/2 the [rows][256] tensor in front of the first / second residual LayerNorm: inner = column / 4, word k = column 4 inner + k
 * `call` is the caller's count of training forwards; a backward passes the value its forward used. */
typedef struct {
  uint64_t seed;
  uint32_t call;
  uint32_t threshold;
  float scale;
} LinetrDropout;

/* linetr_cls_pool_train_forward / _backward with site 0 (every argument they share means what it means there):
 *   a_t = p_t r_t      pooled_h = sum_t a_t x_t      kept_h = sum_t a_t      d_kept [L][4] contiguous; d_lse is that of the full softmax
 *   (the value projection behind it is then Wv_h pooled_h + kept_h bv_h: without dropout kept = 1)
 *   da_t = dpooled_h . x_t + dkept_h      delta_h = dpooled_h . pooled_h + dkept_h kept_h      ds_t = p_t (r_t da_t - delta_h)
 *   dx_t = sum_h (a_t dpooled_h + ds_t u_h)      du_h = sum_t ds_t x_t      d_dkept [L][4] may be NULL: no gradient arrives at kept
 * A (segment, head) all of whose tokens are dropped gives pooled = 0 and kept = 0 exactly and adds nothing to dx and du; no NaN.
 * `drop` is read before the call returns.  LINETR_E_ARG, nothing launched: what the plain entry points refuse, a NULL `drop`, d_kept or
 * (backward) a misaligned d_dkept, a scale that is not finite or below 1. */
int linetr_cls_pool_dropout_forward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_u, int64_t ldu, int64_t L, int32_t S,
                                    const LinetrDropout* drop, float* d_pooled, float* d_kept, float* d_lse, void* stream);
int linetr_cls_pool_dropout_backward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_u, int64_t ldu, const float* d_pooled,
                                     const float* d_lse, const float* d_kept, const float* d_dpooled, const float* d_dkept, int64_t L,
                                     int32_t S, const LinetrDropout* drop, float* d_dx, int64_t lddx, float* d_du, int64_t lddu, void* stream);

/* linetr_layer_norm_forward / _backward with dropout on `a` at `site` (1 or 2; 0 is accepted and draws site 0's words in the layout of
 * sites 1 / 2):  v = fl(r a) + residual -- the product is rounded on its own, so that every output has the bits of the plain entry
 * points on a pre-masked a --, y = LN(v).  The backward returns two tensors: d_dr <- dv (the gradient of the residual, what the plain
 * backward calls dx) and d_da <- r dv; each may be NULL.  The workspace is that of linetr_layer_norm_backward.  LINETR_E_ARG, nothing
 * launched: what the plain entry points refuse, a site outside 0..2, a NULL `drop`, a scale that is not finite or below 1. */
int linetr_layer_norm_dropout_forward(LinetrHandle* h, const float* d_a, int64_t lda, const float* d_r, int64_t ldr, const float* d_gamma,
                                      const float* d_beta, float eps, int64_t rows, int32_t C, const LinetrDropout* drop, int32_t site,
                                      float* d_y, int64_t ldy, float* d_stats, void* stream);
int linetr_layer_norm_dropout_backward(LinetrHandle* h, const float* d_a, int64_t lda, const float* d_r, int64_t ldr, const float* d_stats,
                                       const float* d_gamma, const float* d_g, int64_t ldg, int64_t rows, int32_t C,
                                       const LinetrDropout* drop, int32_t site, float* d_da, int64_t ldda, float* d_dr, int64_t lddr,
                                       float* d_dgamma, float* d_dbeta, void* d_workspace, int64_t workspace_bytes, void* stream);

/* The factors themselves: d_out [rows][inner][4] float32 <- `scale` or 0 for the words of counter (inner, row, call, site).  What the
 * kernels above apply at site 0 to segment `row`, token `inner`, heads 0..3, and at sites 1 / 2 to row `row`, columns 4 inner .. + 3.
 * Stateless; for tests and for looking at a mask.  0 <= rows < 2^31, 1 <= inner < 2^31, rows * inner <= 2^38.  rows = 0: nothing is
 * launched.  LINETR_E_ARG, nothing launched: a shape outside the above, a site outside 0..2, a NULL or misaligned d_out, a NULL
 * `drop`, a scale that is not finite or below 1. */
int linetr_dropout_factors(LinetrHandle* h, const LinetrDropout* drop, int32_t site, int64_t rows, int64_t inner, float* d_out, void* stream);

/* ---- the positional encoders and the token assembly for training (section 8(f) "next" row 4: the sixth link) ---------- */

/* The first layer of LinePositionalEncoder / WordPositionalEncoder (models/line_transformer.py:40-73), Conv1d(Kin -> N, k = 1) with
 * Kin = 5 / 3 and N = 32, which is no GEMM (every later layer is the linear layer above), and its backward:
 *   z [rows][N of ldz] = x [rows][Kin of ldx] W^T + b      W [N][Kin], d_b [N] or NULL (no bias); per channel one fmaf chain in
 *     ascending k that starts at the bias
 *   dW [N][Kin] = g^T x      db [N] = sum_r g      g [rows][N of ldg]: the gradient arriving at z (no activation, so no mask)
 *   dx is not computed: the coordinates, scores and angles the encoders read never require a gradient.
 * 0 <= rows <= 2^30, 1 <= Kin <= 8, N % 4 == 0, 4 <= N <= 64.  x is the narrow tensor: ldx >= Kin floats and any (4-byte) alignment, as W,
 * b, dW and db; z and g are the wide ones: 16-byte aligned, ldz / ldg at least N and multiples of 4 floats.  dW / db: the rows are cut
 * into chunks of linetr_input_layer_chunk_rows() rows (a compile-time constant), each chunk is summed in float32 in a fixed order and the
 * chunks are added in ascending order in float64 through the workspace.  d_dW, d_db: each may be NULL and is then not computed (both
 * NULL: nothing is launched and the workspace is not needed).  Forward one launch, backward two.  Deterministic: no atomics.  Rows
 * behind `rows` and columns behind the widths are neither read nor written.  Asynchronous on `stream`; nothing inside allocates or
 * waits; `h` may be NULL.  rows = 0: no row is touched (dW / db, where asked for, are zeros).  LINETR_E_ARG, nothing launched: a shape
 * outside the above, a bad row stride, a misaligned pointer, a NULL required pointer (forward: d_x, d_W, d_z; backward: d_x, d_g, and
 * the workspace when a gradient is asked for), a workspace smaller than linetr_input_layer_backward_workspace_bytes says (0 for a
 * shape that is refused). */
int32_t linetr_input_layer_chunk_rows(void);
int64_t linetr_input_layer_backward_workspace_bytes(int64_t rows, int32_t N, int32_t Kin);
int linetr_input_layer_forward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_W, const float* d_b, int64_t rows, int32_t N,
                               int32_t Kin, float* d_z, int64_t ldz, void* stream);
int linetr_input_layer_backward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_g, int64_t ldg, int64_t rows, int32_t N,
                                int32_t Kin, float* d_dW, float* d_db, void* d_workspace, int64_t workspace_bytes, void* stream);

/* The token rows the descriptive layer reads (KeylineEncoder, models/line_transformer.py:116-121): per segment (sub-line) l of S tokens
 *   x [L][S + 1][256]      x[l][0] = cls      x[l][1 + t] = desc[l][t] + pos[l][t]  (one float32 add)
 *   d_desc, d_pos [L S][256] contiguous rows, d_cls [256]
 * and its backward from d_dx [L][S + 1][256], in one pass over it:
 *   d_dtok [L S][256] = dx[:, 1:] as contiguous rows: the gradient of desc and of pos alike      d_dcls [256] = sum_l dx[l][0]
 *     (float32 partial sums per block of segments in segment order, the blocks added in ascending order in float64 through the workspace)
 *   d_dtok, d_dcls: each may be NULL and is then not computed
 * 1 <= S <= 255 (with the CLS slot: the 256 rows the pooling takes), 0 <= L <= 2^24; 16-byte aligned pointers.  Forward one launch,
 * backward two.  Deterministic.  Asynchronous on `stream`; nothing inside allocates or waits; `h` may be NULL.  L = 0: no row is
 * touched (dcls, where asked for, is zeros).  LINETR_E_ARG, nothing launched: S or L outside the above, a pointer that is not 16-byte
 * aligned, a NULL required pointer (forward: all four; backward: d_dx, and the workspace when d_dcls is asked for), a workspace smaller
 * than linetr_token_assemble_backward_workspace_bytes says (0 for an L that is refused). */
int64_t linetr_token_assemble_backward_workspace_bytes(int64_t L);
int linetr_token_assemble_forward(LinetrHandle* h, const float* d_desc, const float* d_pos, const float* d_cls, int64_t L, int32_t S,
                                  float* d_x, void* stream);
int linetr_token_assemble_backward(LinetrHandle* h, const float* d_dx, int64_t L, int32_t S, float* d_dtok, float* d_dcls,
                                   void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- ground-truth line assignment of a homography pair (the producer of d_assign / d_lmatches above) ---------- */

/* What the reference's dataset builder computes for one image pair with two Python double loops over every pair of sub-lines
 * (dataloaders/build_homography_dataset.py:210-237), for a batch of B pairs, on the device:
 *   :214-218  klns0_projected = cv2.perspectiveTransform(klns0, H), klns1_projected = cv2.perspectiveTransform(klns1, inv(H)),
 *             restated from OpenCV's arithmetic (cv2 is not a dependency): in double w = x m6 + y m7 + m8, w = (w != 0) ? 1 / w : 0,
 *             X = (x m0 + y m1 + m2) w, cast to the coordinate type;
 *   :222-225  find_line_matches (dataloaders/utils/util_lines.py:67-114) in both directions -- direction 0: reference line lines0[i]
 *             against proj(lines1[j], inv(H)); direction 1: reference line lines1[j] against proj(lines0[i], H).  A pair is skipped
 *             when BOTH end points lie further than thres_reprojected from the reference line, or abs(angle1 - angle0) % 180 >
 *             thres_angdiff with angle = degrees(arctan2(dx, dy)), or neither end point lies on the reference line and the largest
 *             end-point distance exceeds len0 + len1;
 *   :227-233  calculate_line_overlaps (util_lines.py:116-171) in both directions; assign[i][j] = both directions matched ? the larger
 *             of the two overlaps : 0;
 *   :234-237  lmatches = np.where(assign > min_overlap_ratio) in row-major order, -1 behind the list.
 * coord_type selects the arithmetic: LINETR_COORD_F32 is the reference as executed (its sub-lines are float32 tensors, so NumPy
 * computes every scalar in float32), LINETR_COORD_F64 is for float64 geometry.  No contraction, the reference's operation order,
 * x * x for ** 2, correctly rounded divide and square root: every compare but the angle one is the reference's bit for bit, and the
 * overlaps are its values.  (arctan2 is not correctly rounded on either side: an entry can differ only where the angle compare is
 * within a few ulp of an angle of flipping.  The reference's scalar ** 2 is libm's powf, which may round an exact tie of x * x the
 * other way.)  thres_reprojected and thres_angdiff are compared in the coordinate type, min_overlap_ratio in float64 against the
 * unrounded value, as NumPy does.
 *   d_lines0 [B][n0][2][2], d_lines1 [B][n1][2][2]   end points (x, y) in the coordinate type
 *   d_H [B][2][9] float64                            per item H (image 0 -> image 1), then inv(H) as the caller computed it
 *   d_count0 / d_count1 [B] int32 or NULL            valid prefix of each item (clamped to 0 .. n); rows / columns beyond it hold 0
 *                                                    and no match.  0 is legal.
 * Outputs, any may be NULL:
 *   d_assign [B][n0 + pad][n1 + pad] float32         pad = 1 adds the zero dustbin row and column linetr_val_step's d_assign has
 *   d_lmatches [B][M][2] int32, d_found [B] int32    the list, -1 behind it.  d_found is never capped: an item with d_found[b] > M
 *                                                    has been cut to its first M pairs and nothing is written past M (the contract
 *                                                    of linetr_superpoint_keypoints' d_found).  Deterministic: no atomics.
 *   d_match_dir [B][2][n0][n1] uint8                 find_line_matches per direction, direction 1 stored transposed as [i][j]
 *   d_overlap_dir [B][2][n0][n1] coordinate type     calc_overlap per direction for EVERY pair, matched or not, stored likewise
 *   d_proj0 [B][n0][2][2], d_proj1 [B][n1][2][2]     the projected lines (all n rows, whatever the counts)
 * Asynchronous on `stream`; nothing inside allocates or waits; `h` may be NULL.  B, n0 or n1 <= 0 (or beyond 65535 items / 32768
 * lines), M < 0, pad outside {0, 1}, an unknown coord_type, a NULL input or a workspace smaller than
 * linetr_gt_assign_workspace_bytes says: LINETR_E_ARG, nothing launched. */
enum { LINETR_COORD_F32 = 0, LINETR_COORD_F64 = 1 };
int64_t linetr_gt_assign_workspace_bytes(int32_t B, int32_t n0, int32_t n1);
int linetr_gt_assign(LinetrHandle* h, int32_t coord_type, const void* d_lines0, int32_t n0, const void* d_lines1, int32_t n1,
                     const double* d_H, int32_t B, const int32_t* d_count0, const int32_t* d_count1, double thres_reprojected,
                     double thres_angdiff, double min_overlap_ratio, int32_t pad, float* d_assign, int32_t* d_lmatches, int32_t M,
                     int32_t* d_found, uint8_t* d_match_dir, void* d_overlap_dir, void* d_proj0, void* d_proj1, void* d_workspace,
                     int64_t workspace_bytes, void* stream);

/* ---- fixed-size training samples (the producer of the batches linetr_forward_train, linetr_gt_assign and the criterion consume) ---------- */

/* The pseudo lines conv_fixed_size pads a sample with (dataloaders/utils/util_lines.py:559-617, make_pseudo_lines), host, float64:
 * n lines h_lines [n][2][2] for image `image_index` of a batch.  Per line: start point (shape0 - min_length - 15, shape1 - min_length
 * - 15) * U^2, angle 2 pi U, length (160 - min_length) U + min_length, end point = start + length (cos, sin), both coordinates
 * clipped to [15, shape_i - 15]; the first draw stands unless it came out shorter than min_length, a redraw must be longer (the
 * reference's two compares).  The reference draws from NumPy's reseeded global generator; here every U is 53 bits of
 * Philox4x32-10 (the generator of the dropout masks), key = (seed, image_index), counter = (line, attempt, draw, 0): draw 0 gives
 * the start point (words 0,1 -> x; 2,3 -> y), draw 1 the angle and the length; U = ((hi >> 5) 2^26 + (lo >> 6)) / 2^53.  At most 64
 * attempts, then the fixed line (15, 15) -> (15 + 2 min_length, 15).  The same (seed, image_index, line) gives the same bits on
 * every call, whatever n.  LINETR_E_ARG: n < 0, a seed beyond 32 bits, min_length outside (0, 160), a shape without room
 * (shape_i < 30 + 2 min_length). */
int linetr_make_pseudo_lines(uint64_t seed, int32_t image_index, int32_t n, double shape0, double shape1, double min_length,
                             double* h_lines);

/* find_line_attributes (util_lines.py:634-668), host, float64: end points swapped unless sp_x < ep_x, length = sqrt(dx dx + dy dy),
 * lines shorter than min_length dropped, sorted by descending length under linetr_prefilter's tie rule (equal lengths by descending
 * original index), cut to [:max_sublines], angles as get_angles (the pre-filter's).  Writes *n_out rows of h_klines [n][2][2],
 * h_length [n], h_angles [n][2] (each sized for all n lines).  LINETR_E_ARG: n < 0, a NULL array with n > 0, a NULL n_out, a coordinate
 * that is NaN or infinite (its length has no place in the order).  max_sublines may be any int32 (negative: the slice [:max_sublines]). */
int linetr_find_line_attributes(const double* h_lines, int32_t n, double min_length, int32_t max_sublines, double* h_klines,
                                double* h_length, double* h_angles, int32_t* n_out);

/* The 'klines' branch of conv_fixed_size (dataloaders/utils/util_lines.py:695-766, called at build_homography_dataset.py:205-206) for a
 * batch of B images, on the device, straight from line records: what linetr_tokenize would emit for image b, padded to M =
 * max_sublines sub-lines with tokenised pseudo lines or cut to M, in [B, M, ...] tensors.
 *   d_recs, h_cu_k, h_cu_n     the batch's records (device; image-major, as linetr_prefilter_batch writes them) and the HOST prefix
 *                              sums [B + 1] of key-lines (num_klns) and sub-lines (num_slns) per image; an image may have none
 *   d_pseudo, h_pseudo, h_cu_p the pseudo records on the device and the same array on the host, with their HOST prefix sums [B + 1].
 *                              Image b must bring exactly max(M - num_slns, 0) of them, `image` = b, `line_local` = 0, 1, .. and
 *                              n_sub = 1 each (linetr_pack_lines with image_index b; first_sub / first_tok are not read)
 *   clip_height / clip_width   the end-point clip of the real lines (linetr_tokenize's; <= 0: height / width);
 *   pseudo_clip_height / _width  the one of the pseudo lines: the builder hands conf['data']['resize'] = (640, 480) to line_tokenizer
 *                              as (height, width), i.e. x <= 479.4 and y <= 639.4 for a 480 x 640 image (util_lines.py:701,713)
 *   d_dense_desc / d_dense_score, dense_is_nhwc, align_corners   as linetr_tokenize
 * Outputs, all required, every byte written exactly once by this call (nothing has to be cleared), float32 unless noted:
 *   out.klines [B,M,2,2], out.length [B,M], out.angles [B,M,2]   real key-lines at [:num_klns], the pseudo key-lines (the tokeniser's
 *                              float32 copies, clipped end points included) behind them, zeros behind those
 *   out.sublines [B,M,2,2], out.pnt [B,M,T,2], out.mask [B,M,T+1], out.resp [B,M], out.angle_sub [B,M,2], out.desc [B,M,T,256],
 *   out.score [B,M,T]          the image's first min(num_slns, M) sub-line rows, then the pseudo rows.  The cut may fall inside a split
 *                              key-line.  Every row has the bits linetr_tokenize gives it (one device body each)
 *   out.mat [B,M,M]            eye(M) with the block [:num_klns, :min(num_slns, M)] replaced by the image's mat_klines2sublines: a pseudo
 *                              sub-line j has its 1 at [j][j], and rows num_klns .. num_slns - 1 keep a diagonal 1 (the reference's)
 *   d_num_klns, d_num_slns [B] int32   the counts before padding / truncation
 * Superset of the reference: an image without a surviving line is M pseudo lines with num_klns = num_slns = 0 (the reference raises).
 * Three launches (+ the layout pass of an NCHW map, + one small launch per 32 images that carries the prefix sums): nothing var-len is
 * materialised, tokens, scores and descriptors go straight to their final rows.  Asynchronous on `stream`; nothing inside allocates or
 * waits; the host arrays are read before the call returns; `h` may be NULL.  LINETR_E_ARG, nothing launched, no output changed: B < 1
 * (or above 65 535), height / width no multiple of 8, M outside 1 .. 32 768, T outside 1 .. 4096, token_distance <= 0, B M T beyond
 * 2^33, a NULL pointer, prefix sums that do not start at 0 or ascend, an image with more key-lines than M (the reference raises
 * there), a pseudo count other than max(M - num_slns, 0), a pseudo line that does not make exactly one sub-line, a channel-last map,
 * out.desc or workspace that is not 16-byte aligned.  LINETR_E_WORKSPACE, nothing launched: a workspace smaller than
 * linetr_fixed_size_workspace_bytes says. */
int64_t linetr_fixed_size_workspace_bytes(int32_t n_images, int32_t height, int32_t width, int32_t dense_is_nhwc);
int linetr_fixed_size(LinetrHandle* h, const LinetrLineRec* d_recs, const int32_t* h_cu_k, const int32_t* h_cu_n,
                      const LinetrLineRec* d_pseudo, const LinetrLineRec* h_pseudo, const int32_t* h_cu_p, int32_t n_images,
                      int32_t max_sublines, int32_t max_tokens, double token_distance, const float* d_dense_desc,
                      const float* d_dense_score, int32_t height, int32_t width, int32_t clip_height, int32_t clip_width,
                      int32_t pseudo_clip_height, int32_t pseudo_clip_width, int32_t align_corners, int32_t dense_is_nhwc,
                      LinetrTokens out, int32_t* d_num_klns, int32_t* d_num_slns, void* d_workspace, int64_t workspace_bytes,
                      void* stream);

/* ---- the optimizer step (section 8(f) "next" row 4: the line that changes the weights) ---------- */

/* torch.optim.Adam as the reference builds it (train.py:82) and steps it (:195), over a table of tensors in ONE launch, and the global
 * gradient norm of the same table, whose clipping coefficient the step can read on the device.
 *
 * h_table: a HOST array of n_tensors entries; p / g / m / v are DEVICE pointers to n float32 each (parameter, gradient, exp_avg,
 * exp_avg_sq).  The library cuts every tensor into chunks of 4 096 elements, one block each, and puts the table with its chunk prefix
 * into the caller's workspace through the arguments of small launches of 64 entries each in front of the update: h_table is read
 * before the call returns, nothing on the host is kept, and the call never waits for the stream.  A block finds its tensor by a
 * binary search of the prefix.
 *
 * The update, per element, float32, one rounding per written operation: the order of torch's non-capturable single-tensor path
 * (torch/optim/adam.py, _single_tensor_adam, torch 2.10).  Every float(.) is formed in double first.
 *   g  <- fl(scale g)                         only when d_grad_scale != NULL (one float32 read on the device); rounded on its own
 *   coupled   (decoupled == 0, weight_decay != 0):  g <- fmaf(wd, p, g)
 *   decoupled (decoupled == 1, weight_decay != 0):  p <- p float(1 - lr wd)
 *   m' = fmaf(float(1 - beta1), g - m, m)
 *   v' = fmaf(float(1 - beta2) g, g, float(beta2) v)
 *   d  = sqrtf(v') / bc2_sqrt + float(eps)     IEEE square root and division
 *   p' = fmaf(-step_size, m' / d, p)
 * p, m and v are updated in place; g is only read (a scale never rewrites it).  step_size = lr / (1 - beta1^step) and bc2_sqrt =
 * sqrt(1 - beta2^step) are made by the caller in double, per tensor, as torch makes them: a parameter that got no gradient on some
 * steps has its own step count.  `lr` of the hyper-parameters is read by the decoupled decay alone.
 * 16 bytes per lane where p, g, m and v of a tensor are all 16-byte aligned, 4 bytes per lane otherwise (views carved out of a flat
 * buffer); nothing outside [0, n) of a tensor is touched.  Deterministic; no atomics.  Asynchronous on `stream`; nothing inside
 * allocates or waits; `h` may be NULL.  A table of no elements at all: LINETR_OK, nothing launched.
 * LINETR_E_ARG, nothing launched, no output changed: a NULL table or hyper; n_tensors outside 1 .. 65 536; n < 0; more than 2^30
 * chunks; for a tensor with n > 0 a NULL or not 4-byte aligned p / g / m / v, two of the four equal, a step_size that is not finite, a
 * bc2_sqrt not in (0, 1]; a beta outside [0, 1); eps or weight_decay negative or not finite; decoupled not 0 / 1, or 1 with an lr that
 * is not finite; a misaligned d_grad_scale; a NULL, not 256-byte aligned or short workspace (linetr_adam_workspace_bytes of the table's
 * n_tensors and total element count; 0 for a shape that is refused). */
typedef struct {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  float step_size;
  float bc2_sqrt;
} LinetrAdamTensor; /* 48 bytes */
typedef struct {
  double beta1, beta2, eps, weight_decay, lr;
  int32_t decoupled;
} LinetrAdamHyper;

int64_t linetr_adam_workspace_bytes(int32_t n_tensors, int64_t n_total);
int linetr_adam_step(LinetrHandle* h, const LinetrAdamTensor* h_table, int32_t n_tensors, const LinetrAdamHyper* hyper,
                     const float* d_grad_scale, void* d_workspace, int64_t workspace_bytes, void* stream);

/* The L2 norm of every g of the table together (only g and n of an entry are read), deterministic, and the coefficient of
 * torch.nn.utils.clip_grad_norm_:
 *   d_norm[0]  <- sqrt(sum g^2)                                float64
 *   d_scale[0] <- float(min(1, max_norm / (norm + 1e-6)))      max_norm = +inf: the norm alone, the scale is then 1; a NaN norm gives NaN
 * Same chunks as the step.  Each chunk's squares are summed in float64 in a fixed order into the workspace (lane t of 256 adds elements
 * t, t + 256, ... in ascending order; the lanes by a fixed tree); a second, one-block launch adds the chunks' sums: 256 contiguous runs,
 * each in ascending order, then the runs in ascending order.  The bits depend on the table's sizes alone, not on alignment.  No host
 * wait: linetr_adam_step reads d_scale on the device.  A table of no elements: norm 0, scale 1 (one launch).
 * LINETR_E_ARG, nothing launched, no output changed: what the step refuses of the table (g alone of the pointers), a max_norm that is
 * negative or NaN, a NULL d_norm (8-byte aligned) or d_scale (4-byte aligned), a NULL, not 256-byte aligned or short workspace
 * (linetr_grad_norm_workspace_bytes). */
int64_t linetr_grad_norm_workspace_bytes(int32_t n_tensors, int64_t n_total);
int linetr_grad_norm(LinetrHandle* h, const LinetrAdamTensor* h_table, int32_t n_tensors, double max_norm, double* d_norm,
                     float* d_scale, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- dense-map producer (section 8(f) "next" row 2) ------------------------------------------------- */

/* Post-processing of SuperPoint's two heads, fused with the layout change the tokeniser needs; replaces
 *   models/superpoint.py:161-167  scores = softmax(convPb(.), 1)[:, :-1]; permute/reshape to [B, 8Hc, 8Wc]
 *   models/superpoint.py:190-193  dense_descriptor = F.normalize(convDb(.), p=2, dim=1)
 * d_score_logits [B,65,Hc,Wc] and d_desc_raw [B,256,Hc,Wc] are the raw convPb / convDb outputs (float32, NCHW,
 * contiguous).  Outputs (any may be NULL): d_dense_score [B,8Hc,8Wc]; d_dense_desc_nhwc [B,Hc,Wc,256] -- pass it
 * to linetr_describe with dense_is_nhwc = 1 and the NCHW->NHWC pass disappears; d_dense_desc_nchw [B,256,Hc,Wc],
 * the reference's 'dense_descriptor' layout.  `h` may be NULL (no weights involved; current HIP device).
 * Every output must be 16-byte aligned, and so must both inputs when Hc * Wc is a multiple of 4 (their planes are then loaded as
 * 16-byte vectors): LINETR_E_ARG otherwise, before anything is launched. */
int linetr_superpoint_heads(LinetrHandle* h, const float* d_score_logits, const float* d_desc_raw, int32_t B,
                            int32_t Hc, int32_t Wc, float* d_dense_score, float* d_dense_desc_nhwc,
                            float* d_dense_desc_nchw, void* stream);

/* linetr_superpoint_heads for raw head outputs and descriptor maps of another element type (a SuperPoint run under autocast).
 * in_type: the type of d_score_logits AND d_desc_raw; out_type: the type of d_dense_desc_nhwc AND d_dense_desc_nchw; each 0 (float32),
 * LINETR_DENSE_F16 or LINETR_DENSE_BF16, anything else is refused with nothing written.  d_dense_score is float32 always.  The
 * arithmetic is linetr_superpoint_heads': half inputs are converted exactly at the load, so the results equal that call's on the upcast
 * inputs; half outputs are its float32 outputs rounded to nearest-even.  linetr_superpoint_heads is this call with 0, 0.
 * Alignment (LINETR_E_ARG otherwise): float32 pointers 16 bytes as there; half outputs 8 bytes; half inputs 8 bytes when Hc * Wc is a
 * multiple of 4 (the vector path), else 2. */
int linetr_superpoint_heads_typed(LinetrHandle* h, const void* d_score_logits, const void* d_desc_raw, int32_t in_type, int32_t B,
                                  int32_t Hc, int32_t Wc, float* d_dense_score, void* d_dense_desc_nhwc, void* d_dense_desc_nchw,
                                  int32_t out_type, void* stream);

/* ---- SuperPoint key-point branch (models/superpoint.py:48-93, 168-187, 195-197) ---------------------- */

/* Non-maximum suppression, threshold, border filter, optional top-k and (x, y) conversion for a batch of score maps, on the device:
 * simple_nms(scores, nms_radius); nonzero(scores > keypoint_threshold); remove_borders; top_k_keypoints; flip to (x, y).
 * d_dense_score [B,H,W].  Image b's key points lie at rows d_cu_kp[b] .. d_cu_kp[b+1] of d_keypoints [B*cap_per_image,2] (x, y) and
 * d_scores [B*cap_per_image], in the reference's order: row-major (torch.nonzero) without a top-k or for an image with no more than
 * max_keypoints candidates, otherwise by descending score, equal scores by ascending row-major index (a stable descending sort).
 * Key points and scores are bit-identical to the reference's (compares, selects and copies only).  d_found[b] = the image's
 * candidates before the top-k, never capped: an image with d_found[b] > cap_per_image has been truncated to its first
 * cap_per_image candidates -- nothing is written past the capacity, the call still returns 0, and the caller repeats it with a
 * larger one.  nms_radius 0..8; max_keypoints -1 (all) or 1..4096; keypoint_threshold >= 0; other values: LINETR_E_ARG.
 * Asynchronous on `stream`; nothing inside allocates or waits.  `h` may be NULL (no weights involved; current HIP device).
 * The query answers 0 for H W or B H beyond 2^31 - 1, which the entry point refuses. */
int64_t linetr_superpoint_keypoints_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t cap_per_image);
int linetr_superpoint_keypoints(LinetrHandle* h, const float* d_dense_score, int32_t B, int32_t H, int32_t W, int32_t nms_radius,
                                float keypoint_threshold, int32_t remove_borders, int32_t max_keypoints, int32_t cap_per_image,
                                float* d_keypoints, float* d_scores, int32_t* d_cu_kp, int32_t* d_found, void* d_workspace,
                                int64_t workspace_bytes, void* stream);

/* sample_descriptors (models/superpoint.py:81-93) for the packed key points of a batch: bilinear lookup in image b's map for the
 * rows d_cu_kp[b] .. d_cu_kp[b+1] of d_keypoints [n_total,2], L2-normalised, stored in the reference's layout: image b owns a
 * contiguous [256, n_b] block at float offset 256 * d_cu_kp[b] of d_desc_cn.  d_dense_desc is [B,Hc,Wc,256] (dense_is_nhwc = 1,
 * sampled in place) or [B,256,Hc,Wc] (transposed into the workspace first).  Same sampler and `align_corners` as
 * linetr_sample_descriptors.  Asynchronous on `stream`; `h` may be NULL.  A channel-last map and d_workspace must be 16-byte aligned
 * (LINETR_E_ARG otherwise); d_keypoints, d_desc_cn and an NCHW map may lie anywhere. */
int64_t linetr_point_descriptors_workspace_bytes(int32_t B, int32_t Hc, int32_t Wc, int32_t dense_is_nhwc);
int linetr_point_descriptors(LinetrHandle* h, const float* d_keypoints, const int32_t* d_cu_kp, int32_t B, int64_t n_total,
                             const void* d_dense_desc, int32_t Hc, int32_t Wc, int32_t align_corners, int32_t dense_is_nhwc,
                             float* d_desc_cn, void* d_workspace, int64_t workspace_bytes, void* stream);

/* linetr_superpoint_heads for channel-last raw head outputs: d_score_rows [B*Hc*Wc][ld_score >= 65] and d_desc_rows
 * [B*Hc*Wc][ld_desc >= 256] (row strides in floats), cell (b, h, w) at row (b Hc + h) Wc + w -- what linetr_sp_encoder_forward writes.
 * Same three outputs, same rules; the softmax / normalisation body is the same code, so given the same values the two entry
 * points give the same bits.  A row stride below the row's length: LINETR_E_ARG.  The rows are read float by float and may lie anywhere;
 * the outputs must be 16-byte aligned as for linetr_superpoint_heads. */
int linetr_superpoint_heads_rows(LinetrHandle* h, const float* d_score_rows, int64_t ld_score, const float* d_desc_rows, int64_t ld_desc,
                                 int32_t B, int32_t Hc, int32_t Wc, float* d_dense_score, float* d_dense_desc_nhwc,
                                 float* d_dense_desc_nchw, void* stream);

/* ---- homography views (dataloaders/build_homography_dataset.py:164-167, 179-184; dataloaders/utils/utils.py:317-351, 677-704) ------- */

/* d_dst[b, c, y, x] = d_src[b, c] sampled at the source position of destination pixel (x, y), for contiguous float32 [B,C,H,W] tensors
 * (C >= 1).  h_mat: B row-major 3x3 float64 matrices on the HOST, read before the call returns; matrix b maps the destination pixel
 * (x, y, 1) to (x', y', w') and the source position is (x' / w', y' / w'), in PIXEL coordinates (pixel centres at the integers).
 *   mode 0  bilinear with zero padding: F.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=True) read in pixel units.
 *           Taps at floor(x), floor(x) + 1 and the same in y; a tap outside the image contributes 0.
 *   mode 1  nearest: the pixel at nearbyint (half to even) of the position, 0 where that lies outside the image.
 * The position is computed per pixel in float64 (one reciprocal of w'), the four weights in float64 and rounded once, products and sums
 * in float32.  A non-finite position (w' == 0, overflow) gives 0; a finite one with negative w' is sampled like any other.  The
 * position is clamped to [-2, extent + 1] before it becomes an integer, which changes no result.
 * d_valid: NULL or uint8 [B,H,W], written by the same launch whatever the mode: 1 where the nearest source pixel lies inside the image,
 * else 0 (compute_valid_mask at erosion_radius = 0).
 * One launch per 32 images (their matrices travel in the kernel's arguments); no atomics, the same call gives the same bits; nothing is
 * read or written outside the tensors.  Asynchronous on `stream`; nothing inside allocates or waits; `h` may be NULL.
 * linetr_warp_tile: the spatial tiles of the two kernels in pixels (the unit tests walk their edges).
 * LINETR_E_ARG, nothing launched, no output changed: a NULL d_src / d_dst / h_mat, B, C, H or W below 1, H or W above 32 768, H W C at or
 * beyond 2^31, a mode other than 0 or 1, a non-finite matrix entry, d_dst == d_src, a float pointer that is not 4-byte aligned. */
int linetr_warp_images(LinetrHandle* h, const float* d_src, int32_t B, int32_t C, int32_t H, int32_t W, const double* h_mat, int32_t mode,
                       float* d_dst, uint8_t* d_valid, void* stream);
int linetr_warp_tile(int32_t* tile_h, int32_t* tile_w, int32_t* erode_tile_h, int32_t* erode_tile_w);

/* Binary erosion of a uint8 [B,H,W] mask (non-zero = set; the output holds 0 / 1) by the (2 radius + 1)^2 square of ones.  Pixels outside
 * the image count as set: cv2.erode's default border, scipy.ndimage.binary_erosion(border_value=1).  radius 2 is the dataset builder's
 * cv2.erode(mask, np.ones((5, 5))) (build_homography_dataset.py:183-184); radius 0 copies.  One launch, a separable AND over a tile plus
 * halo in LDS.  LINETR_E_ARG, nothing launched: a NULL pointer, B (above 65 535), H or W (above 32 768) below 1, H W at or beyond 2^31,
 * radius outside 0 .. 8, d_out overlapping d_mask. */
int linetr_mask_erode(LinetrHandle* h, const uint8_t* d_mask, int32_t B, int32_t H, int32_t W, int32_t radius, uint8_t* d_out, void* stream);

/* ---- photometric augmentation (dataloaders/build_homography_dataset.py:105-121, 154-158; dataloaders/utils/photometric.py) ----------- */

/* The distortions of the dataset builder for batches of float32 grey images, seeded and deterministic: ImgAugTransform followed by
 * customizedTransform, the same stages in the same order with the same 0..255 quantisation between them.  linetr_amd/csrc/lt_photometric.h
 * is the contract (every stage down to its operation order, the Philox counter layout, the deviations from imgaug / OpenCV);
 * tests/photometric_reference.py restates it in NumPy float64.  Stage bits of LinetrPhotoParams.stages / LinetrPhotoConfig.stages: */
#define LINETR_PHOTO_BRIGHTNESS 1
#define LINETR_PHOTO_CONTRAST 2
#define LINETR_PHOTO_NOISE 4
#define LINETR_PHOTO_IMPULSE 8
#define LINETR_PHOTO_MOTION 16
#define LINETR_PHOTO_BLUR 32
#define LINETR_PHOTO_SHADE 64
#define LINETR_PHOTO_MAX_K 7
#define LINETR_PHOTO_MAX_KSIZE 351
#define LINETR_PHOTO_MAX_ELLIPSES 20

/* The ranges of homography.yaml's augmentation.photometric.params (a stage whose bit is clear is never drawn as enabled). */
typedef struct LinetrPhotoConfig {
  int32_t stages;              /* LINETR_PHOTO_* of the primitives the configuration has */
  int32_t max_abs_change;      /* random_brightness: d uniform on the integers -max .. max; 0 .. 255 */
  double strength_range[2];    /* random_contrast: alpha uniform in [lo, hi) */
  double stddev_range[2];      /* additive_gaussian_noise: sigma uniform in [lo, hi), in levels */
  double prob_range[2];        /* additive_speckle_noise: p uniform in [lo, hi), inside 0 .. 1; thr = floor(p 2^32) */
  int32_t max_kernel_size;     /* motion_blur: applied with probability 1/2 with an odd K uniform on 3 .. max; 3 .. 7 */
  int32_t nb_ellipses;         /* additive_shade: 0 .. 20 */
  double blur_sigma;           /* GaussianBlur: sigma > 0; ksize by imgaug's rule (2.6 / 3.3 / 5.21 sigma below 3 / below 5 / above, at least 5, made odd) */
  double transparency_range[2];/* additive_shade: t uniform in [lo, hi) */
  int32_t kernel_size_range[2];/* additive_shade: ksize uniform on the integers lo .. hi - 1, made odd by + 1; the result within 1 .. 351 */
} LinetrPhotoConfig;

/* One image's drawn values: what the device call reads.  A field of a stage whose bit is clear is ignored but must still be valid. */
typedef struct LinetrPhotoParams {
  int32_t stages;              /* LINETR_PHOTO_* */
  int32_t d;                   /* brightness, -255 .. 255 */
  double alpha;                /* contrast */
  double sigma;                /* noise, >= 0 */
  uint32_t thr;                /* impulse threshold on a 32-bit word */
  int32_t K;                   /* motion kernel extent: 1, 3, 5 or 7 */
  float weights[49];           /* the K x K kernel row-major in the first K K entries */
  int32_t blur_ksize;          /* stage 6: odd, 1 .. 351 */
  double blur_sigma;           /* stage 6: >= 0; 0 = 0.3 ((ksize - 1) / 2 - 1) + 0.8 */
  int32_t n_ellipses;          /* 0 .. 20 */
  double ellipse[20][6];       /* cx, cy, ax, ay, c, s: centre, half axes (> 0), cosine and sine of the rotation */
  double t;                    /* shade transparency */
  int32_t shade_ksize;         /* odd, 1 .. 351 */
} LinetrPhotoParams;

/* linetr_photometric_sample: HOST only.  Fills h_params[0 .. B) for the images first .. first + B - 1 of an H x W batch from Philox4x32-10
 * with key (seed, image) and counter (n, 0, 0, 1); u(n, 0) / u(n, 1) are the 53-bit uniforms of words 0, 1 / 2, 3 of call n:
 *   n = 0: d = floor(u0 (2 max + 1)) - max; alpha.   n = 1: sigma; p.   n = 2: motion iff u0 < 1/2; K = 3 + 2 floor(u1 ((max - 3) / 2 + 1)).
 *   n = 3: theta = pi u0; weights[i][j] = max(0, 1 - |cos(theta) (i - K / 2) - sin(theta) (j - K / 2)|), normalised in float64, rounded once.
 *   n = 4: t; shade ksize.   n = 5 + 3 e, 6 + 3 e, 7 + 3 e for ellipse e: (ax, ay) = int(max(u min_dim, min_dim / 5)) with min_dim = min(H, W) / 4;
 *   (cx, cy) = max_rad + floor(u (extent - 2 max_rad)) with max_rad = max(ax, ay); angle = 90 u0 degrees.
 * Every range is lo + u (hi - lo).  The reference's randint(max_rad, extent - max_rad) cannot raise for any extent (2 max_rad <= min(H, W) / 2),
 * but below min(H, W) = 20 an axis can become 0, which the analytic ellipse does not define: LINETR_E_ARG there when the shade is configured.
 * LINETR_E_ARG also: NULL pointers, B, H or W below 1, first < 0, a seed beyond 32 bits, a range outside the above or with hi < lo.
 *
 * linetr_photometric: d_dst[b] = the stages of h_params[b] applied to d_src[b], float32 [B,1,H,W] in [0,1] in and out (an input outside
 * [0,1] is clamped by stage 0).  Image b draws its per-pixel randomness with key (seed, first + b): a batch gives each image the bits it
 * gets alone.  quantise_out = 1: floor of the shaded level (see the contract).  h_params is read before the call returns (it travels in the
 * arguments of one small launch per 3 images; no host buffer has to outlive the call).  Asynchronous on `stream`; nothing inside allocates,
 * waits or uses atomics; the same call gives the same bits; `h` may be NULL.
 * linetr_gaussian_blur: stage 6 alone on float32 [B,C,H,W] of any values: per image an odd h_ksize[b] in 1 .. 351 and h_sigma[b] >= 0
 * (0 = OpenCV's rule); quantise = 1 rounds the result to levels 0..255, 0 leaves the float32 sums.
 * linetr_photometric_workspace_bytes: the bytes both calls need for [B,C,H,W] (C = 1 for linetr_photometric), 0 for a shape they refuse.
 * linetr_photometric_tile: tile (rows, columns) and halo of the point kernel, strip (rows, columns) of the row pass, tile (rows, columns) of
 * the column pass and the largest blur radius (the unit tests walk their edges).
 * LINETR_E_ARG, nothing launched, no output changed: a NULL pointer; B, C, H or W below 1, B C above 65 535, H or W above 32 768, H W C at or
 * beyond 2^31; a seed beyond 32 bits, first < 0 or first + B beyond 2^31; unknown stage bits; an even ksize or one outside 1 .. 351; K outside
 * {1, 3, 5, 7}; n_ellipses outside 0 .. 20; d outside -255 .. 255; a non-finite parameter, a negative sigma, ax or ay <= 0; quantise_out /
 * quantise other than 0 or 1; d_dst == d_src; a tensor that is not 4-byte or a workspace that is not 256-byte aligned.
 * LINETR_E_WORKSPACE, nothing launched: a workspace shorter than linetr_photometric_workspace_bytes says. */
int linetr_photometric_sample(const LinetrPhotoConfig* cfg, uint64_t seed, int32_t first, int32_t B, int32_t H, int32_t W,
                              LinetrPhotoParams* h_params);
int64_t linetr_photometric_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int linetr_photometric(LinetrHandle* h, const float* d_src, int32_t B, int32_t H, int32_t W, const LinetrPhotoParams* h_params, uint64_t seed,
                       int32_t first, int32_t quantise_out, float* d_dst, void* d_workspace, int64_t workspace_bytes, void* stream);
int linetr_gaussian_blur(LinetrHandle* h, const float* d_src, int32_t B, int32_t C, int32_t H, int32_t W, const int32_t* h_ksize,
                         const double* h_sigma, int32_t quantise, float* d_dst, void* d_workspace, int64_t workspace_bytes, void* stream);
int linetr_photometric_tile(int32_t* tile_h, int32_t* tile_w, int32_t* halo, int32_t* row_tile_h, int32_t* row_tile_w, int32_t* col_tile_h,
                            int32_t* col_tile_w, int32_t* max_radius);

/* ---- line segment detector (the surface of models/line_detector.py:11-28; NOT OpenCV's LSD) ------------------------------------------ */

/* A detector of the LSD / Burns family whose every step is independent of any processing order (DESIGN.md 4.18 has the algorithm down to
 * its integer arithmetic; tests/line_detector_reference.py restates it in NumPy).  Pixel centres sit at the integers.  Per octave: the
 * image is smoothed by [1 2 1] x [1 2 1] (reflect-101, kept times 16), the gradient (gx, gy) is taken on every 2 x 2 cell, a cell is used
 * iff gx^2 + gy^2 >= grad_threshold, its orientation is put into one of eight buckets twice (partition A: boundaries at multiples of 45
 * degrees; partition B: at 22.5 degrees + multiples of 45), regions are the 8-connected components of used cells with the same bucket, every
 * cell votes for the partition in which its region is larger (A on a tie), a region with size >= min_region_size and 2 * votes > size is
 * fitted through its gradient-weighted integer moments (float64), and kept if its rectangle is filled to at least `density`.
 * Octave o + 1 is octave o under the separable [1 4 6 4 1] kernel, (sum + 128) >> 8, even rows and columns. */
typedef struct LinetrDetectConfig {
  int32_t n_octaves;        /* 1 .. 12; an octave below 2 x 2 pixels yields no lines */
  int32_t scale;            /* 2, nothing else */
  int32_t grad_threshold;   /* >= 1; 28160 = LSD's rho = 2 / sin 22.5 deg on the 2 x 2 norm, at this scale */
  int32_t min_region_size;  /* >= 4 (the candidate tables hold Nc / 4 regions per partition); 16 */
  double density;           /* 0 .. 1; 0.6 */
} LinetrDetectConfig;

/* d_images: [B][H][W] on the device, uint8 (images_are_float = 0) or float32 in [0,1] (1; quantised as uint8(v * 255): float32 multiply,
 * truncation, clamped to 0..255).  d_rows: float64 [B][capacity][6] rows (startX, startY, endX, endY, lineLength, octave) as
 * linetr_prefilter_batch takes them: end points in pixels of the input image, lineLength in pixels of the line's octave.  Per image the rows
 * are ordered by octave, then partition A before B, then by the region's smallest cell index.  h_counts: int32 [B][n_octaves] in PINNED host
 * memory, the true number of lines per image and octave, copied there by the stream; rows beyond `capacity` are not written (call again with
 * more).  d_debug_regions: NULL or int64 [B][capacity][10], for row r: octave, partition, label, n, sum w, sum wx, sum wy, sum wxx, sum wxy,
 * sum wyy.  Integer atomics and min / max only: two calls give the same bytes.  Asynchronous on `stream`; nothing inside allocates or waits;
 * `h` may be NULL.  linetr_detect_tile: the tile of the gradient and labelling kernels in cells (the unit tests walk its edges).
 * LINETR_E_ARG, nothing launched: B outside 1 .. 32 767, H or W outside 1 .. 2048, a config outside the ranges above, a NULL d_images /
 * cfg / d_rows / h_counts / d_workspace, capacity below 0, a workspace shorter than linetr_detect_lines_workspace_bytes (0 for extents that
 * would be refused), misaligned rows (float32 images 4, d_rows and d_debug_regions 8, h_counts 4, the workspace 256 bytes). */
int64_t linetr_detect_lines_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t n_octaves);
int linetr_detect_lines(LinetrHandle* h, const void* d_images, int32_t images_are_float, int32_t B, int32_t H, int32_t W,
                        const LinetrDetectConfig* cfg, int32_t capacity, double* d_rows, int32_t* h_counts, int64_t* d_debug_regions,
                        void* d_workspace, int64_t workspace_bytes, void* stream);
int linetr_detect_tile(int32_t* tile_h, int32_t* tile_w);

/* Parts of the detector alone, for the unit tests.
 * linetr_detect_debug_labels: the three labelling kernels on caller-provided bucket maps, int8 [B][H][W] with -1 = unused (H x W counts
 * cells here, 1 .. 2048 each; B up to 65 534): d_labels int32 [B][H][W] = the smallest linear index y * W + x of the cell's region, -1 for an
 * unused cell.  Workspace: linetr_detect_debug_labels_workspace_bytes.
 * linetr_detect_debug_gradient: quantisation, pyramid and gradient kernel up to `octave`: d_m2 int32 and both bucket maps int8 (-1 =
 * unused), each [B][Ho - 1][Wo - 1] for the octave's Ho x Wo pixels; nothing is written for an octave below 2 x 2.  Workspace as for
 * linetr_detect_lines.  Refusals as above. */
int64_t linetr_detect_debug_labels_workspace_bytes(int32_t B, int32_t H, int32_t W);
int linetr_detect_debug_labels(LinetrHandle* h, const int8_t* d_buckets, int32_t B, int32_t H, int32_t W, int32_t* d_labels, void* d_workspace,
                               int64_t workspace_bytes, void* stream);
int linetr_detect_debug_gradient(LinetrHandle* h, const void* d_images, int32_t images_are_float, int32_t B, int32_t H, int32_t W,
                                 const LinetrDetectConfig* cfg, int32_t octave, int32_t* d_m2, int8_t* d_bucket_a, int8_t* d_bucket_b,
                                 void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- native SuperPoint encoder (models/superpoint.py:113-134, 148-160, 188-189) ---------------------- */

/* Inference only, float32 in and out, channel-last inside, deterministic (a fixed summation order; no atomics).  OFF by default at every
 * level above this header (Engine.superpoint_encode, FusedHeadSuperPoint(native_encoder=True), Matching's config['native_encoder']).
 *
 * One 3x3 layer alone, on channel-last tensors: y = [maxpool2x2](relu(conv3x3(x, stride 1, zero padding 1) + bias)).
 *   d_x [B,H,W,Cin] -> d_y [B,H,W,Cout], or [B,H/2,W/2,Cout] with pool = 1 (floors like nn.MaxPool2d(2, 2): an odd last row or column is
 *   computed and dropped; H or W = 1 gives an empty output and launches nothing).  Exact-fp32 MFMA, fp32 accumulation.
 *   (Cin, Cout): (64,64) (64,128) (128,128) (128,256) and (128,512) = convPa | convDa as one layer.
 *   d_packed_w: the state_dict weight [Cout,Cin,3,3] re-ordered ONCE by linetr_sp_conv3x3_pack into the K order the kernel walks
 *   (linetr_sp_conv3x3_pack_bytes bytes; 0 for an unsupported pair):
 *       packed[(((c / 32) * 9 + 3 ky + kx) * 4 + (c % 32) / 8) * Cout + n][c % 8] = w[n][c][ky][kx]
 *   linetr_sp_conv3x3_tile: the kernel's spatial tile in pixels (the unit tests walk its edges).
 * linetr_sp_conv1a: the first layer (Cin = 1, no GEMM): gray image d_image [B,1,H,W] -> d_y [B,H,W,64], d_w [64,1,3,3] and d_bias [64] in
 * state_dict layout, bias + ReLU.
 * All asynchronous on `stream`; nothing inside allocates or waits; `h` may be NULL.  LINETR_E_ARG, nothing launched, no output changed:
 * B < 1 (or above 65 535), H or W below 1 (or above 32 768), a (Cin, Cout) outside the set, pool outside 0 .. 1, a pointer that is NULL
 * or not 16-byte aligned. */
int linetr_sp_conv3x3_tile(int32_t* tile_h, int32_t* tile_w);
int64_t linetr_sp_conv3x3_pack_bytes(int32_t Cin, int32_t Cout);
int linetr_sp_conv3x3_pack(const float* d_w, int32_t Cin, int32_t Cout, float* d_packed, void* stream);
int linetr_sp_conv3x3(LinetrHandle* h, const float* d_x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* d_packed_w,
                      const float* d_bias, int32_t Cout, int32_t pool, float* d_y, void* stream);
int linetr_sp_conv1a(LinetrHandle* h, const float* d_image, int32_t B, int32_t H, int32_t W, const float* d_w, const float* d_bias,
                     float* d_y, void* stream);

/* The whole encoder: conv1a .. conv4b with the three poolings, convPa | convDa as one launch, then the two 1x1 heads convPb / convDb
 * (the same implicit-GEMM kernel with one tap; convPb's 65 outputs are padded with zero weights to its 128-channel tile and the
 * padding is never stored).  11 launches for a batch.
 *   linetr_sp_encoder_create        allocates the packed-weight arena on `device` (the only allocation of the encoder's life)
 *   linetr_sp_encoder_set_weights   d_weights[12] / d_biases[12]: HOST arrays of device pointers in state_dict layout and order --
 *                                   conv1a conv1b conv2a conv2b conv3a conv3b conv4a conv4b convPa convPb convDa convDb; packs them
 *                                   asynchronously on `stream` (a forward on the same stream sees them); may be called again
 *   linetr_sp_encoder_forward       d_image [B,1,H,W] -> d_score_rows [B*Hc*Wc][LINETR_SP_SCORE_LD] (convPb, raw logits in columns 0..64;
 *                                   the row stride of 68 floats keeps every row, and so every image's block, 16-byte aligned; columns
 *                                   65..67 are never written) and d_desc_rows [B*Hc*Wc][256] (convDb, raw): the rows
 *                                   linetr_superpoint_heads_rows takes, Hc = H / 8, Wc = W / 8 (floor at every pooling); d_feat (or NULL) [B,Hc,Wc,128] = conv4b's output, for the tests.  Asynchronous on `stream`;
 *                                   nothing inside allocates or waits.
 * LINETR_E_ARG, nothing launched, no output changed: a NULL encoder or one without weights, B < 1 (or above 65 535), H or W below 8 (or
 * above 32 768), a required pointer that is NULL or not 16-byte aligned (d_feat: misaligned), a workspace smaller than
 * linetr_sp_encoder_workspace_bytes says.  The query answers 0 for a B, H or W outside those ranges. */
#define LINETR_SP_SCORE_LD 68
typedef struct LinetrSpEncoder LinetrSpEncoder;
int linetr_sp_encoder_create(int32_t device, LinetrSpEncoder** out);
void linetr_sp_encoder_destroy(LinetrSpEncoder* enc);
int linetr_sp_encoder_set_weights(LinetrSpEncoder* enc, const float* const* d_weights, const float* const* d_biases, void* stream);
int64_t linetr_sp_encoder_workspace_bytes(int32_t B, int32_t H, int32_t W);
int linetr_sp_encoder_forward(LinetrSpEncoder* enc, const float* d_image, int32_t B, int32_t H, int32_t W, float* d_score_rows,
                              float* d_desc_rows, float* d_feat, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- arithmetic mode of the dense contractions ----------------------------------------------------- */

/* All Linear/Conv1d(k=1) contractions run on one of three MFMA paths (fp32 in, fp32 accumulate, fp32 out):
 *   LINETR_PREC_F32     v_mfma_f32_32x32x2_f32, exact fp32 products                (157 TF ceiling)
 *   LINETR_PREC_BF16X6  operands split into 3 bf16 planes, 6 cross products: fp32-faithful (~2^-23 per
 *                       product, same class as fp32 summation-order noise)          (417 TF-equivalent)
 *   LINETR_PREC_BF16X3  2 planes, 3 cross products: ~1e-5 relative per product      (833 TF-equivalent)
 *   LINETR_PREC_F16X3   2 fp16 planes (22 significand bits), 3 cross products: ~2^-22 per product, i.e. fp32-class
 *                       (measured 1.1e-6 on the descriptors vs 4.4e-7 for BF16X6), but every GEMM operand must
 *                       stay below 65504 in magnitude (fp16 range)                  (833 TF-equivalent)
 * Default: LINETR_PREC_BF16X6, overridable with the environment variable LINETR_PRECISION=f32|bf16x6|bf16x3|f16x3
 * at linetr_create time.  The signature attention's two contractions (S^T = K Q^T and O^T = V^T P^T) follow the mode as well: exact
 * fp32 MFMA in LINETR_PREC_F32, the six-product bf16 split (fp32-faithful) in the three split modes; its softmax, the token sampler,
 * the pooling, LayerNorm / L2 normalisation and every other non-GEMM stage are fp32 in all modes.  The matcher's distance products
 * are exact fp32 MFMA in all modes (an argmin must not inherit a split's error). */
enum { LINETR_PREC_F32 = 0, LINETR_PREC_BF16X3 = 1, LINETR_PREC_BF16X6 = 2, LINETR_PREC_F16X3 = 3 };
int linetr_set_precision(LinetrHandle* h, int32_t mode);
int linetr_get_precision(const LinetrHandle* h);

/* ---- diagnostics ---------------------------------------------------------------------------- */

/* Runs layers 1-3 of a positional encoder (MLP of models/line_transformer.py:9-20, BN folded, ReLU) alone, for the
 * unit tests: which = 0 WordPositionalEncoder (line_transformer.py:52-73; d_in0 = token points [rows,2] in pixels,
 * d_in1 = token scores [rows], d_in2 unused), which = 1 LinePositionalEncoder (:40-50; d_in0 = sub-lines [rows,2,2] in
 * pixels, d_in1 = resp [rows], d_in2 = angles [rows,2]).  d_out [rows,128] = activations after the third ReLU.
 * Coordinates are normalised with the handle's image_shape as in normalize_keylines (:22-38). */
int linetr_debug_posenc(LinetrHandle* h, int32_t which, const float* d_in0, const float* d_in1, const float* d_in2,
                           int64_t rows, float* d_out, void* stream);

/* Runs the library's fp32-MFMA GEMM  Y[M,N] = act(A[M,K] W[N,K]^T + bias) (+ R)  on device buffers; used
 * by the unit tests (vs a plain PyTorch fp32 reference) and by the kernel micro-benchmarks.  act: 0 none,
 * 1 ReLU, 2 erf-GELU, 3 max(2-2x,0).  d_bias / d_residual may be NULL.  N % 64 == 0, K % 32 == 0.
 * lda / ldy are the row strides of A and Y (and of the residual) in floats, multiples of 4.
 * cache_weights != 0 keeps the split-bf16 copy of d_W (keyed by pointer) for later calls, so repeated
 * calls time the GEMM kernel alone; the caller then promises not to change the contents of d_W. */
int linetr_debug_gemm(LinetrHandle* h, const float* d_A, int32_t lda, const float* d_W, const float* d_bias,
                      const float* d_residual, float* d_Y, int32_t ldy, int32_t M, int32_t N, int32_t K,
                      int32_t act, int32_t cache_weights, void* stream);

/* Runs ONE kernel of the GEMM family on everything the forward pass can ask of it, for the unit tests
 * (tests/test_gpu_gemm_tiles.py: every tile against float64 at its tile edges):
 *     Y_g[M,N] = norm( act([A_g | A2_g] W_g^T + bias_g) (+ R) ) (+ add2),   g = 0 .. groups - 1
 * A [M][K1] (K1 = K without A2) and A2 [M][K - K1] with row strides lda / lda2; W [groups * N][K] and bias [groups * N] (or
 * NULL) contiguous; R (or NULL) and Y with row stride ldy.  Group g reads A + g gA and A2 + g gA and writes Y + g gY (gA = 0: all
 * groups share A); a grouped launch takes no R and no norm.  act as in linetr_debug_gemm.  norm: 0 none, 1 LayerNorm(x) gamma +
 * beta with eps inside the sqrt, 2 x / max(||x||_2, 1e-12), applied after bias, activation and residual, then + add2 (row stride
 * 256, or NULL); needs N = ldy = 256.  The normalisation runs in the tile's epilogue, or -- via_row_norm != 0, or tile = -1 where
 * the dispatcher's tile does not own whole rows -- the product goes to a scratch buffer and row_norm_kernel writes Y.
 * tile: -1 = what the forward pass takes for this problem at the handle's precision (the choice is made by the same host function
 *       the forward pass calls.  Two differences: the experiments library's own launch hooks -- stream-K, the row-owner GEMM --
 *       are not consulted here, and a 128 -> 256 weight always gets a split-tile image here, while in the forward pass only
 *       the weights created with one can take the weight-stationary kernel); LINETR_GEMM_TILE_WS = the weight-stationary kernel; otherwise an index into the tile names,
 *       split modes: 0 32x32k4, 1 112x256, 2 128x64, 3 256x128, 4 128x256, 5 64x256, 6 128x128, 7 128x128s, 8 256x256, 9 64x64,
 *                    10 64x128;          f32 mode: 0 128x64, 1 128x128, 2 64x128.
 * *tile_used (may be NULL) receives the kernel that launches, after the launchers' own fallback rules: N % 128 != 0 takes 128x64,
 * a 256-wide tile on N % 256 != 0 takes 64x128, and so does 256x256 (built in the experiments library's two-plane modes only).
 * Refused with LINETR_E_ARG, nothing launched: a normalisation asked of the epilogue of anything but 128x256 with N = 256; the
 * weight-stationary kernel for anything but act(A[M,128] W[256,128]^T + bias), act none / ReLU, bf16x6, one group, no A2 / R / norm;
 * 112x256 with groups; K1 not a multiple of 32; strides that are not multiples of 4 floats, misaligned (16 bytes) tensors.
 * With A = W = Y = NULL only the choice (and any refusal) is reported and nothing is launched or dereferenced: A2 and R then only
 * say whether the operand is there.  Per-call scratch (the split copies of W) is freed after synchronising `stream`. */
#define LINETR_GEMM_TILE_WS 100
typedef struct {
  const float* A;   int32_t lda;
  const float* A2;  int32_t lda2;  int32_t K1;
  const float* W;
  const float* bias;
  const float* R;
  float* Y;         int32_t ldy;
  int32_t M, N, K, act;
  int32_t groups;   int64_t gA, gY;
  int32_t norm;     const float* gamma;  const float* beta;  const float* add2;  float eps;
  int32_t via_row_norm;
  int32_t tile;
} LinetrGemmCase;
int linetr_debug_gemm_case(LinetrHandle* h, const LinetrGemmCase* c, int32_t* tile_used, void* stream);

/* Runs ONE signature-attention kernel (models/line_transformer.py:132-154 up to, not including, the merge conv) on a
 * var-len batch, for the unit tests (tests/test_gpu_attention.py: every kernel against a float64 reference).
 * kernel: -1 = what the forward pass takes for this handle's precision, n_images, N = h_cu_sub[n_images] and the largest
 *              image max_n (the choice is made by the same host function the forward pass calls), reported in *kernel_used;
 *          0 sig_attn_kernel (exact fp32 MFMA)          -- taken in f32 mode
 *          1 sig_attn_small_kernel (32-query blocks, the 4 waves split the KV range) -- n_images * 4 * ceil(max_n / 256) < 64
 *          2 sig_attn_split_kernel<4>                   -- otherwise, max_n <= 128
 *          3 sig_attn_split_kernel<8>                   -- otherwise, max_n > 128
 *          4 sig_qkv_attn_kernel (projection + attention fused) -- bf16x6, max_n <= 256, n_images * 4 >= 128, not the
 *                                                          folded single-pair path (small kernel and N <= 960)
 *          4 + LINETR_SIG_EIGHT_WAVES (36): kernel 4 in its eight-compute-wave form whatever the size.  Kernel 4 itself runs
 *            images of up to 224 sub-lines (max_n <= 224) with seven row-owning waves and the eighth as the operand ring's only
 *            DMA issuer, and max_n 225 .. 256 with eight row-owning waves that each issue their share; both forms give the same
 *            bits.  Forced only -- never the dispatcher's choice, never reported for kernel = -1 -- and reported back in
 *            *kernel_used as 36.  Everything said of kernel 4 below holds for it.  (5 .. 35 stay refused.)
 * kernel 0-3: d_in = q/k/v rows [N][ld_in], head-major (q at column h*64 + d, k at 256 +, v at 512 +), q pre-scaled by 1/8 as
 *             the library's projection weights make them.  ld_in = 768; 1024 is legal for kernel 1 only (q/k/v behind x_out,
 *             the folded single-pair layout: d_in points at q, i.e. at column 256 of the [N][1024] rows).  `layer` is not read.
 *             A forced kernel 0-3 runs whatever the handle's precision is, and each is correct for every max_n: kernels 2 and
 *             3 walk all KV tiles of an image and spread its queries over ceil(max_n / 128) resp. ceil(max_n / 256) blocks.
 * kernel 4:   d_in = z rows [N][256] (ld_in = 256); q/k/v are projected inside the kernel with signature layer `layer`'s weights.
 * d_msg [N][256] head-major (c' = h*64 + d), i.e. what the kernels write BEFORE the merge conv (folded into the next GEMM).
 * A forced kernel is launched exactly as the forward pass launches it.  Refused with LINETR_E_ARG, nothing launched: kernel 4
 * with max_n > 256, a precision other than bf16x6, `layer` out of range or ld_in != 256; ld_in other than 768 (1024: kernel 1)
 * for kernels 0-3; a training-mode handle; misaligned (16 bytes) or NULL tensors.  With kernel = -1 and d_in = d_msg = NULL
 * only the choice is reported and nothing is launched.  kernel_used may be NULL.  Synchronises `stream` before returning. */
enum { LINETR_SIG_EIGHT_WAVES = 32 };
int linetr_debug_sig_attention(LinetrHandle* h, int32_t kernel, int32_t layer, const float* d_in, int32_t ld_in,
                               const int32_t* h_cu_sub, int32_t n_images, float* d_msg, int32_t* kernel_used, void* stream);

/* Runs ONE launch of the positional encoders' MLP up to its fourth ReLU (models/line_transformer.py:9-20, 40-73 without the last
 * linear layer; BatchNorm folded) alone, for the unit tests (tests/test_gpu_front.py: every variant against float64 at its tile
 * edges).  Word encoder: d_pnt [rows_word][2] token coordinates in pixels, d_score [rows_word]; line encoder: d_sublines
 * [rows_line][2][2] end points in pixels, d_resp [rows_line], d_angle [rows_line][2]; coordinates are normalised with the
 * handle's image_shape (normalize_keylines, :22-38).  d_out_word [rows_word][256], d_out_line [rows_line][256].
 * variant: 0 tok_mlp_kernel<word>, 1 tok_mlp_kernel<line>, 2 tok_mlp_dual_kernel (both encoders side by side, one block per
 *          64-row tile), 3 tok_mlp_seq_kernel (every persistent block walks the word encoder's tiles, then the line encoder's),
 *          4 the unfused chain the forward pass falls back to (layers 1-3 in mlp123_kernel, layer 4 through the GEMM dispatcher),
 *          for every encoder that has rows; -1 = what the forward pass takes for these row counts at the handle's precision
 *          (the choice is made by the same host function the forward pass calls): 2 while ceil(rows_word / 64) +
 *          ceil(rows_line / 64) <= compute units, 3 above; 0 / 1 when the other encoder has no rows; 4 outside bf16x6 mode.
 * max_blocks: 0 = the persistent kernels (0, 1, 3) launch one block per compute unit (at most one per tile), as the forward pass
 *          does; > 0 caps that grid, so that a block walks several tiles at a few hundred rows.  Not read by variants 2 and 4.
 * *variant_used (may be NULL) receives what launches.  With variant = -1 and both outputs NULL only the choice is reported and
 * nothing is launched or dereferenced.  An encoder without rows is not launched (variants 0, 1, 4).  Refused with LINETR_E_ARG,
 * nothing launched: variant 2 whose blocks do not fit the chip, variants 2 / 3 with an empty encoder, a training-mode handle,
 * negative sizes, NULL tensors, outputs that are not 16-byte aligned.  Synchronises `stream` before returning. */
int linetr_debug_tok_mlp(LinetrHandle* h, int32_t variant, const float* d_pnt, const float* d_score, int64_t rows_word,
                         const float* d_sublines, const float* d_resp, const float* d_angle, int64_t rows_line,
                         float* d_out_word, float* d_out_line, int32_t max_blocks, int32_t* variant_used, void* stream);

/* Runs BatchNorm1d in TRAINING mode + ReLU (csrc/lt_bntrain.h: bn_partial_kernel, bn_finalize_kernel, bn_apply_kernel behind
 * their host function bn_train_layer) alone, for the unit tests (tests/test_gpu_bn_train.py: against float64 at the channel widths,
 * row strides and row counts where the kernels' loops and chunks end).  `h` must be a training-mode handle (bn_batch_stats = 1).
 * which = -1: ONE free-standing layer, the handle's weights are not read.  d_z [rows][ld] holds C <= ld pre-activations per row and
 *          is transformed in place to max((z - mean) / sqrt(var + 1e-5) gamma + beta, 0), mean and the BIASED variance taken per
 *          channel over all rows; d_gamma, d_beta [C]; d_running [2 C] = mean | var is moved in place to (1 - momentum) old +
 *          momentum (mean | var rows / (rows - 1)) (rows = 1: the variance, 0, as it is); d_batch [2 C] (may be NULL) receives mean |
 *          biased variance; d_affine [2 C] (may be NULL) receives alpha = gamma / sqrt(var + 1e-5) | beta' = beta - mean alpha, the
 *          float32 constants the transform multiplies and adds.  d_in0 / d_in1 / d_in2 / d_out are not read.
 * which = 0 / 1: the word / line positional encoder's four conv + BatchNorm(batch) + ReLU layers on the handle's unfolded weights,
 *          as linetr_forward_train runs them.  First-layer inputs as linetr_debug_tok_mlp's: d_in0 = d_pnt [rows][2], d_in1 =
 *          d_score [rows] (word; d_in2 not read) or d_in0 = d_sublines [rows][2][2], d_in1 = d_resp [rows], d_in2 = d_angle
 *          [rows][2] (line).  d_out [rows][keyline_encoder[3]]; d_running / d_batch (may be NULL) hold the encoder's four layers
 *          packed as linetr_forward_train packs them (2 (e0 + e1 + e2 + e3) floats).  d_z, C, ld, d_gamma, d_beta, d_affine are
 *          not read.
 * *nb_used (may be NULL) receives the number of row chunks the statistics were summed in: min(512, max(1, rows / 64)).
 * d_ws: linetr_debug_bn_train_workspace_bytes(h, which, rows) bytes, 256-byte aligned (-1 on bad arguments).
 * Refused with LINETR_E_ARG, nothing launched: an inference handle; C outside 4 .. 512 or no multiple of 4; ld < C or no multiple
 * of 4; d_z / d_out not 16-byte aligned; rows < 0; momentum outside [0, 1]; NULL tensors.  A workspace that is too small is
 * LINETR_E_WORKSPACE.  rows = 0 launches nothing.  Synchronises `stream` before returning. */
int64_t linetr_debug_bn_train_workspace_bytes(const LinetrHandle* h, int32_t which, int64_t rows);
int linetr_debug_bn_train(LinetrHandle* h, int32_t which, float* d_z, int64_t rows, int32_t C, int32_t ld, const float* d_gamma,
                          const float* d_beta, const float* d_in0, const float* d_in1, const float* d_in2, float* d_out,
                          float momentum, float* d_running, float* d_batch, float* d_affine, int32_t* nb_used, void* d_ws,
                          int64_t ws_bytes, void* stream);

/* Runs ONE CLS-row pooling kernel of the descriptive layer (models/line_attention.py:6-75 restricted to query row 0) alone, for
 * the unit tests (tests/test_gpu_front.py).  d_pooled [N][4][544] = per sub-line and head [sum_j p_j desc_j (256) | sum_j p_j
 * a4_j (256) | p_CLS | 31 zeros], the sums over the token keys j >= 1.
 * kernel: 0 cls_pool_kernel (the dense token stage of linetr_forward): reads d_desc_dense [N][T][256] and d_a4 [N*T][256] only;
 *         1 cls_pool_online_kernel<1> (one wave per sub-line), sub-lines in forward order;  2 the same, last sub-lines first;
 *         3 cls_pool_online_kernel<4> (the block's four waves share one sub-line);
 *         -1 = what the forward pass takes: 0 for a dense token stage (d_desc_dense != NULL), otherwise 3 up to 2048
 *         sub-lines and 2 above (the choice is made by the same host function the forward pass calls).
 * Kernels 1-3 get the kernel's own operands, as linetr_describe prepares them: the records d_recs [K] (first_sub, n_tok, n_sub,
 * image and first_tok are read), the sub-line -> key-line map d_sub2line [N], the compact token coordinates d_cpnt [first_pad +
 * n_images][2] and word-encoder activations d_a4 [first_pad + n_images][256], whose row first_pad + i is image i's shared
 * padding token, and the n_images dense descriptor maps d_map of Hc x Wc cells: NHWC, or (dense_is_nhwc = 0) NCHW, which
 * nchw_to_nhwc_kernel first transposes into the call's own scratch.
 * *kernel_used (may be NULL) receives what launches; with d_pooled = NULL only the choice is reported and nothing is launched or
 * dereferenced.  Refused with LINETR_E_ARG, nothing launched: T outside 1 .. 4096, a d_sub2line entry outside [0, K), a sub-line
 * outside its key-line's range or token count, first_tok + n_tok > first_pad, image outside [0, n_images) (records and map are
 * copied to the host for this), NULL or misaligned tensors (16 bytes: d_a4, d_pooled, d_desc_dense, an NHWC map; 8: d_recs),
 * a training-mode handle.  Synchronises `stream` before returning. */
int linetr_debug_cls_pool(LinetrHandle* h, int32_t kernel, const LinetrLineRec* d_recs, int32_t K, const int32_t* d_sub2line,
                          int32_t N, int32_t T, const float* d_cpnt, const float* d_a4, int64_t first_pad, int32_t n_images,
                          const void* d_map, int32_t dense_is_nhwc, int32_t Hc, int32_t Wc, int32_t align_corners,
                          const float* d_desc_dense, float* d_pooled, int32_t* kernel_used, void* stream);

/* Runs ONE path of the descriptor-distance matcher alone, for the unit tests (tests/test_gpu_match_kernels.py: every matcher kernel
 * against float64 at its tile edges).  Operands as linetr_match; the extra arguments choose what launches:
 * path:  0 the three launches (pair_dist_kernel, pair_pool_kernel, pair_final_kernel) -- batches, and single pairs beyond the
 *          one-launch matcher;
 *        1 pair_match_fused_kernel<false> -- one pair, k0, k1 in 1 .. 4096, n1 <= 1024;
 *        2 pair_match_fused_kernel<true>  -- the same with one sub-line per key-line on both sides (n0 = k0, n1 = k1);
 *       -1 what linetr_match takes for these dims (linetr_match, linetr_match_gathered and this entry point run one body).
 * For path 0 only, each -1 (the matcher's own choice) or 0 / 1:
 *   seg1_global   image 1's segment table in the workspace, built by pair_seg1_kernel (the matcher: more than 12000 key-lines in
 *                 an image 1), instead of in the pooling block's LDS;
 *   cache_dk      the pooling block keeps its 16 pooled rows in LDS (the matcher: up to 896 key-lines in every image 1);
 *   device_table  the pair table travels through the pinned staging ring into the workspace (the matcher: more than 8 pairs)
 *                 instead of inside the kernel arguments.
 * *path_used (may be NULL) receives what launched.  With path = -1 and all six tensors NULL only the choice is reported: nothing
 * is launched, queued on the stream or dereferenced but dims (the choice is made from the sizes and the device's LDS alone; the
 * matcher itself falls back to path 0 when no scratch slot is left for the stream, after 256 streams).  A forced path is launched exactly as the matcher launches it: same grid, same
 * LDS size, same scratch slot.  Refused with LINETR_E_ARG, nothing launched and the outputs untouched: path 1 / 2 with P != 1 or
 * sizes beyond the one-launch matcher; path 2 with n0 != k0 or n1 != k1; cache_dk = 1 with a k1 above 896; seg1_global = 0 with a
 * k1 above 12000; device_table = 0 with more than 8 pairs; a switch forced on a path other than 0; bad dims; NULL or misaligned
 * tensors (descriptors and workspace 16 bytes, the others 4).  A forced path 1 / 2 on a device that refuses the kernel's dynamic
 * LDS, or on a stream that gets no scratch slot, is LINETR_E_HIP with its own message -- never the three launches instead.
 * Synchronises `stream` before returning. */
int linetr_debug_match(LinetrHandle* h, int32_t P, const int32_t* dims, const float* d_desc0, const int64_t* off_n0,
                       const int32_t* d_s2l0, const float* d_desc1, const int64_t* off_n1, const int32_t* d_s2l1, float thr,
                       int32_t mutual, float* d_dk, const int64_t* off_dk, int32_t* d_match01, const int64_t* off_k0, void* d_ws,
                       int64_t ws_bytes, int32_t path, int32_t seg1_global, int32_t cache_dk, int32_t device_table,
                       int32_t* path_used, void* stream);

/* Runs ONE stage from the middle of the forward pass alone on the caller's rows, with the handle's (folded) weights and at its
 * precision mode, for the unit tests (tests/test_gpu_stages.py: both stages against float64 references built from the unfolded
 * state dict).  The stage is run by the host functions the forward pass itself calls, in the forward pass's workspace layout.
 * stage LINETR_STAGE_TAIL: the descriptive layer behind the CLS pooling (models/line_attention.py:36-40, 79-83,
 *     models/line_transformer.py:128).  d_in0 = pooled [N][4][544] rows as linetr_debug_cls_pool writes them, d_in1 = line_pos
 *     [N][256].  d_out0 = att [N][256] (the value projection, head-major), d_out1 = o = LN(fc(att) + cls), d_out2 = the sentence
 *     rows line_pos + LN(w_2(gelu(w_1 o)) + o); each may be NULL.  h_cu_sub and n_images are not read; plan must be -1.
 * stage LINETR_STAGE_SIG: the line-signature network, final projection and L2 normalisation (models/line_transformer.py:132-183,
 *     245-246).  d_in0 = the sentence rows z0 [N][256] (copied into the workspace: not written), h_cu_sub [n_images + 1] the images'
 *     prefix sums ending at N, d_in1 not read.  d_out0 = line_desc [N][256]; d_out1 (may be NULL) = taps [L - 1][N][256], x_out
 *     behind the signature layers 0 .. L - 2 of the handle's L (the last layer's x_out exists only inside the final projection);
 *     d_out2 not read.
 *     plan: -1 = what the forward pass takes for this batch, or the signature-attention kernel 0 .. 4 as linetr_debug_sig_attention
 *     numbers them (4: the fused projection + attention) + LINETR_STAGE_FOLD_NEXT for the single-pair path whose x_out and next
 *     q/k/v projection come out of one contraction, or 4 + LINETR_SIG_EIGHT_WAVES (the fused kernel's eight-compute-wave form at
 *     any size).  *plan_used (may be NULL) receives the plan that ran, in the same encoding.
 *     A forced plan the stage's buffers or kernels cannot serve is refused: kernels 1-3 or 4 in f32 mode, 4 outside bf16x6 mode,
 *     with an image above 256 sub-lines or with fold_next, fold_next with a kernel other than 1 or above 960 sub-lines.
 * d_ws: linetr_debug_stage_workspace_bytes(h, N, n_images) bytes (n_images = 1 for the tail; -1 on bad arguments): the forward
 * pass's workspace without its token rows.  Refused with LINETR_E_ARG, nothing launched or written: a training-mode handle, a bad
 * stage / plan / cu_sub, NULL tensors, tensors or a workspace that are not 16-byte aligned, a workspace that is too small
 * (LINETR_E_ARG here too).  N = 0 launches nothing.  Synchronises `stream` before returning. */
enum { LINETR_STAGE_TAIL = 0, LINETR_STAGE_SIG = 1, LINETR_STAGE_FOLD_NEXT = 8 };
int64_t linetr_debug_stage_workspace_bytes(const LinetrHandle* h, int32_t N, int32_t n_images);
int linetr_debug_stage(LinetrHandle* h, int32_t stage, int32_t N, const float* d_in0, const float* d_in1, const int32_t* h_cu_sub,
                       int32_t n_images, int32_t plan, float* d_out0, float* d_out1, float* d_out2, int32_t* plan_used, void* d_ws,
                       int64_t ws_bytes, void* stream);

/* The weight preparation of linetr_create alone, on the host: no device, no handle (tests/test_prepare_cpu.py: every fold against a
 * float64 restatement, bit for bit).  cfg .. numel as linetr_create takes them, refused with the same codes and texts.  One call
 * prepares once and returns everything:
 *   h_image  the float32 image of the weight arena exactly as linetr_create uploads it (every entry starts at a multiple of 64
 *            floats), and behind it 8 more floats, c_tok[4] and s_cls[4] of the CLS pooling, which the handle keeps on the host;
 *   h_table  one LinetrPreparedEntry per tensor, in placement order.
 * *n_floats / *n_entries receive the two sizes whenever the preparation itself succeeded.  h_image and h_table both NULL: only the
 * sizes.  A buffer shorter than its size (image_capacity in floats, table_capacity in entries): LINETR_E_CAPACITY, nothing written
 * but the sizes.
 * Entry names.  A GEMM weight W<x> [rows][K = cols] (LINETR_PREP_GEMM) is followed by its bias b<x> [rows]:
 *   Wword1 bword1 (no GEMM), Wword2 .. Wword4, Wline1 bline1 (no GEMM), Wline2 .. Wline5   the positional encoders, BatchNorm folded
 *   U, U2 [4][256], c_tok, s_cls [4]                                                       the CLS pooling constants
 *   Watt [256][544], Wfc (bias + cls_token), ln1g, ln1b, Wf1, Wf2, ln2g, ln2b              the descriptive layer behind the pooling
 *   Wqkv<l> [768][256] (head-major rows, q / 8), W1m<l> [512][512] (BatchNorm and merge folded), W2<l>      signature layer l
 *   Wnext<l> [1024][768]                                                                   layers 0 .. L - 2
 *   Wfin, Wfin2 [256][768] (L > 0)
 *   bn_g<s>, bn_b<s> [channels]      a training-mode configuration: gamma / beta of slot s of the packed statistics, placed in front of
 *                                    their (then unfolded) convolution
 * LINETR_PREP_ST: linetr_create also makes a split-tile image of the weight.
 * LINETR_E_ARG (linetr_create too): n_tensors < 0, a NULL entry of `names` (a NULL h_data[i] is an omitted tensor), a negative capacity. */
typedef struct {
  char name[24];      /* NUL-terminated                         */
  int64_t offset;     /* in floats from h_image                 */
  int32_t rows, cols;
  int32_t flags;      /* LINETR_PREP_*                          */
  int32_t reserved;
} LinetrPreparedEntry; /* 48 bytes */
enum { LINETR_PREP_GEMM = 1, LINETR_PREP_ST = 2 };
int linetr_debug_prepare(const LinetrModelConfig* cfg, int32_t n_tensors, const char* const* names, const float* const* h_data,
                         const int64_t* numel, float* h_image, int64_t image_capacity, LinetrPreparedEntry* h_table,
                         int32_t table_capacity, int64_t* n_floats, int32_t* n_entries);

#ifdef LINETR_EXPERIMENTS
/* ---- split-tile ("ST") operands (csrc/lt_st_image.h; the GEMM on them: experiments/csrc/lt_gemm_st.h): experiments build only --------------------
 * (liblinetr_hip_experiments.so, `python -m linetr_amd.build --experiments`; measured and not shipped)
 * The signature network keeps its activations in HBM pre-split into three bf16 planes, in 512-byte chunks that are the
 * LDS image of a 16-row x 16-column block (K-step-major), so that a GEMM's K steps travel by LDS-DMA.  These three entry points expose
 * the format and the kernel to the unit tests and micro-benchmarks (no reference counterpart: the reference's
 * nn.Conv1d(k=1) calls, models/line_transformer.py:157-183, are what the GEMM replaces).
 * linetr_st_bytes: size of the ST image of a [rows][K] matrix (K % 16 == 0; rows are padded to a multiple of 128),
 * -1 on bad arguments.
 * linetr_debug_to_st / from_st: fp32 rows (row stride ld floats, multiple of 4) <-> ST image; exact both ways.
 * linetr_debug_gemm_st: Y = act([A1 | A2] W^T + bias) (+ R), all operands ST images (d_A2 / d_bias / d_R may be NULL),
 * result as an ST image (d_Yst) or, when d_Yst is NULL, as fp32 rows d_Y (row stride ldy).  N % 256 == 0,
 * (K1 + K2) % 32 == 0. */
int64_t linetr_st_bytes(int64_t rows, int32_t K);
int linetr_debug_to_st(LinetrHandle* h, const float* d_X, int32_t ld, int32_t rows, int32_t K, void* d_st, void* stream);
int linetr_debug_from_st(LinetrHandle* h, const void* d_st, int32_t rows, int32_t K, float* d_X, int32_t ld, void* stream);
int linetr_debug_gemm_st(LinetrHandle* h, const void* d_A1, int32_t K1, const void* d_A2, int32_t K2, const void* d_W,
                         const float* d_bias, const void* d_R, void* d_Yst, float* d_Y, int32_t ldy, int32_t M, int32_t N,
                         int32_t act, void* stream);
/* Diagnostics of the single-pair persistent signature network (csrc/lt_pairnet.h): the next launches write wall-clock stamps
 * (100 MHz ticks) per block and stage into d_buf [blocks][4 n_sig_layers + 1][8] = {first unit picked up, its producers seen,
 * last body done, last unit published, four probes inside the unit}; the caller zeroes the buffer.  NULL switches the stamps off.  tools/pairnet_timeline.py */
int linetr_debug_pairnet_stamps(LinetrHandle* h, unsigned long long* d_buf);
#endif  /* LINETR_EXPERIMENTS */

/* ---- multi-GPU: the descriptor all-gather as a C entry point --------------------------------------
 * ONE all-gather of the ranks' packed slabs (header | sub-line -> key-line map | line_desc rows; layout in
 * linetr_amd/parallel.py, which the Python surface uses through torch.distributed) over an RCCL communicator the CALLER
 * owns: d_out [world][slab_bytes] receives every rank's d_slab.  `nccl_comm` is an ncclComm_t.  The library does not link
 * against RCCL: ncclAllGather is resolved at the first call from the RCCL already loaded in the process (PyTorch's or
 * /opt/rocm's librccl.so); LINETR_E_HIP if none is loaded.  No reference counterpart (BASELINE.json cfg4); asynchronous
 * on `stream`.  linetr_match_gathered then matches straight out of d_out. */
int linetr_allgather_desc(void* nccl_comm, const void* d_slab, void* d_out, int64_t slab_bytes, void* stream);

/* The ncclAllGather to call.  A process can hold two RCCL copies (PyTorch's bundled one and /opt/rocm's); the function must
 * come from the copy that created `nccl_comm`, so a caller that knows which one that is hands its ncclAllGather in here
 * (dlsym on its own library handle).  Without this call linetr_allgather_desc takes the first ncclAllGather the process-wide
 * symbol resolution finds -- correct when only one RCCL is loaded.  NULL resets to that default. */
int linetr_set_allgather_fn(void* nccl_allgather_fn);

/* One rank's slab for that all-gather in ONE launch (the layout linetr_amd/parallel.py documents and GatheredSet /
 * linetr_match_gathered read): float32 [hr + mr + rows_cap][256] = int32 header {n_images, sub-lines per image[cap],
 * key-lines per image[cap]} | int32 sub2line[rows_cap] | line_desc rows, with hr = ceil((1 + 2 cap) / 256) and
 * mr = ceil(rows_cap / 256).  The counts are taken from the DEVICE prefix sums d_cu_n / d_cu_k [n_images + 1] (what
 * linetr_describe leaves there), so nothing is copied from the host; d_cu_k / d_sub2line may be NULL.  zero_tail != 0 also
 * clears the descriptor rows N .. rows_cap.  LINETR_E_CAPACITY if the batch does not fit.  No reference counterpart. */
int linetr_pack_slab(const float* d_line_desc, int32_t N, const int32_t* d_cu_n, const int32_t* d_cu_k, int32_t n_images,
                     const int32_t* d_sub2line, int32_t n_images_cap, int32_t rows_cap, int32_t zero_tail, float* d_slab,
                     void* stream);

/* ---- instrumentation ------------------------------------------------------------------------ */

/* Per-kernel-class HIP-event timing.  linetr_set_profiling(h,1) clears the accumulators and makes
 * every subsequent kernel launch of this handle be bracketed by hipEventRecord on its stream;
 * linetr_get_profile synchronises the recorded events and returns, per kernel class, the number of
 * launches, the summed duration and the ALGORITHMIC flops / bytes (SURVEY.md section 8d accounting)
 * those launches performed.  bench.py derives its roofline object from this. */
typedef struct {
  const char* name;   /* static string, e.g. "gemm_f32_128x128" */
  int32_t calls;
  float ms;           /* summed over calls */
  double flops;       /* summed algorithmic flops */
  double bytes;       /* summed compulsory HBM bytes */
} LinetrProfileEntry;
int linetr_set_profiling(LinetrHandle* h, int32_t on);
int linetr_get_profile(LinetrHandle* h, LinetrProfileEntry* out, int32_t max_entries, int32_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* LINETR_HIP_H */
