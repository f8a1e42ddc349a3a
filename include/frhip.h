/*
 * frhip.h — C ABI of the MI355X-native face-embedding + gallery-match path.
 *
 * This is the drop-in boundary for the hot path of sin0235/FaceRecognition
 * (SURVEY.md §8a/§8b).  The reference has no FFI layer: its boundary is the
 * Python call `model(x, labels=None)` / `model(x)` plus the match loops.
 * Each entry point below names the reference interface it replaces
 * (paths relative to the reference root).  Plain C types only: device
 * buffers are passed as raw pointers (e.g. torch `tensor.data_ptr()`),
 * streams as `void*` (a hipStream_t, e.g. torch `current_stream().cuda_stream`),
 * and every function returns FR_OK (0) or a negative FR_ERR_* code with a
 * thread-local message in fr_last_error().
 */
#ifndef FRHIP_H
#define FRHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FR_ABI_VERSION 1

/* ---- status codes (reference error convention: SURVEY.md §8b row "Error convention") ---- */
#define FR_OK 0
#define FR_ERR_ARG (-1)     /* bad argument / unsupported shape              */
#define FR_ERR_HIP (-2)     /* a HIP runtime call failed                      */
#define FR_ERR_WEIGHTS (-3) /* weight blob malformed or tensor missing        */
#define FR_ERR_STATE (-4)   /* call order violated (no weights, no gallery)   */
#define FR_ERR_OOM (-5)     /* device allocation failed                       */
#define FR_ERR_STAGE (-6)   /* a split stage's bounded halo wait ran out in an FR_EMBED_ASYNC forward:
                             * that forward's affected embeddings are NaN (see fr_sync_check)   */

/* ---- backbone architectures ---- */
#define FR_ARCH_RESNET50_ARCFACE 0 /* models/arcface/arcface_model.py:65-202 (ArcFaceModel, ResNet-50 trunk) */
#define FR_ARCH_IRESNET100 1       /* insightface iresnet100 (README.md:72 only; no reference code)         */
#define FR_ARCH_IRV1_FACENET 2     /* models/facenet/facenet_model.py:7-36 (facenet_pytorch InceptionResnetV1) */

/* ---- compute dtypes ---- */
#define FR_DTYPE_BF16 0 /* bf16 activations/weights, f32 accumulate (v_mfma_f32_16x16x32_bf16) */
#define FR_DTYPE_FP8 2  /* BASELINE config 5: e4m3 weights (per-output-channel scale) x e4m3 activations
                         * (dynamic per-tensor power-of-two scale) on v_mfma_scale_f32_16x16x128_f8f6f4,
                         * f32 accumulate; activations stay bf16 in memory (residual stream at bf16);
                         * the stem and the 25088->512 head stay bf16.  Weight blob convs carrying
                         * "<name>.wscale" run fp8 (values in "<name>.w" must be e4m3-representable). */
#define FR_DTYPE_F16 1  /* f16 activations/weights, f32 accumulate (v_mfma_f32_16x16x32_f16): same MFMA
                           rate, 3 more mantissa bits; stores saturate at +-65504 */

/* ---- input formats accepted by fr_embed ---- */
#define FR_IN_U8_NHWC 0  /* aligned crops, u8 [B,H,W,3] RGB; ToTensor+Normalize(0.5,0.5) fused (extract_embeddings.py:170-185) */
#define FR_IN_F32_NCHW 1 /* already-normalized f32 [B,3,H,W], i.e. the output of get_transform()                             */

/* ---- fr_embed flags ---- */
#define FR_EMBED_RAW 1 /* return the un-normalized head output (= model(x, labels=None)); default is F.normalize'd */
/* Return as soon as the forward is enqueued.  Without this flag, a forward that runs an IResNet100 split
 * stage (layer1 / layer2: several workgroups per image waiting for each other's boundary rows, bounded)
 * is waited for before fr_embed returns, and if any of those waits ran out the forward is run again on
 * the per-conv path (no waits), so the returned embeddings are always valid (fr_debug_stage_reruns counts
 * the re-runs).  With it, a part whose wait ran out writes NaN into its image's activations (the
 * embedding is NaN, never a plausible wrong vector) and the handle latches FR_ERR_STAGE, returned once by
 * fr_sync_check or by the next fr_embed / fr_embed_match on the handle. */
#define FR_EMBED_ASYNC 2

typedef struct fr_handle fr_handle;

/* Thread-local message describing the last failure on this thread ("" if none). */
const char* fr_last_error(void);
int fr_abi_version(void);

/* Create a handle bound to HIP device `device`.
 * Replaces: ArcFaceModel(...)/FaceNetModel(...) construction in
 * load_arcface_model (inference/extract_embeddings.py:80-123) and
 * load_facenet_model (:126-167). */
int fr_create(fr_handle** out, int device, int arch, int dtype);
void fr_destroy(fr_handle* h);

/* Load BN-folded weights (FRW1 blob written by facerecognition_amd/weights.py).
 * Replaces: model.load_state_dict(checkpoint['model_state_dict'])
 * (inference/extract_embeddings.py:104-106, :150-153). */
int fr_load_weights(fr_handle* h, const void* blob, size_t nbytes);

/* Pre-allocate activation workspace for batches up to max_batch (no allocation
 * happens inside fr_embed once reserved, so it can be stream-captured). */
int fr_reserve(fr_handle* h, int max_batch);

/* Embedding dimension (512) and the square input side the arch expects (112/160). */
int fr_embed_dim(const fr_handle* h);
int fr_input_size(const fr_handle* h);

/* Forward pass: `in` (device) → `out` (device f32 [B, embed_dim]).
 * Replaces: `model(x, labels=None)` + `F.normalize(p=2, dim=1)` in
 * extract_embedding_single (inference/extract_embeddings.py:377-382) and
 * extract_embeddings_batch (:430-435); FaceNetModel.forward (facenet_model.py:28-36). */
int fr_embed(fr_handle* h, const void* in, int in_fmt, int B, int H, int W,
             float* out, int flags, void* stream);

/* ---- explanations (replaces GradCAM.generate, inference/explainability.py:76-131, as called by
 *      ExplainabilityEngine.explain :298-359, and the activation map of FaceNetExplainabilityEngine.explain
 *      :482-501) ----
 * No backward pass: everything after the explained tensor is affine in eval mode and folded into the head
 * matrix, so d score / d tensor = head.w^T . g with g = d score / d embedding in closed form.
 *   FR_ARCH_RESNET50_ARCFACE  Grad-CAM on backbone.layer4 (= "backbone.layer4.2", the avg-pool's input), as the
 *                             reference's GradCAM default target.
 *   FR_ARCH_IRESNET100        Grad-CAM on "layer4.2", the input of bn2 -> flatten -> fc -> features (the reference
 *                             has no IResNet100 code: this target is this library's choice).
 *   FR_ARCH_IRV1_FACENET      the activation map |block8.conv2d output| summed over channels (that conv is run
 *                             once more without its residual, into scratch of fr_reserve); `target` is ignored.
 * Score: (emb ** 2).sum() when target is NULL, else F.cosine_similarity(emb, target) (norms clamped at 1e-8).
 * Map: channel weights = mean gradient over positions; low = weighted channel sum per position; ReLU; bilinear
 * upsample (align_corners = False) to S x S; (c - min) / (max - min) when max > min, else unchanged (IRV1: no
 * ReLU, zeros when max == min). */

/* Shape of the explained layer (h, w, C) and the map side S (= fr_input_size). */
int fr_explain_shape(const fr_handle* h, int* th, int* tw, int* tc);
/* Forward (as fr_embed with FR_EMBED_RAW) + class-activation map, on `stream` in that order.
 * target [B, D] device f32 or NULL; cam [B,S,S] f32; low [B,th,tw] f32 or NULL (pre-ReLU map);
 * emb [B,D] f32 or NULL (raw embeddings of this forward).  B must not exceed the batch of fr_reserve
 * (FR_ERR_ARG); weights not loaded or nothing reserved: FR_ERR_STATE. */
int fr_explain(fr_handle* h, const void* in, int in_fmt, int B, int H, int W, const float* target,
               float* cam, float* low, float* emb, void* stream);

/* K of the tensor the embedding head reads: 2048 (resnet50_arcface), 25088 (iresnet100), 1792 (irv1_facenet);
 * FR_ERR_ARG on a null handle, FR_ERR_STATE before the weights are loaded. */
int fr_features_dim(const fr_handle* h);
/* One forward under fr_explain's rules (waited for, B at most the reserved batch and at most one chunk, else
 * FR_ERR_ARG), then the head's input as device f32 out [B][K] in torch's flatten order: the pooled vector of the two
 * pooled models, c * 49 + p (NCHW) for IResNet100 (whose device tensor is NHWC).  The values are the 16-bit
 * activations the engine's own head reads, converted to f32.  This is the input of fr_head_forward. */
int fr_features(fr_handle* h, const void* in, int in_fmt, int B, int H, int W, float* out, void* stream);

/* A tensor inside the trunk, for training what comes after it ("Backbone training" below).  cut = FR_CUT_LAYER4_IN:
 * the output of backbone.layer3.5, which layer4.0.conv1 and layer4.0.downsample.0 read, as device f32 physical NHWC
 * out [B][h][w][c] ([B][7][7][1024] for a 112 x 112 input; fr_features_at_shape gives h, w, c).  resnet50_arcface
 * handles only, and not FR_DTYPE_FP8 ones: anything else is FR_ERR_ARG.  fr_features' rules otherwise: one whole
 * forward, waited for, B at most the reserved batch and at most one chunk; the values are the engine's 16-bit
 * activations converted to f32, whichever of the fused layer3 chain or its member convs the plan ran. */
#define FR_CUT_LAYER4_IN 0
int fr_features_at_shape(const fr_handle* h, int cut, int* th, int* tw, int* tc);
int fr_features_at(fr_handle* h, const void* in, int in_fmt, int B, int H, int W, int cut, float* out, void* stream);

/* Synchronize `stream`, then report (once) a split-stage wait that ran out in an FR_EMBED_ASYNC forward
 * of this handle since the last report: FR_ERR_STAGE, else FR_OK. */
int fr_sync_check(fr_handle* h, void* stream);

/* ---- gallery + match (replaces RecognitionEngine.recognize_with_db's loop,
 *      recognition_engine.py:267-289, the notebook np.dot+argmax/argsort,
 *      evaluate_arcface_kaggle.ipynb cells 15-16, and faiss IndexFlatIP.search,
 *      recognition_engine.py:291-326) ---- */

/* Install gallery rows G [N, D] f32 (host or device memory).  Rows whose L2
 * norm differs from 1 by >= 1e-3 are divided by their norm so that the stored
 * dot product equals cosine_similarity (recognition_engine.py:41-63); zero rows
 * stay zero (score 0.0).  `index_base` is added to every returned index (gallery
 * sharding: rank r passes the global row of its first shard row). */
int fr_gallery_set(fr_handle* h, const float* G, int64_t N, int D, int64_t index_base, int g_on_device);
int64_t fr_gallery_rows(const fr_handle* h);

/* Write rows [row0, row0 + n) of the gallery from G [n, D] (host or device): an in-place update of
 * existing rows and/or a contiguous append (row0 <= fr_gallery_rows).  Only the written rows are
 * prepared as in fr_gallery_set (and split for the bf16x3 path); appends grow the allocation
 * geometrically.  Replaces the rebuild-per-edit of the reference's dict db / IndexFlatIP.add
 * (recognition_engine.py:406-418 add_to_db; extract_embeddings.py:625-632). */
int fr_gallery_write(fr_handle* h, const float* G, int64_t row0, int64_t n, int D, int g_on_device);

/* Top-k of P [B, D] (device f32, L2-normalized probes) against the gallery.
 * Results (device): scores [B, k] f32 descending, idx [B, k] int32; ties are
 * broken by lower index (stable sort(reverse=True) / np.argmax semantics).
 * Rows past the gallery end come back as score -inf, idx -1.  1 <= k <= 4096 (faiss
 * IndexFlatIP.search takes any k, recognition_engine.py:291,304): k <= 16 keeps register
 * top-k lists; larger k materialises the exact score rows in stream-ordered scratch
 * (<= 256 MiB per probe chunk) and radix-selects per probe -- the same scores bit for bit,
 * so a large-k list starts with the small-k list.  k > 16 needs N < 2^31. */
int fr_match_topk(fr_handle* h, const float* P, int B, int k, float* scores, int32_t* idx, void* stream);

/* Labelled evaluation of P [B, D] (device f32) against the gallery, without the B x N score matrix
 * (replaces the host similarity matrix of evaluate_arcface_kaggle.ipynb cells 15-19 -- argmax,
 * argsort[:, -5:], sims[i, true_idx], max(axis=1) -- and the per-image loop of
 * inference/evaluate.py:275-349).  true_idx [B] int32 (device) is each probe's true gallery row as a
 * global index, in the index space of fr_match_topk's idx (index_base included).  Results (device):
 *   scores / idx [B, k]  exactly fr_match_topk's (the same launches); k = 0 skips them (both may be
 *                        NULL then, and neither is written);
 *   true_score [B] f32   the score of row true_idx[b], the bits the exact f32 match path gives that pair;
 *   true_rank [B] int32  the number of gallery rows sorting before the true row in fr_match_topk's order
 *                        (score descending, index ascending): its 0-based position, so
 *                        true_rank[b] < k <=> idx[b, true_rank[b]] == true_idx[b];
 *   hist [nbins] u64     (NULL: none) the scores of all pairs (b, j) with j != true_idx[b], ADDED to the
 *                        caller's (zeroed) counts, so that probe chunks accumulate;
 *                        bin = clamp((int)floorf((s - lo) * inv_w), 0, nbins - 1) with inv_w =
 *                        (float)nbins / (hi - lo), every operation rounded to f32 on its own;
 *                        1 <= nbins <= 2048, hi > lo.
 * A true_idx outside [index_base, index_base + N) (another shard's row, or negative) gives true_score
 * -inf and true_rank -1, and all N rows count as impostors of that probe.  N < 2^31. */
int fr_match_eval(fr_handle* h, const float* P, int B, const int32_t* true_idx, int k,
                  float* scores, int32_t* idx, float* true_score, int32_t* true_rank,
                  uint64_t* hist, int nbins, float lo, float hi, void* stream);

/* Threshold (range) search of P [B, D] (device f32) against the gallery: every gallery row whose score is
 * >= thresh, without the B x N score matrix and without a guessed k.  This is the reference's decision rule
 * as a query -- an identity is known iff not best_score < threshold (recognition_engine.py:286,323) -- and
 * the IndexFlatIP.range_search member of the surface fr_match_topk serves; NOTE faiss's own range_search
 * keeps score > radius (strict), this keeps score >= thresh.  Scores are the bits the exact f32 match path
 * (fr_match_topk) gives each pair.  The result is a CSR list in two stream-ordered calls with no host
 * synchronisation inside:
 *   fr_match_range_count  writes lims [B + 1] int64 (device): lims[b] = number of hits of probes < b,
 *                         lims[B] = the total; and fills the workspace ws (device,
 *                         fr_match_range_workspace(h, B) bytes, need not be zeroed);
 *   fr_match_range_fill   writes scores [.] f32 and idx [.] int32 (device): probe b's hits are positions
 *                         lims[b] .. lims[b + 1] - 1 in ascending gallery index (global: index_base
 *                         included), the same order in every run (no atomics, no sort).  Positions
 *                         >= capacity are not written, so capacity < lims[B] truncates the list at its end
 *                         (the caller sees it by reading lims[B]).
 * fill must be given the same P, B, thresh, after and ws as the count that produced lims, with the gallery
 * unchanged (no fr_gallery_set / fr_gallery_write) between the two calls; anything else is undefined.
 * after (NULL: none) is [B] int32 (device) of global indices: probe b keeps only rows with index >
 * after[b].  With the gallery's own rows as probes (fr_gallery_read) and after[b] = the probe's own global
 * index this is the self-join "all pairs i < j with score >= thresh", each pair once.
 * thresh = -INFINITY keeps every row (a NaN score is never kept); a NaN thresh is FR_ERR_ARG.  N < 2^31.
 * Null or bad arguments: FR_ERR_ARG; no gallery: FR_ERR_STATE.  fr_match_range_workspace returns 0 on error
 * (null handle, B <= 0, no gallery); its value depends on B and on the gallery's rows and dimension. */
size_t fr_match_range_workspace(const fr_handle* h, int B);
int fr_match_range_count(fr_handle* h, const float* P, int B, float thresh, const int32_t* after,
                         void* ws, int64_t* lims, void* stream);
int fr_match_range_fill(fr_handle* h, const float* P, int B, float thresh, const int32_t* after,
                        const void* ws, const int64_t* lims, float* scores, int32_t* idx,
                        int64_t capacity, void* stream);

/* Copy the stored gallery rows [row0, row0 + n) (local row numbers, as in fr_gallery_write) to out [n, D]
 * f32 in host or device memory: the prepared rows the match uses (divided by their norm where
 * fr_gallery_set's rule says so).  IndexFlatIP.reconstruct_n; also the self-join's probes without a host
 * copy of the gallery.  n = 0 copies nothing; n < 0 or a range outside the gallery is FR_ERR_ARG.
 * Synchronous. */
int fr_gallery_read(const fr_handle* h, int64_t row0, int64_t n, float* out, int out_on_device);

/* Merge n_lists candidate lists per probe: cand_s/cand_i [B, n_lists, k] → [B, k]
 * with the same (score desc, index asc) order.  Used after the RCCL all-gather of
 * per-shard candidates. */
int fr_topk_merge(const float* cand_s, const int32_t* cand_i, int B, int n_lists, int k,
                  float* scores, int32_t* idx, void* stream);

/* The same merge over the multi-GPU candidate exchange block as all-gathered (SURVEY.md §8e step
 * 3-4, one collective): xchg = [n_ranks][2][B][k] 4-byte words, rank r's block holding its shard's
 * top-k scores (f32 [B][k]) followed by their global indices (int32 [B][k]).  Each rank writes its
 * block with fr_match_topk straight into the send buffer; the all-gather output is merged as is
 * (no repacking, no permute).  Replaces the per-shard exchange the reference does not have
 * (single-process recognize_with_db / IndexFlatIP.search, recognition_engine.py:267-326). */
int fr_topk_merge_ranks(const void* xchg, int n_ranks, int B, int k, float* scores, int32_t* idx,
                        void* stream);

/* Fused convenience: fr_embed (normalized) then fr_match_topk on the same stream. */
int fr_embed_match(fr_handle* h, const void* in, int in_fmt, int B, int H, int W, int k,
                   float* emb_out, float* scores, int32_t* idx, void* stream);

/* Segmented mean + renormalize (gallery construction: extract_embedding_for_folder
 * inference/extract_embeddings.py:755-760, compute_prototypes :555-592,
 * RecognitionEngine.add_to_db recognition_engine.py:411-413):
 * out[s] = m / (||m|| + 1e-8), m = mean of E[seg_start[s] .. seg_start[s+1]) (device). */
int fr_segment_mean_normalize(const float* E, int D, const int32_t* seg_start, int n_seg,
                              float* out, void* stream);

/* ---- crop preparation on the device (u8 RGB NHWC in and out) ---- */

/* Bytes of device workspace fr_resize_u8 needs for this shape (0 when the width is unchanged). */
size_t fr_resize_u8_workspace(int B, int H, int W, int OH, int OW);
/* Replaces: PIL Image.resize((OW, OH), Image.BILINEAR) inside get_transform / get_facenet_transform's
 * Resize (inference/extract_embeddings.py:170-185): Pillow's two-pass antialiased bilinear resampler,
 * bit-exact (coefficients in double as Pillow, 22-bit fixed point, horizontal pass first).  in: device
 * [B,H,W,3] u8; out: device [B,OH,OW,3] u8; ws: device workspace of fr_resize_u8_workspace bytes. */
int fr_resize_u8(const uint8_t* in, int B, int H, int W, uint8_t* out, int OH, int OW, void* ws, size_t ws_bytes,
                 void* stream);
/* Replaces: cv2.warpAffine(image, M, (OW, OH), borderValue=0) of align_face (extract_embeddings.py:216-242,
 * recognition_engine.py:169-204; INTER_LINEAR, BORDER_CONSTANT 0), restating OpenCV's fixed-point path
 * (1/32-pixel grid, 15-bit weights).  M: device [B][2][3] float64, the FORWARD source->destination matrices
 * (SimilarityTransform(src landmarks -> ARCFACE_TEMPLATE).params[:2], as the reference passes them). */
int fr_warp_affine_u8(const uint8_t* in, int B, int H, int W, const double* M, uint8_t* out, int OH, int OW,
                      void* stream);

/* ---- face detection before the path: the building blocks of the device MTCNN
 *      (facerecognition_amd/face_detector.py), replacing facenet-pytorch's MTCNN behind
 *      FaceDetector._detect_mtcnn (preprocessing/face_detector.py:78-97, 144-210).  f32 NHWC tensors. ---- */

/* F.interpolate(mode='area') of u8 RGB regions + (x - 127.5) * 0.0078125 (detect_face's imresample and
 * normalisation): regions (device int32 [n][5]) = image index, y0, x0, h, w inside img [*, H, W, 3];
 * out (device f32) [n, oh, ow, 3].  Bit-identical to torch's CPU adaptive average pooling. */
int fr_area_resample_u8(const uint8_t* img, int H, int W, const int32_t* regions, int n, int oh, int ow, float* out,
                        void* stream);
/* Valid (unpadded) stride-1 conv, weights [Cout][kh][kw][Cin], + bias, then PReLU when slope != NULL. */
int fr_mtcnn_conv(const float* x, int B, int H, int W, int Cin, const float* w, const float* bias, const float* slope,
                  int Cout, int kh, int kw, float* y, void* stream);
/* MaxPool2d(k, stride, ceil_mode=True): y [B, Ho, Wo, C] with Ho = ceil((H - k) / stride) + 1 (torch's rule). */
int fr_mtcnn_maxpool(const float* x, int B, int H, int W, int C, int k, int stride, float* y, void* stream);
/* Linear: y [B, N] = x [B, K] . w [N, K]^T + bias, then PReLU when slope != NULL. */
int fr_mtcnn_dense(const float* x, int B, int K, const float* w, const float* bias, const float* slope, int N, float* y,
                   void* stream);
/* Net heads: out [M, n_out] = x [M, C] . w [n_out, C]^T + bias, columns 0-1 replaced by their softmax
 * (face probability in column 1), the rest raw (box regression, landmarks). */
int fr_mtcnn_head(const float* x, int64_t M, int C, const float* w, const float* bias, int n_out, float* out,
                  void* stream);

/* Greedy NMS on the host (detect_face's batched_nms / batched_nms_numpy): boxes [n][4] (x1, y1, x2, y2) float32,
 * order = the candidates' score order; a box is dropped when a kept box earlier in the order overlaps it with
 * IoU > thresh (min_mode = 0: torchvision's areas and test, a 0 / 0 IoU keeps) or unless intersection / min
 * area <= thresh (min_mode = 1: nms_numpy's 'Min', +1-pixel extents), float32 arithmetic as numpy's.  keep [n] receives the kept indices in
 * order, *n_keep their count.  Grid-bucketed: O(n) for boxes of bounded size. */
int fr_nms_host(const float* boxes, int64_t n, const int64_t* order, float thresh, int min_mode, int64_t* keep,
                int64_t* n_keep);

/* Greedy NMS on the device (nms_device.hip): fr_nms_host's contract over independent segments, every buffer in device
 * memory.  boxes [n][4] float32 (16-byte aligned); order [n] int64, the visiting order; seg_start [n_seg + 1] int64,
 * a CSR that cuts order into segments (seg_start[0] <= ... <= seg_start[n_seg] <= n; entries of order past
 * seg_start[n_seg] are never read); thresh and min_mode as fr_nms_host.  Segment s visits boxes
 * order[seg_start[s] .. seg_start[s + 1]) and never sees another segment's boxes.  keep [n] int64 receives the kept
 * box indices, segment after segment, each in greedy order; seg_kept [n_seg + 1] int64 is their CSR.  The kept
 * lists equal fr_nms_host run on each segment with the same order, element for element (the same float32 operations
 * in the same order, IEEE division; degenerate boxes included).  An order entry outside [0, n) is skipped.
 * One workgroup per segment walks it in chunks of 64 candidates against the kept list: O(n x kept / 1024) per segment,
 * n / 64 sequential steps; meant for the 10^2..10^4 boxes per segment of a working detector.
 * ws: fr_nms_workspace(n, n_seg) bytes of device memory, 16-byte aligned (0 bytes are reported as an error: n or n_seg
 * out of range).  n_seg == 0 returns at once; n == 0 zeroes seg_kept and launches nothing; a workgroup with an empty
 * segment returns at once.  Refused with FR_ERR_ARG and a message before any HIP call: null or misaligned pointers,
 * n < 0 or > 2^30, n_seg < 0 or > 2^24, a non-finite or negative thresh, min_mode not 0 / 1, a short workspace. */
size_t fr_nms_workspace(int64_t n, int64_t n_seg);
int fr_nms(const float* boxes, int64_t n, const int64_t* order, const int64_t* seg_start, int64_t n_seg, float thresh,
           int min_mode, int64_t* keep, int64_t* seg_kept, void* ws, size_t ws_bytes, void* stream);

/* ---- box stages of the batched detector (mtcnn_boxes.hip; DeviceMTCNN.detect_batch): detect_face's numpy lines
 *      between the nets as launches over device buffers, float32 with every product rounded before its add,
 *      bit-identical to the host path.  A selection keeps the input order through an ordered compaction (counts per
 *      workgroup, an exclusive scan, writes behind an in-wave prefix; no atomics).  Boxes are [.][4] float32
 *      (x1, y1, x2, y2) and regression rows [.][4] float32, both 16-byte aligned; scores [.] float32; image or
 *      segment ids [.] int32; counters are device int32.  ws: fr_mtcnn_compact_workspace(items) bytes of device
 *      memory (items = B hh ww, or n).  Every limit is FR_ERR_ARG with a message before any HIP call. ---- */
size_t fr_mtcnn_compact_workspace(int64_t total);
/* P-net candidates of one pyramid level: from map [B][hh][ww][6] (prob(bg), prob(face), reg x4) the cells with
 * prob(face) >= thresh in np.nonzero order (image, y, x), appended behind the running total *counter (the previous
 * level's call left it there; zero it before level 0): box = (floor((2 x + 1) / scale), floor((2 y + 1) / scale),
 * floor((2 x + 12) / scale), floor((2 y + 12) / scale)), score = prob(face), reg = the four regression values,
 * seg = level * B + image.  *counter += this level's count, also past capacity: rows at or past capacity are counted
 * and not written.  B, hh, ww >= 1 with B hh ww <= 2^30, scale finite > 0, thresh finite >= 0, 0 <= level <= 4095,
 * 1 <= capacity <= 2^30. */
int fr_mtcnn_candidates(const float* map, int B, int hh, int ww, float scale, float thresh, int level,
                        int64_t capacity, float* box, float* score, float* reg, int32_t* seg, int32_t* counter,
                        void* ws, size_t ws_bytes, void* stream);
/* R-net (C = 6) / O-net (C = 16) selection: the rows of out [n][C] with out[.][1] > thresh (strict), in row order:
 * obox = box of the row, oscore = out[.][1], oreg = out[.][2..6), oimg = img of the row, and for C = 16
 * opts [.][10] = out[.][6..16) (opts is NULL exactly when C = 6).  *counter = the number of rows kept.  Outputs
 * hold n rows.  1 <= n <= 2^30, thresh finite >= 0. */
int fr_mtcnn_select(const float* out, int64_t n, int C, float thresh, const float* box, const int32_t* img,
                    float* obox, float* oscore, float* oreg, int32_t* oimg, float* opts, int32_t* counter, void* ws,
                    size_t ws_bytes, void* stream);
/* Regression, _rerec, _pad and the ok filter, one thread per box.  Row i takes source row g = keep[i] (keep NULL:
 * g = i) for i < *n_keep (n_keep NULL: i < n; both device int64, as fr_nms leaves them); n is the number of source
 * rows and the bound on i.  plus1 = 0 is the P stage's b + reg (x2 - x1), plus1 = 1 is _bbreg's
 * b + reg (x2 - x1 + 1); then _rerec ((b + w 0.5) - l 0.5, then + l), _pad (truncate to int32, clamp to 1 / W / H)
 * and ok = (ey > y - 1) & (ex > x - 1).  The rows that pass ok, in order: obox = the squared box, oscore = score[g],
 * oimg = img[g] % B, regions [.][5] int32 = (image, y - 1, x - 1, ey - y + 1, ex - x + 1), fr_area_resample_u8's
 * layout.  *counter = their number.  Outputs hold n rows. */
int fr_mtcnn_crop_boxes(const float* box, const float* score, const float* reg, const int32_t* img, int64_t n, int B,
                        const int64_t* keep, const int64_t* n_keep, int plus1, int W, int H, float* obox,
                        float* oscore, int32_t* oimg, int32_t* regions, int32_t* counter, void* ws, size_t ws_bytes,
                        void* stream);
/* The O stage's last lines for rows i < min(n, *n_dev) (n_dev NULL: n): opts [.][5][2] = the landmark points
 * ((w pt) + x1) - 1, ((h pt) + y1) - 1 from pts [.][10] (five x then five y), w = x2 - x1 + 1, and obox = _bbreg. */
int fr_mtcnn_final_boxes(const float* box, const float* reg, const float* pts, int64_t n, const int32_t* n_dev,
                         float* obox, float* opts, void* stream);

/* ---- LBPH (the models/lbphmodel package, cv2.face.LBPHFaceRecognizer): OpenCV's published algorithm restated, handle-free.
 *      Checked against a float32/float64 numpy restatement (tests/lbph_ref.py), not against a cv2.face build.
 *      A histogram is kept as u16 counts [D], D = grid_x * grid_y * 2^neighbors, cells row-major; OpenCV's float32
 *      histogram is count / (float)P, P = cw * ch pixels per cell, cw = (W - 2 radius) / grid_x,
 *      ch = (H - 2 radius) / grid_y (integer division; pixels past grid * cell are ignored). ---- */

/* The extended-LBP neighbour table (host only): for neighbour n, offs[n] = {fx, fy, cx, cy} and
 * w[n] = {w1, w2, w3, w4}, float32 as OpenCV computes them.  radius 1..4, neighbors 1..8, else FR_ERR_ARG. */
int fr_lbph_table(int radius, int neighbors, int32_t* offs /*[n][4]*/, float* w /*[n][4]*/);
/* img (device u8) [B][H][W] gray -> counts (device u16, 4-byte aligned) [B][D].  Bit n of a pixel's code is set when
 * the float32 bilinear sample t = w1 a + w2 b + w3 c + w4 d (each product rounded, summed left to right, no fused
 * multiply-add) has t > centre or |t - centre| < FLT_EPSILON.  Supported: radius 1..4, neighbors 1..8, grid_x and
 * grid_y 1..16, H and W <= 512, cw >= 1, ch >= 1, P <= 65535, B 1..2^24; anything else is FR_ERR_ARG, decided
 * before any HIP call. */
int fr_lbph_hist(const uint8_t* img, int B, int H, int W, int radius, int neighbors, int grid_x, int grid_y,
                 uint16_t* counts, void* stream);
/* Bytes of device workspace fr_lbph_match needs (0 and a message on bad arguments). */
size_t fr_lbph_match_workspace(int B, int64_t N, int D, int k);
/* HISTCMP_CHISQR_ALT top-k: for each of B probe count rows Q [B][D] the k smallest
 * d = 2 * sum_j (a_j - b_j)^2 / (a_j + b_j) over the gallery count rows G [N][D] (a = count / P; bins with
 * a_j + b_j = 0 skipped), ascending, equal distances by ascending row; dist (device f64) [B][k], idx (device i32)
 * [B][k], +inf / -1 past N.  Computed on the counts: each term (ka - kb)^2 / (ka + kb) in float32 with IEEE
 * division, summed in float64 in an order that depends on D alone, times 2 / P: a probe's result is bitwise the
 * same alone and in a batch.  No B x N matrix is written.  B 1..65535, N 1..2^30, D 1..65536, cell_pixels (P)
 * 1..65535, k 1..32, else FR_ERR_ARG. */
int fr_lbph_match(const uint16_t* Q, int B, const uint16_t* G, int64_t N, int D, int cell_pixels, int k, double* dist,
                  int32_t* idx, void* ws, size_t ws_bytes, void* stream);

/* ---- t-SNE (inference/extract_embeddings.py visualize_tsne, sklearn.manifold.TSNE's defaults): sparse kNN input
 *      affinities as in sklearn's Barnes-Hut path, the repulsive term summed exactly over all pairs (angle 0), two
 *      components.  Handle-free, caller-owned device buffers.  Common limits, each FR_ERR_ARG with a message before
 *      any HIP call: non-null pointers, N >= 2, 1 <= k < N, k <= 4095, 2 N k < 2^31.  Every result is bitwise
 *      repeatable: sums run in a fixed order and no floating-point atomics are used. ---- */

/* d2 (device f32) [N][k] = sum_d (X[i][d] - X[idx[i][j]][d])^2 for X (device f32) [N][D], idx (device i32) [N][k]
 * with entries in [0, N) (not checked), by direct subtraction in float32.  D >= 1. */
int fr_tsne_knn_sqdist(const float* X, int N, int D, const int32_t* idx, int k, float* d2, void* stream);
/* Bytes of device workspace fr_tsne_affinities needs (0 and a message on bad arguments). */
size_t fr_tsne_affinities_workspace(int N, int k);
/* Per row i the bandwidth beta[i] whose conditional p_j|i = exp(-beta d2[i][j]) / sum has entropy log(perplexity)
 * (sklearn's _binary_search_perplexity: beta from 1, doubled or halved while unbounded, at most 100 steps, stop at
 * |H - log perplexity| <= 1e-5; searched in float64 with each row's smallest distance subtracted first, which
 * leaves p unchanged and keeps a far row from underflowing to zero), then P_ij = (p_j|i + p_i|j) / (2 N) as CSR
 * with ascending columns: indptr (i32) [N + 1], col (i32) and val (f32) of capacity 2 N k each, of which the first
 * indptr[N] are written.  A row's idx entries must be distinct and differ from the row's own index (not checked;
 * repeated entries leave val unspecified but every write in bounds).  perplexity finite and > 0. */
int fr_tsne_affinities(const int32_t* idx, const float* d2, int N, int k, float perplexity, int32_t* indptr,
                       int32_t* col, float* val, float* beta, void* ws, size_t ws_bytes, void* stream);
/* Bytes of device workspace fr_tsne_gradient and fr_tsne_run need (0 and a message on bad arguments). */
size_t fr_tsne_gradient_workspace(int N);
/* grad (f32) [N][2]: g_i = 4 (e sum_j P_ij w_ij (y_i - y_j) - sum_j w_ij^2 (y_i - y_j) / Z), w_ij = 1 / (1 + |y_i -
 * y_j|^2), Z = sum_{i != j} w_ij, e = exaggeration; stats (device f64) [3] = {KL, Z, |grad|_2} with KL = sum_nnz
 * P_ij (log P_ij + log(1 + |y_i - y_j|^2)) + log Z in float64 (entries with P_ij = 0 skipped; P without the
 * exaggeration).  Pair terms in float32, each difference y_i - y_j formed before it is weighted.  The CSR's columns
 * must lie in [0, N) (not checked).  exaggeration finite and > 0. */
int fr_tsne_gradient(const int32_t* indptr, const int32_t* col, const float* val, int N, const float* Y,
                     float exaggeration, float* grad, double* stats, void* ws, size_t ws_bytes, void* stream);
/* n_steps (>= 1) steps of sklearn's _gradient_descent on Y, update, gains (f32 [N][2] each), in place and enqueued
 * without host synchronisation: inc = update g < 0; gains += 0.2 where inc, *= 0.8 elsewhere, at least 0.01;
 * update = momentum update - learning_rate gains g; Y += update.  grad and stats are those of the last step's
 * gradient (evaluated before that step's update).  momentum and learning_rate finite and > 0. */
int fr_tsne_run(const int32_t* indptr, const int32_t* col, const float* val, int N, float* Y, float* update,
                float* gains, float exaggeration, float momentum, float learning_rate, int n_steps, float* grad,
                double* stats, void* ws, size_t ws_bytes, void* stream);
/* The repulsion launch of one iteration alone (timing): the per-split partials {sum w^2 dx, sum w^2 dy,
 * sum_{j != i} w} of Y [N][2] go to the start of the workspace (fr_tsne_gradient_workspace bytes) as 16-byte records
 * {fx, fy, z, 0}, and nothing else is written. */
int fr_op_tsne_repulsion(const float* Y, int N, void* ws, size_t ws_bytes, void* stream);

/* ---- ArcFace margin loss (models/arcface/arcface_model.py ArcMarginProduct + nn.CrossEntropyLoss(label_smoothing)
 *      + train_arcface.py's mixup criterion), forward and backward, without a B x C matrix.  Handle-free,
 *      caller-owned device buffers; f32 and i32 device pointers, 16-byte aligned E, W, dE, dW.
 *      With e^ = e / max(|e|, 1e-12), w^ likewise, c_bj = e^_b . w^_j (exact f32), s = scale, m = margin:
 *        z_bj = s c_bj (j != y_b),  z_b,y = s zy,  q = 1 - c^2, sine = sqrt(max(q, 1e-7)), phi = c cos m - sine sin m,
 *        zy = c > cos(pi - m) ? phi : c - sin(pi - m) m      (easy_margin: c > 0 ? phi : c)
 *        CE(z, y) = (1 - ls)(lse - z_y) + ls (lse - mean_j z_j),  loss_b = lam CE(z_b, y_b) + (1 - lam) CE(z_b, y'_b)
 *      (label_b NULL: lam = 1).  Only the first label gets the margin.  A label outside [0, C), in either array, is
 *      defined: its CE term is 0 and gives no gradient, it never indexes memory, and an out-of-range first label
 *      also means no margin for the row.
 *      Limits, each FR_ERR_ARG with a message before any HIP call: B >= 1, C >= 2, D >= 4 and D % 4 == 0,
 *      B C <= 2^40, C D <= 2^40, B D <= 2^40 (all indexing is 64-bit), scale finite and > 0, margin in [0, pi),
 *      lam in [0, 1], label_smoothing in [0, 1), required pointers non-null, ws_bytes >= fr_arcmargin_workspace.
 *      Every result is bitwise repeatable: sums run in an order fixed by (B, C, D), no floating-point atomics. ---- */

/* Bytes of device workspace the two calls below need (0 and a message on bad arguments): the per-split partials
 * of the log-sum-exp and of dE, a small multiple of B D floats -- never B C. */
size_t fr_arcmargin_workspace(int B, int C, int D);
/* loss [B], lse [B] = log sum_j exp z_bj, inv_e [B] = 1 / max(|e_b|, 1e-12), inv_w [C] (IEEE sqrt and division);
 * logits [B][C] = z when non-NULL (ArcMarginProduct.forward's return value), else no B x C buffer exists. */
int fr_arcmargin_forward(const float* E, int B, int D, const float* W, int C, const int32_t* label,
                         const int32_t* label_b /*NULL*/, float lam, float scale, float margin, int easy_margin,
                         float label_smoothing, float* loss, float* lse, float* inv_e, float* inv_w,
                         float* logits /*NULL*/, void* ws, size_t ws_bytes, void* stream);
/* dE [B][D] and / or dW [C][D] (at least one non-NULL) of sum_b u_b loss_b (u [B], with the forward's lse) or of a
 * function of z with gradient dlogits [B][C] (lse may be NULL); exactly one of u and dlogits is non-NULL.  inv_e and
 * inv_w are the forward's.  g_bj = u_b (softmax(z_b)_j - target_bj) s (j == y_b ? dzy/dc : 1) (or dlogits_bj in place
 * of the first two factors), dE^ = g W^, dW^ = g^T E^, dE_b = (dE^_b - (dE^_b . e^_b) e^_b) / max(|e_b|, 1e-12), dW
 * likewise; dzy/dc = cos m + (q >= 1e-7 ? sin m c / sine : 0) on the phi branch, 1 on the other. */
int fr_arcmargin_backward(const float* E, int B, int D, const float* W, int C, const int32_t* label,
                          const int32_t* label_b /*NULL*/, float lam, float scale, float margin, int easy_margin,
                          float label_smoothing, const float* lse, const float* inv_e, const float* inv_w,
                          const float* u /*NULL*/, const float* dlogits /*NULL*/, float* dE /*NULL*/,
                          float* dW /*NULL*/, void* ws, size_t ws_bytes, void* stream);

/* ---- Triplet mining and loss (models/facenet: mine_semi_hard_triplets, mine_batch_hard_triplets, mine_triplets,
 *      TripletLoss = nn.TripletMarginLoss(margin, p=2), and train_facenet.py's compute_triplet_metrics).  Handle-free,
 *      caller-owned device buffers; E (device f32) [N][D], 16-byte aligned, not necessarily normalised; labels
 *      (device i32) [N], any values, none is "ignored".
 *      Mining distance (the Gram form torch.cdist itself uses above 25 rows): g_ij = e_i . e_j (exact f32),
 *        s_i = sum_k e_ik^2,  d2_ij = max(s_i + s_j - 2 g_ij, 0),  d_ij = sqrt(d2_ij) (IEEE square root).
 *      The order of every floating-point operation is fixed by (N, D): neither the workspace size nor the banding
 *      changes a bit.
 *      Positives of anchor a: rows p != a with labels[p] == labels[a], ascending p.  Negatives: rows of another label.
 *      An anchor without a positive or without a negative yields nothing (the reference's mine_triplets raises on an
 *      anchor without negatives; here it is skipped).
 *        FR_TRIPLET_SEMI_HARD  one triplet per (anchor, positive): among the negatives with d_an > d_ap and
 *                              d_an < d_ap + margin (f32 sum, f32 comparisons) the one of smallest d_an; if there is
 *                              none, the negative of smallest d_an of all.
 *        FR_TRIPLET_BATCH_HARD one triplet per anchor: the positive of largest d_ap, the negative of smallest d_an.
 *        FR_TRIPLET_FIRST      one triplet per (anchor, positive): the semi-hard negative of lowest index; if there is
 *                              none, the negative of LARGEST d_an (what the reference's mine_triplets does).
 *      Every tie goes to the lowest index.  Triplets are listed by ascending anchor, then ascending positive, the same
 *      in every run (no atomics, no sort).  Every index written lies in [0, N) whatever E holds; which row is chosen
 *      among non-finite distances is unspecified.  The selection costs T N comparisons (T = number of triplets): one
 *      class of c rows gives c (c - 1) triplets, so do not feed it one giant class.
 *      Loss, from the difference form: delta(x, y) = |x - y + 1e-6|_2, h_t = max(margin + delta(a_t, p_t) -
 *      delta(a_t, n_t), 0), loss = (1 / T) sum_t h_t.  The triplet indices a, p, n (device i32 [T]) must lie in [0, N):
 *      like labels they are the caller's responsibility and are not checked.
 *      Limits, each FR_ERR_ARG with a message before any HIP call: 2 <= N <= 32768, D >= 4 and D % 4 == 0, margin
 *      finite and > 0, mode one of the three, 1 <= T <= 2^40, u finite, required pointers non-null, capacity >= 0,
 *      ws_bytes at least the stated minimum.  Every result is bitwise repeatable: sums run in a fixed order, no
 *      floating-point atomics. ---- */
#define FR_TRIPLET_SEMI_HARD 0
#define FR_TRIPLET_BATCH_HARD 1
#define FR_TRIPLET_FIRST 2

/* Recommended bytes of device workspace for fr_triplet_mine (0 and a message on bad arguments): the whole N x N
 * distance matrix where that is at most 256 MiB, else as many 64-anchor bands as fit, plus the norms.  The minimum
 * fr_triplet_mine accepts is one band: 4 (64 N + 64 ceil(N / 64)) bytes. */
size_t fr_triplet_workspace(int N, int D);
/* lims (device i64) [N + 1]: lims[a] = the number of triplets of anchors < a, lims[N] = T.  From the labels alone. */
int fr_triplet_count(const int32_t* labels, int N, int mode, int64_t* lims /*[N+1]*/, void* stream);
/* The triplets of fr_triplet_count's lims (same labels and mode): a_idx, p_idx, n_idx (device i32), triplet
 * lims[a] + k = anchor a with its k-th positive; positions >= capacity are not written.  semi (device u8, NULL ok):
 * 1 where the semi-hard branch was taken, 0 where the fallback (always 0 for FR_TRIPLET_BATCH_HARD, which ignores
 * margin).  Anchors are processed in bands of as many whole multiples of 64 rows as ws_bytes holds. */
int fr_triplet_mine(const float* E, int N, int D, const int32_t* labels, int mode, float margin, const int64_t* lims,
                    int32_t* a_idx, int32_t* p_idx, int32_t* n_idx, int64_t capacity, uint8_t* semi /*NULL*/, void* ws,
                    size_t ws_bytes, void* stream);
/* terms (device f32, 16-byte aligned) [T][4] = {h_t, |a - p|, |a - n|, margin + delta_ap - delta_an}; stats (device
 * f32, 16-byte aligned) [4] = {loss, accuracy, pos_dist, neg_dist}: the mean of h_t, the share of triplets with
 * |a - p| < |a - n|, the means of |a - p| and |a - n| (compute_triplet_metrics: these distances are WITHOUT the
 * 1e-6).  The per-triplet terms are also the storage the fixed-order reduction reads, so terms is required. */
int fr_triplet_loss_forward(const float* E, int N, int D, const int32_t* a, const int32_t* p, const int32_t* n,
                            int64_t T, float margin, float* terms /*[T][4]*/, float* stats /*[4]*/, void* stream);
/* dE [N][D] (fully written, zeros included) = the gradient of u loss.  A triplet is active when margin + delta_ap -
 * delta_an >= 0 (clamp_min passes the gradient at equality).  With w_ap = (u / T) / delta_ap and w_an likewise (0
 * where delta is 0: torch's norm subgradient), an active triplet adds w_ap (a - p + 1e-6) - w_an (a - n + 1e-6) to row
 * a, -w_ap (a - p + 1e-6) to row p and +w_an (a - n + 1e-6) to row n.  A row's contributions are summed in ascending
 * triplet index and, within a triplet, in the order anchor, positive, negative.  Each row has one owner, which scans
 * the three index arrays (N T integer reads).  ws: at least 8 T bytes (the two weights per triplet). */
int fr_triplet_loss_backward(const float* E, int N, int D, const int32_t* a, const int32_t* p, const int32_t* n,
                             int64_t T, float margin, float u, float* dE, void* ws, size_t ws_bytes, void* stream);

/* ---- All-pairs verification (the 1:1 question behind the reference's compute_verification_accuracy,
 *      models/arcface/train_arcface.py and models/facenet/train_facenet.py, on EVERY pair of one labelled set instead
 *      of 10 000 sampled ones).  Handle-free, caller-owned device buffers; E (device f32) [N][D], 16-byte aligned;
 *      labels (device i32) [N], any values, none is "ignored".  No N x N matrix is stored.
 *      Score of the pair (i, j): g_ij = e_i . e_j (exact f32, fr_match_topk's operation order).  normalize = 1:
 *        r_i = 1 / (sqrt(sum_k e_ik^2) + 1e-8f),  s_ij = (g_ij r_i) r_j
 *      (the reference's a / (|a| + 1e-8) applied to the score; every operation rounded to f32, IEEE square root and
 *      division).  normalize = 0: s_ij = g_ij, the rows as given.
 *      A pair is genuine when labels[i] == labels[j], otherwise an impostor; the diagonal is never a pair.
 *      The order of every floating-point operation is fixed by (N, D): the workspace size and the banding change no
 *      bit, and every result is bitwise repeatable (integer atomics only).
 *      With non-finite scores which row is chosen is unspecified; every index written lies in [-1, N).
 *      Limits, each FR_ERR_ARG with a message before any HIP call: 2 <= N <= 2^22, D >= 4 and D % 4 == 0, normalize
 *      0 or 1, 0 <= T <= 64 with thresholds and counts non-null when T > 0, every threshold finite, 1 <= nbins <= 2048
 *      and finite hi > lo when hist is given, E, labels, totals and ws non-null, row_score and row_idx together or not
 *      at all, ws_bytes at least the stated minimum. ---- */
#define FR_VERIFY_MAX_THRESHOLDS 64

/* Recommended bytes of device workspace for fr_verify_pairs (0 and a message on bad arguments): the norms and every
 * row's partial results (32 bytes per row and 1024-column chunk) where those are at most 256 MiB, else as many 64-row
 * bands as fit.  The minimum fr_verify_pairs accepts is one band: 4 * 64 ceil(N / 64) + 2048 ceil(N / 1024) bytes. */
size_t fr_verify_workspace(int N, int D);
/* One pass over all pairs.  thresholds: HOST f32 [T] (read before the call returns).  Outputs, all on the device:
 *   totals [2] u64 (required)   the number of genuine and of impostor pairs i < j; overwritten.
 *   counts [T][2] u64           per threshold the number of genuine and of impostor pairs i < j with s > t (strict f32
 *                               comparison, the reference's rule, not the engine's >=); overwritten.
 *   hist [2][nbins] u64 (NULL)  the genuine and the impostor histogram over i < j, ADDED to the caller's counts; bin =
 *                               clamp((int)floorf((s - lo) * inv_w), 0, nbins - 1) with inv_w = (float)nbins / (hi - lo)
 *                               rounded once (fr_match_eval's rule).
 *   row_score [N][3] f32, row_idx [N][3] i32 (both or NULL)   per row i over all j != i: its best genuine mate (largest
 *                               s), its worst genuine mate (smallest s) and its best impostor (largest s); ties to the
 *                               lowest j; where there is no such j the score is -inf, +inf, -inf and the index -1.
 *   row_sum [N][2] f32 (NULL)   per row the sum of its genuine and of its impostor scores over j != i: per 1024-column
 *                               chunk a lane's columns (j mod 16 equal) in ascending j, a 16-lane tree, then the chunks in
 *                               ascending order.
 * Without row outputs only the upper triangle is computed.  Stream-ordered, no host synchronisation inside. */
int fr_verify_pairs(const float* E, int N, int D, const int32_t* labels, int normalize,
                    const float* thresholds /*host [T]*/, int T, uint64_t* counts /*[T][2]*/,
                    uint64_t* totals /*[2]*/, uint64_t* hist /*[2][nbins], NULL*/, int nbins, float lo, float hi,
                    float* row_score /*[N][3], NULL*/, int32_t* row_idx /*[N][3], NULL*/,
                    float* row_sum /*[N][2], NULL*/, void* ws, size_t ws_bytes, void* stream);

/* ---- Augmentation: the training transforms of the reference's dataloaders (torchvision on PIL images) as a per-image
 *      op list run on the device, one workgroup per image with the image resident in LDS.  Handle-free, caller-owned
 *      device buffers.  in (device u8) [B][H][W][3].  ops (HOST i32) [B][n_ops] and args (HOST f64) [B][n_ops][8] are
 *      read and checked before the call returns, then staged into ws and the kernel is enqueued on the stream.
 *      Image b runs ops[b][0 .. n_ops) in order on its u8 image (Pillow's arithmetic unless stated; the restatement and
 *      its checks against Pillow are tests/augment_ref.py and tests/test_augment_ref.py):
 *        FR_AUG_NOP                   nothing (pads a row)
 *        FR_AUG_FLIP_H                transpose(FLIP_LEFT_RIGHT)
 *        FR_AUG_AFFINE_NEAREST        Image.transform(size, AFFINE, m, NEAREST), fill 0, as Pillow's 16.16 fixed-point
 *                                     walk: FIX(v) = floor(65536 v + 0.5), source x = (FIX(m2 + m0/2 + m1/2) + FIX(m1) y
 *                                     + FIX(m0) x) >> 16, y likewise from m3..m5.  args m0..m5 (output -> input map).
 *                                     As Pillow requires for this walk, |m0 x + m1 y + m2| and |m3 x + m4 y + m5| must be
 *                                     < 32768 at (0,0), (W,0), (0,H), (W,H).  (Pillow answers m1 = m3 = 0 from another
 *                                     routine that steps in double; here every matrix takes the fixed-point walk.)
 *        FR_AUG_PERSPECTIVE_BILINEAR  Image.transform(size, PERSPECTIVE, a, BILINEAR), fill 0: double arithmetic at
 *                                     (x + 0.5, y + 0.5), truncating store; a source outside [0,W) x [0,H) or NaN is 0.
 *                                     args a0..a7.
 *        FR_AUG_CROP_RESIZE           crop((j, i, j + w, i + h)).resize((W, H), BILINEAR): the two-pass antialiased
 *                                     resampler of fr_resize_u8 with per-image 22-bit coefficients.  args i, j, h, w:
 *                                     integers, 1 <= h, 1 <= w, the box inside the image.
 *        FR_AUG_BRIGHTNESS / FR_AUG_CONTRAST / FR_AUG_SATURATION   ImageEnhance.{Brightness, Contrast, Color}.enhance(f):
 *                                     t = d + (float)f (src - d) in f32 against d = 0 / the constant int(mean(L) + 0.5) /
 *                                     L, truncated for 0 <= f <= 1, else clipped to [0, 255] first;
 *                                     L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.  args f >= 0.
 *        FR_AUG_HUE                   torchvision's PIL adjust_hue: convert("HSV"), H += (uint8)(int)(255 f) with u8 wrap,
 *                                     convert back.  args f in [-0.5, 0.5].
 *        FR_AUG_GRAYSCALE             convert("L") in all 3 channels
 *        FR_AUG_GAUSS_BLUR            torchvision's tensor gaussian_blur of a u8 image: taps (float)w[dy] (float)w[dx]
 *                                     (one f32 product), reflect padding, the f32 sum from 0 in row-major tap order,
 *                                     every product rounded, rintf, clamp to [0, 255].  args k, w[0 .. k): k in {3, 5, 7},
 *                                     k / 2 < min(H, W).
 *        FR_AUG_ERASE                 RandomErasing(value = 0): the box of out_f32 is 0.0f; out_u8 is not touched.  args
 *                                     i, j, h, w as for the crop.  At most one per row, and only FR_AUG_NOP after it.
 *      Outputs (either may be NULL, not both): out_f32 [B][3][H][W] = ToTensor + Normalize(0.5, 0.5) of the result,
 *      ((float)u / 255.0f - 0.5f) / 0.5f per byte u (what fr_embed takes as FR_IN_F32_NCHW); out_u8 [B][H][W][3].
 *      No atomics and no randomness: the result is a pure function of (in, ops, args), bitwise repeatable.
 *      Limits, each FR_ERR_ARG with a message before any HIP call: B >= 1 (B <= 2^24), H, W >= 1 with
 *      6 H W <= 153600 and H + W <= 512 (the two LDS image buffers and the coefficient tables: 160 x 160 is the largest
 *      square), 0 <= n_ops <= 16, in, ws, and (when n_ops > 0) ops and args non-null, an output non-null, known opcodes,
 *      every argument of every row finite, the per-op limits above, ws_bytes >= fr_augment_workspace. ---- */
#define FR_AUGMENT_MAX_OPS 16
#define FR_AUGMENT_ARGS 8
#define FR_AUG_NOP 0
#define FR_AUG_FLIP_H 1
#define FR_AUG_AFFINE_NEAREST 2
#define FR_AUG_PERSPECTIVE_BILINEAR 3
#define FR_AUG_CROP_RESIZE 4
#define FR_AUG_BRIGHTNESS 5
#define FR_AUG_CONTRAST 6
#define FR_AUG_SATURATION 7
#define FR_AUG_HUE 8
#define FR_AUG_GRAYSCALE 9
#define FR_AUG_GAUSS_BLUR 10
#define FR_AUG_ERASE 11

/* Bytes of device workspace fr_augment needs (the staged op lists and the normalisation table); 0 and a message on
 * bad arguments. */
size_t fr_augment_workspace(int B, int n_ops);
/* Stream-ordered.  The host arrays may be reused as soon as the call returns; the call may wait for the staging copy of
 * the previous fr_augment call on the same device. */
int fr_augment(const uint8_t* in, int B, int H, int W, const int32_t* ops /*host [B][n_ops]*/,
               const double* args /*host [B][n_ops][8]*/, int n_ops, float* out_f32 /*[B][3][H][W], NULL*/,
               uint8_t* out_u8 /*[B][H][W][3], NULL*/, void* ws, size_t ws_bytes, void* stream);

/* ---- Head training: the embedding head between a frozen trunk and the losses above, forward and backward
 *      (ArcFaceModel's bn1 -> dropout -> fc -> bn2, IResNet100's bn2 -> flatten -> fc -> features, FaceNet's
 *      dropout -> last_linear -> last_bn).  Handle-free, caller-owned f32 device buffers; X, W, Y, dW, dX (and A, Z, dY)
 *      16-byte aligned.
 *      X [B][K] with K = Cin S; feature f belongs to input-BN channel f / S (S = 1: BatchNorm1d; S = 49: IResNet100's
 *      BatchNorm2d before the flatten).  W [N][K], bias [N] or NULL, gamma1 / beta1 [Cin] or both NULL (no input BN),
 *      gamma2 / beta2 [N].  flags: FR_HEAD_BATCH_STATS (both BNs use batch statistics and update the running ones; else
 *      they use the running ones and update nothing) | FR_HEAD_DROPOUT (dropout is active).  freeze_bn is DROPOUT alone.
 *      Forward, n1 = B S, n2 = B:
 *        mean1_c = sum x / n1, var1_c = sum (x - mean1_c)^2 / n1 (two passes, biased), rstd1 = 1 / sqrt(var1 + eps) (IEEE),
 *        running_mean1 <- (1 - mom) running_mean1 + mom mean1, running_var1 <- (1 - mom) running_var1 + mom var1 n1 / (n1 - 1)
 *        (running statistics: mean1 = running_mean1, var1 = running_var1);  H = gamma1 (x - mean1) rstd1 + beta1  (no BN: H = X)
 *        A = H m / (1 - p): Philox4x32-10 (Random123 constants) with key (lo32 seed, hi32 seed) and counter
 *        (lo32 (i >> 2), hi32 (i >> 2), lo32 offset, hi32 offset) for the 64-bit element index i = b K + f; r = output word
 *        i & 3; keep iff r >= T = (uint32) floor(p 2^32) (in double); kept: H (1.0f / (1.0f - p)), dropped: +0.0f;
 *        p = 0 or the flag off: A = H
 *        Z = A W^T + bias (exact f32; split-K partials merged in split order, the split a function of (B, K, N) alone)
 *        mean2, var2, rstd2 and the running update over the B rows of Z likewise;  Y = gamma2 (Z - mean2) rstd2 + beta2
 *      Backward from dY [B][N], z^ = (Z - mean2) rstd2, x^ = (x - mean1) rstd1:
 *        batch statistics: dgamma2 = sum_b dY z^, dbeta2 = sum_b dY, dZ = gamma2 rstd2 (dY - dbeta2 / n2 - z^ dgamma2 / n2)
 *        running statistics: the same dgamma2, dbeta2; dZ = dY gamma2 rstd2
 *        dW = dZ^T A (every row has one owner), dbias = sum_b dZ, dA = dZ W, dH = dA m / (1 - p)
 *        dgamma1 = sum dH x^, dbeta1 = sum dH (over B S), dX = gamma1 rstd1 (dH - dbeta1 / n1 - x^ dgamma1 / n1)
 *        (running statistics: dX = dH gamma1 rstd1; no input BN: dX = dH).  The mask is regenerated from (seed, offset).
 *      Limits, each FR_ERR_ARG with a message before any HIP call: B >= 1; with BATCH_STATS B S >= 2 where the input BN
 *      is present and B >= 2; K, N >= 4 and multiples of 4; S >= 1 and K % S == 0; B K, N K, B N <= 2^40 (all indexing is
 *      64-bit) and, for the launch grids, B <= 2^24 and K, N <= 4194240; p in [0, 1); eps finite and > 0; momentum in [0, 1]; no unknown flag bits; gamma1 and beta1 both given
 *      or both NULL; running statistics present whenever a BN is; required pointers non-null; ws_bytes >=
 *      fr_head_workspace.  Every result is bitwise repeatable and independent of the workspace size: sums run in an
 *      order fixed by (B, K, S, N), no floating-point atomics. ---- */
#define FR_HEAD_BATCH_STATS 1
#define FR_HEAD_DROPOUT 2

/* Bytes of device workspace the two calls below need (0 and a message on bad arguments): the split-K partials of Z,
 * and for the backward dZ [B][N] plus per-64-row column sums for the input BN -- never a B x K gradient. */
size_t fr_head_workspace(int B, int K, int N);
/* Y [B][N], Z [B][N] (the Linear's output, saved for the backward), mean1 / rstd1 [Cin] (NULL without the input BN),
 * mean2 / rstd2 [N], and A [B][K] when non-NULL (the Linear's input).  running_* are read, and with BATCH_STATS
 * written. */
int fr_head_forward(const float* X, int B, int K, int S, const float* W, int N, const float* bias /*NULL*/,
                    const float* gamma1 /*NULL*/, const float* beta1 /*NULL*/, float* running_mean1 /*NULL*/,
                    float* running_var1 /*NULL*/, const float* gamma2, const float* beta2, float* running_mean2,
                    float* running_var2, int flags, float p, float eps, float momentum, uint64_t seed, uint64_t offset,
                    float* Y, float* Z, float* mean1 /*NULL*/, float* rstd1 /*NULL*/, float* mean2, float* rstd2,
                    float* A /*NULL*/, void* ws, size_t ws_bytes, void* stream);
/* Any of dX [B][K], dW [N][K], dbias [N], dgamma1 / dbeta1 [Cin], dgamma2 / dbeta2 [N] (at least one non-NULL; dgamma1
 * and dbeta1 only with the input BN).  flags, p, seed, offset, Z and the four statistics are the forward's.  With dX
 * NULL (a frozen trunk) no B x K gradient is written anywhere. */
int fr_head_backward(const float* X, int B, int K, int S, const float* W, int N, const float* gamma1 /*NULL*/,
                     const float* beta1 /*NULL*/, const float* gamma2, int flags, float p, uint64_t seed,
                     uint64_t offset, const float* mean1 /*NULL*/, const float* rstd1 /*NULL*/, const float* mean2,
                     const float* rstd2, const float* Z, const float* dY, float* dX /*NULL*/, float* dW /*NULL*/,
                     float* dbias /*NULL*/, float* dgamma1 /*NULL*/, float* dbeta1 /*NULL*/, float* dgamma2 /*NULL*/,
                     float* dbeta2 /*NULL*/, void* ws, size_t ws_bytes, void* stream);

/* ---- Backbone training: convolution and BatchNorm2d in training mode, forward and backward, as ResNet-50's layer4
 *      needs them (the reference's freeze_layers(model, 0.8), models/arcface/arcface_model.py:223, leaves exactly
 *      backbone.layer4 trainable).  Handle-free, caller-owned f32 device buffers, each 16-byte aligned.
 *      Layouts: activations physical NHWC, X [B][H][W][Cin], Z / dZ [B][OH][OW][Cout]; weights Wt / dW
 *      [Cout][k][k][Cin] -- torch's channels_last memory of an NCHW-shaped activation and an OIHW-shaped weight.
 *      k = 1 (pad 0) or 3 (pad 1), the same stride s in both directions, OH = (H + 2 pad - k) / s + 1 (OW likewise).
 *      Convolution, with the optional input transform (scale / shift [Cin], both or neither; FR_CONV_IN_RELU only with
 *      them), which is the folded BN (and ReLU) of the layer before and is applied while the operand is staged -- A is
 *      never stored:
 *        A[b,h,w,c] = X[b,h,w,c]                                  (no transform)
 *                   = relu?(fma(X[b,h,w,c], scale[c], shift[c]))   (transform)
 *        Z[b,oh,ow,n] = sum_{r,s,c} A[b, oh s + r - pad, ow s + s - pad, c] Wt[n,r,s,c], a tap outside the image
 *        contributing +0: the padding is zero in A-space, not relu(shift).  Exact f32; the terms run in (r, s, c)
 *        order, split-K partials merged in split order, the split a function of the shape alone.
 *        dA[b,h,w,c] = sum_{r,s,n} dZ[b,oh,ow,n] Wt[n,r,s,c] over the taps with oh s + r - pad = h (likewise w) and
 *        (oh, ow) inside the output; an input pixel no tap reaches gets +0.0f.  This is the gradient by A, not by X.
 *        dW[n,r,s,c] = sum_{b,oh,ow} dZ[b,oh,ow,n] A[b, oh s + r - pad, ow s + s - pad, c]  (padded taps +0).
 *        Every element of dA and dW has one owner and is written.
 *      BatchNorm2d over Z viewed as [M][C], M = B OH OW (NHWC makes it a column statistic):
 *        FR_BN_BATCH_STATS: mean_c = sum z / M, var_c = sum (z - mean_c)^2 / M (two passes, biased),
 *        running_mean <- (1 - mom) running_mean + mom mean, running_var <- (1 - mom) running_var + mom var M / (M - 1);
 *        else mean = running_mean, var = running_var and nothing is updated.
 *        rstd = 1 / sqrt(var + eps) (IEEE), scale = gamma rstd, shift = beta - mean scale (each operation rounded).
 *        y = fma(Z, scale, shift) (+ Res);  Y = relu?(y)   (FR_BN_RELU)
 *        Backward from dY, z^ = (Z - mean) rstd:  dH = dY [y > 0] (dY without FR_BN_RELU; y is recomputed as above),
 *        dRes = dH, dgamma = sum_m dH z^, dbeta = sum_m dH,
 *        batch statistics: dZ = gamma rstd (dH - dbeta / M - z^ dgamma / M);  running statistics: dZ = dH scale.
 *      One Bottleneck keeps only its raw conv outputs, its input and its output: relu(bn(Z1)) and relu(bn(Z2)) are the
 *      transforms of conv2 and conv3 (forward and dW), and fr_bn_act_backward turns the dA of conv2 / conv3 into dZ1 /
 *      dZ2 with Res = NULL.
 *      Limits, each FR_ERR_ARG with a message before any HIP call: B, H, W >= 1, H, W <= 32768; Cin, Cout multiples of
 *      4 in [4, 262144]; k in {1, 3}; stride in {1, 2}; B H W < 2^31; B H W Cin and B OH OW Cout <= 2^40
 *      (all indexing is 64-bit); M in [1, 2^24], with FR_BN_BATCH_STATS M >= 2; C a multiple of 4 in [4, 2^24]; eps
 *      finite and > 0; momentum in [0, 1]; no unknown flag bits; required pointers non-null; ws_bytes >=
 *      fr_conv_train_workspace; at least one gradient requested.  Every result is bitwise repeatable and independent
 *      of the workspace size: sums run in an order fixed by the shape, no floating-point atomics. ---- */
#define FR_CONV_IN_RELU 1
#define FR_BN_BATCH_STATS 1 /* = FR_HEAD_BATCH_STATS */
#define FR_BN_RELU 2

/* Bytes of device workspace fr_conv_train_forward needs (0 and a message on bad arguments): the split-K partials of Z
 * when M is small, 16 otherwise.  The backward needs none. */
size_t fr_conv_train_workspace(int B, int H, int W, int Cin, int Cout, int k, int stride);
int fr_conv_train_forward(const float* X, int B, int H, int W, int Cin, const float* scale /*NULL*/,
                          const float* shift /*NULL*/, int flags, const float* Wt, int Cout, int k, int stride, float* Z,
                          void* ws, size_t ws_bytes, void* stream);
/* Any of dA [B][H][W][Cin] and dW [Cout][k][k][Cin] (at least one non-NULL).  X, the transform and flags are the
 * forward's.  With dA NULL (the conv sits on a frozen trunk) no B x H x W x Cin gradient is written anywhere. */
int fr_conv_train_backward(const float* X, int B, int H, int W, int Cin, const float* scale /*NULL*/,
                           const float* shift /*NULL*/, int flags, const float* Wt, int Cout, int k, int stride,
                           const float* dZ, float* dA /*NULL*/, float* dW /*NULL*/, void* stream);
/* mean, rstd, scale, shift [C] of one BatchNorm2d over Z [M][C]; flags: FR_BN_BATCH_STATS or 0.  running_* are read,
 * and with FR_BN_BATCH_STATS written. */
int fr_bn2d_train_stats(const float* Z, int64_t M, int C, const float* gamma, const float* beta, float* running_mean,
                        float* running_var, int flags, float eps, float momentum, float* mean, float* rstd, float* scale,
                        float* shift, void* stream);
/* Y [M][C] = relu?(fma(Z, scale, shift) + Res?); flags: FR_BN_RELU or 0.  Needed only where the result must exist in
 * memory: a block's output with its residual, and the downsample branch. */
int fr_bn_act_forward(const float* Z, int64_t M, int C, const float* scale, const float* shift, const float* Res /*NULL*/,
                      int flags, float* Y, void* stream);
/* Any of dZ [M][C] (may be dY itself), dRes [M][C] (only with Res; not dY or dZ), dgamma, dbeta [C]; flags:
 * FR_BN_BATCH_STATS | FR_BN_RELU as in the forward. */
int fr_bn_act_backward(const float* dY, const float* Z, int64_t M, int C, const float* mean, const float* rstd,
                       const float* gamma, const float* scale, const float* shift, const float* Res /*NULL*/, int flags,
                       float* dZ /*NULL*/, float* dRes /*NULL*/, float* dgamma /*NULL*/, float* dbeta /*NULL*/,
                       void* stream);

/* ---- Optimiser step: torch's clip_grad_norm_ followed by SGD, Adam or AdamW over a list of f32 device tensors, in
 *      two stages and without a host round trip.  Handle-free, caller-owned buffers, the caller's stream.  The arrays
 *      of pointers, counts and betas are host arrays, read during the call: the tensor table travels in kernel
 *      arguments (64 tensors per norm launch, 48 per update launch), so nothing of it can go stale.  A tensor whose
 *      gradient pointer is NULL or whose element count is 0 is skipped, in both stages alike.
 *      Stage 1, fr_optim_grad_norm: g' = g / *grad_scale (grad_scale non-NULL; f32 division) else g.  Every gradient is
 *        cut into chunks of FR_OPTIM_CHUNK elements; chunk c (counted over the whole list) gets sum g'^2 of its
 *        elements in ws[c] (double; fixed order), one workgroup adds ws[0 .. n_chunks) in a fixed order, and
 *        norm = (float)sqrt(sum).  The norm is a function of the tensor list alone: not of the launches the list is
 *        cut into, of the pointers' alignment or of ws_bytes.  No floating-point atomics.  The same workgroup writes
 *        the control block ctrl (device, FR_OPTIM_CTRL_BYTES(n_groups), 8-byte aligned; the host never reads it in a
 *        step): head.norm; head.clip = min(1, max_norm / (norm + 1e-6f)) in f32 -- torch's rule, a NaN norm giving NaN
 *        -- or 1 when max_norm <= 0 (no clipping; the norm is still reported); head.skip = (*found_inf != 0, found_inf
 *        non-NULL) or (FR_OPTIM_SKIP_NONFINITE and the norm is not finite).  Unless skip, every group state
 *        g < n_groups advances: step += 1, beta1_pow *= beta1[g], beta2_pow *= beta2[g] (doubles), prev_ok = last_ok,
 *        last_ok = attempt.  attempt >= 1 is the caller's count of fr_optim_grad_norm calls on this block, rising by
 *        at least one per call.  A fresh block is zero except beta1_pow = beta2_pow = 1.
 *      Stage 2, fr_optim_step, one group's tensors in one pass (p, g and the state read once, p and the state written
 *        once; 16-byte accesses through every pointer that is 16-byte aligned, 4-byte ones through one that is not
 *        -- a view at a storage offset -- and for the last numel % 4 elements).  With head.skip set nothing is
 *        written: parameters, state and counters keep every byte.  Otherwise, every operation rounded to f32 (no
 *        fused multiply-add), sqrt and / correctly rounded, Python-double hyper-parameters cast to f32 where torch's
 *        kernels take them, in torch's single-tensor order:
 *          g = (g / *grad_scale) * head.clip;  FR_OPTIM_MAXIMIZE: g = -g
 *          SGD:   wd != 0: g = g + wd p;  momentum != 0: buf = g in the tensor's first applied step (prev_ok < born[i]),
 *                 else buf = buf momentum + (1 - dampening) g;  g = nesterov ? g + momentum buf : buf;  p = p + (-lr) g
 *          Adam:  wd != 0: g = g + wd p;   AdamW: wd != 0: p = p (1 - lr wd)
 *                 d = g - m, w = 1 - beta1: m = w < 0.5 ? m + w d : g - d (1 - w);  v = v beta2 + ((1 - beta2) g) g
 *                 denom = sqrt(v) / sqrt(1 - beta2_pow) + eps;  p = p + (-(lr / (1 - beta1_pow)) m) / denom
 *        state1 is momentum_buffer / exp_avg, state2 exp_avg_sq; born[i] is the attempt at which tensor i's state was
 *        created (0: it was loaded, the buffer is live).  amsgrad (FR_OPTIM_AMSGRAD) is refused.
 *      Limits, each FR_ERR_ARG with a message before any HIP call: n_tensors >= 0 with non-NULL arrays when > 0; every
 *      numel in [0, 2^40], at most 2^24 chunks per call; pointers 4-byte aligned; max_norm not NaN; n_groups in
 *      [0, FR_OPTIM_MAX_GROUPS], group < FR_OPTIM_MAX_GROUPS; betas in [0, 1); lr, eps, weight_decay, momentum >= 0 and
 *      finite, dampening finite; nesterov needs momentum > 0 and dampening = 0; no unknown flag bits; kind one of the
 *      three; a parameter and the state the kind needs non-NULL for every tensor with a gradient; ctrl and ws
 *      non-NULL and 8-byte aligned; ws_bytes >= fr_optim_workspace(n_chunks); attempt >= 1. ---- */
#define FR_OPTIM_SGD 0
#define FR_OPTIM_ADAM 1
#define FR_OPTIM_ADAMW 2
#define FR_OPTIM_NESTEROV 1
#define FR_OPTIM_MAXIMIZE 2
#define FR_OPTIM_AMSGRAD 4        /* refused */
#define FR_OPTIM_SKIP_NONFINITE 8 /* fr_optim_grad_norm only */
#define FR_OPTIM_CHUNK 65536
#define FR_OPTIM_MAX_GROUPS 32
typedef struct fr_optim_ctrl_head {
    float norm, clip;
    int32_t skip;
    int32_t reserved[13];
} fr_optim_ctrl_head; /* 64 bytes */
typedef struct fr_optim_group_state {
    double step, beta1_pow, beta2_pow;
    int64_t last_ok, prev_ok;
    int64_t reserved[3];
} fr_optim_group_state; /* 64 bytes */
#define FR_OPTIM_CTRL_BYTES(n_groups) (64 * (1 + (size_t)(n_groups)))

/* Bytes of device workspace fr_optim_grad_norm needs for n_chunks = sum over the tensors with a gradient of
 * ceil(numel / FR_OPTIM_CHUNK) chunks (0 and a message on bad arguments; never 0 otherwise). */
size_t fr_optim_workspace(int64_t n_chunks);
int fr_optim_grad_norm(const float* const* grads /*host [n_tensors]*/, const int64_t* numel /*host [n_tensors]*/,
                       int n_tensors, double max_norm, int flags, const float* found_inf /*device, NULL*/,
                       const float* grad_scale /*device, NULL*/, int n_groups, const double* beta1 /*host [n_groups]*/,
                       const double* beta2 /*host [n_groups]*/, int64_t attempt, void* ctrl, void* ws, size_t ws_bytes,
                       void* stream);
int fr_optim_step(int kind, float* const* params, const float* const* grads, float* const* state1 /*NULL*/,
                  float* const* state2 /*NULL*/, const int64_t* numel, const int64_t* born /*NULL: all 0*/, int n_tensors,
                  double lr, double weight_decay, double momentum, double dampening, double beta1, double beta2,
                  double eps, int flags, const void* ctrl, int group, const float* grad_scale /*device, NULL*/,
                  void* stream);

/* ---- op-level entry points (kernel parity tests and custom graphs) ---- */

/* Implicit-GEMM convolution on NHWC bf16 with fused epilogue:
 *   y = act( conv(x, w) + bias + res )   written to y[..., y_off : y_off+Cout]
 *   y2 = y * aff_s + aff_b                (optional second output, bf16)
 * Weights: bf16 [Npad][Kpad], row n = output channel, K ordered (r, s, c) with
 * c fastest (KRSC), zero padded; Npad % 128 == 0, Kpad % 64 == 0.
 * Requirements: Cin % 8 == 0, Cx/x_off/Cy/y_off/Cres/res_off % 8 == 0, Cout % 8 == 0. */
typedef struct fr_conv_desc {
    const void* x; int B, H, W, Cx, x_off, Cin;  /* input tensor [B,H,W,Cx], channels [x_off, x_off+Cin) */
    const void* w; int Cout, Kh, Kw, stride_h, stride_w, pad_h, pad_w, Npad, Kpad;
    const float* bias;   /* [Cout] or NULL */
    int act;             /* 0 none, 1 relu, 2 prelu (slope) */
    const float* slope;  /* [Cout] for prelu */
    const void* res; int Cres, res_off; /* residual [B,Ho,Wo,Cres] bf16 or NULL */
    void* y; int Cy, y_off;             /* output [B,Ho,Wo,Cy] bf16 */
    void* y2; int Cy2, y2_off; const float* aff_s; const float* aff_b; /* optional */
    int Ho, Wo;          /* filled by fr_conv_out_shape if 0 */
    int split_k;         /* 0/1 = fused epilogue; >1 = f32 partials into `partial` then reduce */
    float* partial;      /* workspace [split_k, B*Ho*Wo, Npad] f32 when split_k > 1 */
    int dtype;           /* FR_DTYPE_BF16 / FR_DTYPE_F16: element type of x, w, res, y, y2 */
    int tile;            /* 0 = automatic (cost model); 1 + FR_TILE_* forces a tile variant */
    /* Border-class bias for a 3x3 / stride 1 / pad 1 conv whose input BN was folded into the weights
     * (the BN shift meets the zero padding only at the image border): [9][Npad] f32, class
     * 3*rc + cc with rc = 0 / 1 / 2 for output row 0 / interior / Ho-1 (cc likewise for columns).
     * When set it replaces `bias`.  NULL otherwise. */
    const float* bias9;
    /* dtype == FR_DTYPE_FP8: w is e4m3 bytes [Npad][Kpad] (Kpad % 128 == 0, Cin % 64 == 0), wscale [Npad]
     * per-output-channel f32 scales, x_amax -> the input's max |x| (device f32; the activation scale is
     * the power of two 2^e with max|x| / 2^e <= 448); x, res, y, y2 are bf16; a forced tile must be
     * FR_TILE_128x128, FR_TILE_128x64 or FR_TILE_64x128 (any other id: FR_ERR_ARG).  y_amax (any dtype, may
     * be NULL): the epilogue atomically raises it to max |y| of what it stores (caller zeroes it). */
    const float* wscale;
    const float* x_amax;
    float* y_amax;
} fr_conv_desc;

/* conv tile variants (pixels x channels per 256-thread block) */
#define FR_TILE_128x128 0
#define FR_TILE_256x64 1
#define FR_TILE_128x64 2
#define FR_TILE_64x128 3
#define FR_TILE_128x128_S3 4 /* 3-stage DMA ring, 1 block/CU */
#define FR_TILE_256x128 5    /* 8 waves, 3-stage ring */
#define FR_TILE_128x256 6    /* 8 waves, 3-stage ring */
#define FR_TILE_BAND 7       /* row-band direct 3x3/s1/p1 kernel (conv_band.hip); auto-selected when applicable */
#define FR_TILE_128x64_S3 8  /* 3-stage DMA ring, 2 blocks/CU */
#define FR_TILE_64x128_S3 9  /* 3-stage DMA ring, 2 blocks/CU */
#define FR_TILE_IMG56 11     /* the same for 56x56x64->64 (layer1), 4-row bands */
#define FR_TILE_IMG28 10     /* row-band direct 3x3/s1/p1 28x28x128->128 bf16 kernel (conv_img.hip); auto-selected (FR_AB no_img28: off) */
#define FR_TILE_ROWS 12      /* persistent weight-resident 3x3/s1/p1 kernel for Cin = 64, Cout % 64 == 0, W % 56 == 0,
                              * H % 4 == 0, bf16 (conv_rows.hip); auto-selected (FR_AB no_rows: off) */
#define FR_TILE_WRING 13     /* implicit GEMM with a register weight ring (conv_wring.hip): Cin % 64 == 0, Cout % 256 == 0;
                                autotuned per shape against the igemm tiles (FR_AB no_wring: off) */
#define FR_TILE_DIRECT 14    /* persistent small-K direct conv (conv_direct.hip): Cin % 8 == 0, Kpad <= 384, Cout % 32 == 0,
                                bias + activation epilogue; autotuned per shape (FR_AB no_direct: off) */
/* 15: retired (round 5; a hipBLASLt candidate that never won a whole forward) */
#define FR_TILE_64x64_S3 17  /* 3-stage DMA ring, 64 x 64 tiles (round 6: small-M GEMMs over more CUs) */
#define FR_TILE_64x64 18
#define FR_TILE_32x64_S3 19
#define FR_TILE_SMALL 16     /* small-M implicit GEMM, one wave per 16 px x 64 ch over the whole K (conv_small.hip); bit-identical to tile 0.
                                split_k = KS | NF << 8: KS (4 / 8 / 16) waves share a tile's K (split-K summation order), NF
                                (2 / 1; 0 = 4) 16-channel fragments per tile: 1, 4, 8, 1|2<<8, 4|2<<8, 8|2<<8, 1|1<<8, 4|1<<8,
                                8|1<<8, 16|1<<8 */

int fr_op_conv2d(const fr_conv_desc* d, void* stream);

/* The conv paths a forward plan reaches but fr_conv_desc cannot express (kernel parity tests).  A NULL or
 * all-zero ext is fr_op_conv2d.  Every combination a kernel cannot run is refused with FR_ERR_ARG (a message
 * naming fr_op_conv2d_ex), never run by another kernel. */
typedef struct fr_conv_ext {
    /* K-concatenated 1x1 projection (a residual block's downsample folded into its last conv): K steps
     * [K1, K1 + C2), K1 = Kh*Kw*Cin, read x2 [B,H2,W2,Cx2] at (oh * st2, ow * st2), channels
     * [x2_off, x2_off + C2); the weight rows are [W_conv | W_proj | 0-pad] and bias is the sum of both.
     * Needs Cin % 64 == 0, C2 % 64 == 0, K1 + C2 <= Kpad, (Ho-1)*st2 < H2, (Wo-1)*st2 < W2,
     * x2_off + C2 <= Cx2, Cx2 % 8 == 0, x2_off % 8 == 0.  The implicit-GEMM tiles, FR_TILE_WRING and
     * FR_TILE_SMALL take it (the latter two where their own shape rules hold); not FR_DTYPE_FP8. */
    const void* x2; int H2, W2, Cx2, x2_off, C2, st2;
    /* dtype FR_DTYPE_F16 with y stored as bf16 (the end of an f16 section of a bf16 plan): no res, no y2;
     * the implicit-GEMM tiles, FR_TILE_WRING, FR_TILE_SMALL and FR_TILE_DIRECT. */
    int y_bf16;
    /* split_k > 1 on an implicit-GEMM tile: per-tile arrival counters (one int per pixels x channels tile,
     * zero before the call and zero again after it).  Non-NULL: a single launch, the last workgroup of each
     * tile sums the partials in split order and runs the epilogue (the bits of the two-launch reduction). */
    int* splitk_cnt;
    /* y_amax is an array of this many partial maxima (0 = 1); max |y| is the maximum over them. */
    int amax_slots;
} fr_conv_ext;
int fr_op_conv2d_ex(const fr_conv_desc* d, const fr_conv_ext* e, void* stream);

/* u8 NHWC [B,H,W,3] or f32 NCHW [B,3,H,W] → 16-bit NHWC [B,H,W,8] = [q0,q1,q2,q0,q1,q2,0,0] with
 * q = 2u-255 (u8; exact) or q = 255*x (normalized f32), i.e. q = 255 * ((u/255-0.5)/0.5).  The stem
 * conv weights carry 1/255 as a hi/lo pair on the duplicated channels (exact first layer). */
int fr_op_preprocess(const void* in, int in_fmt, int B, int H, int W, void* out, int dtype, void* stream);

/* Max pool NHWC bf16 (padding never wins, as torch MaxPool2d). */
int fr_op_maxpool(const void* x, int B, int H, int W, int Cx, int x_off, int C,
                  int k, int stride, int pad, void* y, int Cy, int y_off, int Ho, int Wo, int dtype, void* stream);

/* Global average pool NHWC bf16 [B,H,W,C] → bf16 [B,C]. */
int fr_op_avgpool(const void* x, int B, int H, int W, int C, void* y, int dtype, void* stream);

/* Linear head: out[B,N] = x[B,K] (bf16) · w[Npad,Kpad]ᵀ (bf16) + bias, f32 out, optional L2
 * normalize (F.normalize eps 1e-12).  `partial` must hold split_k*B*Npad floats. */
int fr_op_linear(const void* x, int B, int K, const void* w, int N, int Npad, int Kpad,
                 const float* bias, int normalize, float* out, int split_k, float* partial, int dtype, void* stream);

/* The small-batch head of the online path (B <= 8 probes): the same result as fr_op_linear from the GEMV
 * kernel, S chunks of K as split-K partials (`partial` holds S*B*Npad floats), then the head's finalize
 * (bias, optional L2 normalize).  K % 8 == 0, Kpad % 8 == 0, Npad % 16 == 0, N % 4 == 0, N <= 1024;
 * w has Npad rows of Kpad elements.  Anything else is refused (FR_ERR_ARG). */
int fr_op_head_gemv(const void* x, int B, int K, const void* w, int N, int Npad, int Kpad, const float* bias,
                    int normalize, float* out, int S, float* partial, int dtype, void* stream);

/* FaceNet projection: out [B,N] = x [B,K] . W [N,K]^T + bias (all f32; bias may be NULL), optional
 * F.normalize (eps 1e-12).  1 <= K <= 1024. */
int fr_op_proj_l2(const float* x, int B, int K, const float* W, const float* bias, int N, int normalize,
                  float* out, void* stream);

/* Row-wise L2 normalize of x [B,D] f32 in place (F.normalize, eps 1e-12). */
int fr_op_l2norm_rows(float* x, int B, int D, void* stream);

/* max |x| of n 16-bit values (n % 8 == 0) raised into amax[0 .. slots): the maximum over the slots, combined
 * with what they held before, is max |x| (the caller zeroes them for a fresh maximum). */
int fr_op_amax(const void* x, size_t n, int dtype, float* amax, int slots, void* stream);

/* fr_op_maxpool from an f16 tensor into a bf16 one (the end of an f16 section of a bf16 plan): each
 * maximum rounded to bf16 once, to nearest even.  k == 3 only. */
int fr_op_maxpool_cvt(const void* x, int B, int H, int W, int Cx, int x_off, int C, int k, int stride, int pad,
                      void* y, int Cy, int y_off, int Ho, int Wo, void* stream);

/* fr_explain's head-gradient pass: v [B, Kpad] = g [B, N] (f32) . w [N rows of Kpad 16-bit elements], f32
 * accumulation; the order of the sum over n depends on N alone (not on B).  Columns [K, Kpad) of v are left
 * untouched.  N <= 1024, K % 8 == 0, Kpad % 8 == 0, Kpad >= K. */
int fr_op_head_grad(const float* g, int B, int N, const void* w, int K, int Kpad, int dtype, float* v, void* stream);
/* fr_explain's map kernel on act [B,h,w,C] (16-bit NHWC): v_layout 0 = v [B, C] is the gradient of the pooled
 * head input (every position's gradient is v / (h w)); 1 = v [B, h*w*C] is the gradient of the flattened NHWC
 * tensor; 2 = the activation map sum_c |act| (v NULL).  cam [B,S,S] f32; low [B,h,w] f32 or NULL (the map before
 * ReLU).  h*w <= 256, C % 8 == 0, C <= 4096. */
int fr_op_cam(const void* act, int B, int h, int w, int C, int dtype, const float* v, int v_layout, int S, float* cam,
              float* low, void* stream);

/* ---- execution options (no reference counterpart: plan choices of this build) ----------------
 * FR_OPT_STAGE (default 1; FR_AB no_stage starts at 0): run the stride-1 IResNet100 layer3 blocks
 *   as one LDS-resident stage kernel per image instead of 58 separate conv launches.  Numerically the
 *   same op sequence and bf16 rounding points (f32 accumulation in a different K order).  0 = never,
 *   1 = auto: at every batch of at most one image per CU (measured faster than the per-conv launches
 *   down to B = 1), and above that only when the rounds of one image per CU are at least
 *   FR_OPT_STAGE_MIN_FILL percent full (B = 257 on 256 CUs takes the per-conv launches), 2 = always.
 * FR_OPT_STAGE_MIN_FILL (default 80): the auto threshold above, in percent.
 * FR_OPT_KEEP_INTERMEDIATES (default 0): the stage kernel also writes every block output and conv1
 *   output to its named tensor (per-layer drift tests; costs HBM writes).
 * Changing an option drops the captured hipGraph replays.  fr_get_option returns the value (FR_OPT_STAGE
 * reads 0 when the plan has no stage) or FR_ERR_ARG. */
#define FR_OPT_STAGE 1
#define FR_OPT_KEEP_INTERMEDIATES 2
/* FR_OPT_MATCH_EXACT (default 0): galleries of >= FR_OPT_X3_MIN_ROWS rows (D = 512) are matched by a bf16x3 candidate
 * pass (|error| <= 1.25e-4 ||p||) plus exact f32 rescoring of the top-16 candidates per probe, with a
 * per-probe proof that no excluded row can enter the top-k (else an exact rescan of that probe): the
 * results equal the exact f32 kernel's.  1 forces the f32-MFMA kernel for every gallery. */
#define FR_OPT_MATCH_EXACT 3
/* FR_OPT_X3_MIN_ROWS (default 32768): smallest gallery given the bf16x3 path (its hi/lo copy is made by
 * the next fr_gallery_set); below it the f32 kernel is as fast. */
#define FR_OPT_X3_MIN_ROWS 4
#define FR_OPT_STAGE_MIN_FILL 5
/* FR_OPT_STAGE_SPIN_LIMIT (default 0 = the kernel's bound, ~0.1 s): sleeps (64 cycles each) a split-stage
 * part waits for a neighbour's boundary rows before the wait counts as run out.  < 0 makes every wait
 * run out at once (debug: exercises the NaN poisoning, the re-run and FR_ERR_STAGE deterministically). */
#define FR_OPT_STAGE_SPIN_LIMIT 6
/* FR_OPT_STAGE_VARIANT (default 0): the layer3 stage kernel's pixel layout -- 0: 13 fragments of 16 pixels
 * per image (196 of 208 slots used), 1: the legacy 14 rows of 16 positions (2 halo columns computed and
 * discarded per row), 2: the 13-fragment layout at one wave per SIMD (each weight fragment loaded once per
 * CU), 3: 8 waves split by output channel (32 each) over all 13 fragments (each weight fragment loaded once
 * per CU, twice the patch reads).  All give the same bits (A/B and regression tests). */
#define FR_OPT_STAGE_VARIANT 7
/* FR_OPT_SPLITK_INLAUNCH (default 1; FR_AB splitk_inlaunch=0 starts at 0): a split-K implicit-GEMM conv may reduce
 * its partials in the same launch (the last workgroup of each tile sums them in split order) where the
 * per-shape tuning measured that faster than a second launch; 0 = always the second launch.  The same bits
 * either way.  fr_debug_plan prints an in-launch split as a negative split count. */
#define FR_OPT_SPLITK_INLAUNCH 8
/* FR_OPT_BATCH_INVARIANT (default 0): batch-size-independent embeddings.  Every conv runs a kernel that sums K in
 * the implicit GEMM's order (igemm tiles, register-ring, direct and small-M kernels unsplit; no split-K, no LDS-resident
 * stage / transition / block kernels) and the head uses bs = 256's split plan at every batch, so a face's embedding
 * is the same bits whatever batch it is in (the reference's recognize_batch is a loop over recognize,
 * recognition_engine.py:383-389).  Slower than the default, which measures the fastest kernels per batch size.
 * FR_DTYPE_FP8 handles refuse value 1 (FR_ERR_ARG): their e4m3 convs scale activations by a per-batch amax. */
#define FR_OPT_BATCH_INVARIANT 9
/* FR_OPT_FUSED_MASK (default 127): which kinds of fused multi-conv kernels a forward may run (each still measured
 * against its member convs per batch size under FR_OPT_STAGE 1): bit 0 the IResNet100 LDS-resident stages and the
 * fused layer1.0 transition, bit 1 the IRV1 stem (conv_stem160.hip), bit 2 IRV1 repeat_1 (conv_chain35.hip), bit 3
 * IRV1 repeat_2 (conv_chain.hip), bit 4 ResNet-50 layer3.1-3.5 (conv_chain_r50.hip), bit 5 ResNet-50 layer1.0-1.2
 * (conv_bneck28.hip), bit 6 the ResNet-50 stem conv + max-pool (conv_stem_r50.hip).  For A/B timing and for tests
 * that check one fused kernel against its members. */
#define FR_OPT_FUSED_MASK 10
int fr_set_option(fr_handle* h, int option, int value);
int fr_get_option(const fr_handle* h, int option);
/* Number of probes (since the gallery was first split) whose bf16x3 candidate proof failed and were
 * rescanned exactly (synchronizes the device). */
int fr_debug_match_fallbacks(fr_handle* h);
/* Number of gallery splits fr_match_eval's main pass takes for a batch of B probes (no device work). */
int fr_debug_match_eval_splits(fr_handle* h, int B);
/* The same for fr_match_range_count / fr_match_range_fill (the second dimension of their workspace). */
int fr_debug_match_range_splits(fr_handle* h, int B);
/* Number of bounded waits of the split stage kernels (layer2: two workgroups per image, layer1: four,
 * exchanging boundary rows per conv) that ran out before the partner published; 0 on a healthy device
 * (synchronizes the device).  Each one was either re-run (fr_embed's default) or reported as
 * FR_ERR_STAGE with NaN embeddings (FR_EMBED_ASYNC): never returned as a valid embedding. */
int fr_debug_stage_timeouts(fr_handle* h);
/* Number of forwards fr_embed ran again on the per-conv path because a split-stage wait ran out. */
int fr_debug_stage_reruns(fr_handle* h);

/* ---- debug: named intermediate tensors of the forward plan (per-layer drift tests) ----
 * Tensor names are the reference/oracle module whose output the tensor equals
 * (e.g. "backbone.layer2.0", "layer3.7.prelu", "model.repeat_1.2"); "" for internal buffers. */
/* ---- measurement: per-kernel-class timing with HIP events (bench.py roofline) --------------
 * No reference counterpart (the reference has no profiler hook); used by bench.py to time the
 * dominant kernel live, on the stream it is launched on.  fr_prof_enable(h, n) (n >= 1) resets and
 * starts recording an event pair around every n-th launch of fr_embed (conv launches are stamped by
 * their dispatch via hipExtLaunchKernel; n > 1 samples to keep the overhead small); n = 0 stops.
 * Profiled forwards launch eagerly (no hipGraph replay).  fr_prof_collect() waits for the pending
 * events and returns the number of kernel classes; fr_prof_get() reads class i: name (matches the
 * kernel instantiation), summed milliseconds, launch count, summed algorithmic FLOPs (2*M*N*K). */
int fr_prof_enable(fr_handle* h, int on);
/* Restrict timing to one kernel class (name as returned by fr_prof_get; NULL or "" = all).
 * Each event pair serializes the stream slightly, so bench.py times only the dominant class. */
int fr_prof_only(fr_handle* h, const char* kernel_class);
int fr_prof_collect(fr_handle* h);
/* Graph-slot timing (bench.py's timed steps, which replay hipGraphs like the product path):
 * fr_prof_slots(h, class, n) makes n event pairs (n = 0 frees them); with slot i selected
 * (fr_prof_slot_select, -1 = none) a forward records pair i around launch i mod L of `class` (L = the
 * class's launches per forward, counted by the first slot forward) -- captured into slot i's own graph, so
 * every replay of that graph re-stamps the pair on the launching stream; fr_prof_slot_ms reads pair i
 * (milliseconds between the two events), fr_prof_slot_work the timed launch's algorithmic FLOPs and bytes. */
int fr_prof_slots(fr_handle* h, const char* kernel_class, int n);
int fr_prof_slot_select(fr_handle* h, int slot);
int fr_prof_slot_ms(fr_handle* h, int slot, float* ms);
int fr_prof_slot_work(fr_handle* h, int slot, double* flops, double* bytes);
int fr_prof_get(const fr_handle* h, int i, char* name, size_t n, double* total_ms, int64_t* launches,
                double* flops);
/* Algorithmic HBM bytes of class i over its timed launches (each input / weight / output byte once;
 * re-reads through L2 and the Infinity Cache are not counted), for the class's HBM-roofline fraction. */
int fr_prof_get_bytes(const fr_handle* h, int i, double* bytes);

int fr_debug_tensor_count(const fr_handle* h);
/* Text dump of the forward plan at batch B, one line per op:
 * "conv|head M N K Kpad tile split KhxKw name", "stage M 256 2304 2304 nconv 1 3x3 name" or
 * "pre|maxpool|avgpool". */
int fr_debug_plan(fr_handle* h, int B, char* buf, size_t n);
const char* fr_debug_tensor_name(const fr_handle* h, int t);
int fr_debug_tensor_shape(const fr_handle* h, int t, int* H, int* W, int* C);
/* Copy the first B samples of tensor t (bf16 NHWC) to dst (device) after an fr_embed. */
/* Storage dtype of tensor t (FR_DTYPE_BF16 / FR_DTYPE_F16): a bf16 IRV1 plan keeps its high-resolution stem
 * tensors in f16, so fr_debug_copy_tensor's 16-bit elements are to be read in this dtype. */
int fr_debug_tensor_dtype(const fr_handle* h, int t);
int fr_debug_copy_tensor(fr_handle* h, int t, int B, void* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRHIP_H */
