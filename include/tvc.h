/*
 * tvc.h -- C ABI of the MI355X-native text-variant-consistency (TVC) hot path.
 *
 * The reference (Zhang-Xin-Duke/multimodal-detection-consistency) is pure
 * Python and has no FFI; its boundary for this path is duck-typed Python
 * (SURVEY.md section 8b).  This header is the C-ABI that sits underneath the
 * Python mirror in multimodal-detection-consistency_amd/: plain pointers and
 * sizes, no torch types.  Each entry point names the reference call sites it
 * replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer named *_dev is a DEVICE pointer owned by the caller
 *     (in practice a PyTorch-ROCm tensor's data_ptr());
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and
 *     the call never synchronises the device (exceptions are documented);
 *   - return value 0 = TVC_OK, otherwise an error code; the message is
 *     available from tvc_last_error();
 *   - a handle belongs to one GPU and is not thread-safe (the Python shim
 *     holds a lock around submission); entry points that share an internal
 *     workspace (two calls into the same tower, any two tvc_sd_* calls, two
 *     bank searches) must be issued on ONE stream or be ordered by the caller
 *     -- the vision tower, the text tower and the bank search each have their
 *     own workspace and may run on three streams side by side;
 *   - bf16 buffers are raw uint16_t bit patterns (round-to-nearest-even).
 */
#ifndef TVC_H_
#define TVC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TVC_ABI_VERSION 4
#define TVC_MAX_BANKS 8      /* bank slots per handle (tvc_bank_select)          */
#define TVC_MAX_TOPK 128     /* largest k of tvc_bank_search / tvc_topk_merge    */

enum {
    TVC_OK = 0,
    TVC_E_INVALID = 1,     /* bad argument / unsupported geometry            */
    TVC_E_HIP = 2,         /* a HIP runtime call failed                      */
    TVC_E_NOMEM = 3,       /* workspace allocation failed                    */
    TVC_E_STATE = 4,       /* e.g. bank search before tvc_bank_set           */
    TVC_E_OVERFLOW = 5     /* candidate lists overflowed (see tvc_bank_status) */
};

enum { TVC_DTYPE_BF16 = 0, TVC_DTYPE_F32 = 1 };

typedef struct tvc_handle tvc_handle;

/* Transformer tower geometry (CLIP style, pre-LN). */
enum { TVC_ACT_QUICK_GELU = 0, TVC_ACT_GELU = 1 };
typedef struct {
    int32_t width;    /* d_model                          */
    int32_t layers;
    int32_t heads;    /* head_dim = width / heads, must be 64 */
    int32_t mlp;      /* hidden size of the MLP           */
    int32_t act;      /* TVC_ACT_QUICK_GELU: x * sigmoid(1.702 x) (OpenAI CLIP, every tower the detector uses);
                         TVC_ACT_GELU: the exact erf GELU (OpenCLIP ViT-H/14, the text encoder of Stable Diffusion 2.x) --
                         applied by a row kernel after a store-only FC1, not in the GEMM epilogue; not available to
                         tvc_encode_image_grad */
} tvc_tower_arch;

typedef struct {
    int32_t image_size;   /* 224                                  */
    int32_t patch;        /* 32 (ViT-B/32), 14 (ViT-L/14)         */
    int32_t vocab;        /* 49408                                */
    int32_t ctx;          /* 77                                   */
    int32_t embed_dim;    /* D: 512 (B/32), 768 (L/14)            */
    tvc_tower_arch vision;
    tvc_tower_arch text;
} tvc_model_desc;

/* One residual attention block.  GEMM weights are bf16 [out, in] row-major
 * (the nn.Linear layout); LayerNorm parameters and biases are fp32. */
typedef struct {
    const float*    ln1_g;  const float* ln1_b;
    const uint16_t* wqkv;   /* [3d, d]  rows: q | k | v            */
    const float*    bqkv;   /* [3d]                                 */
    const uint16_t* wo;     /* [d, d]                               */
    const float*    bo;
    const float*    ln2_g;  const float* ln2_b;
    const uint16_t* w1;     /* [mlp, d]                             */
    const float*    b1;
    const uint16_t* w2;     /* [d, mlp]                             */
    const float*    b2;
} tvc_layer_weights;

typedef struct {
    const uint16_t* patch_w;   /* bf16 [d, Kp], Kp = round_up(3*patch*patch, 64), zero padded;
                                  columns ordered (c, ky, kx) like the conv weight          */
    const float* cls;          /* [d]                                                       */
    const float* pos;          /* [T, d], T = (image_size/patch)^2 + 1                      */
    const float* ln_pre_g;  const float* ln_pre_b;
    const float* ln_post_g; const float* ln_post_b;
    const uint16_t* proj;      /* bf16 [D, d]                                               */
    const tvc_layer_weights* layers;   /* HOST array of `vision.layers` structs            */
} tvc_vision_weights;

typedef struct {
    const float* tok_emb;      /* fp32 [vocab, d]                                           */
    const float* pos;          /* fp32 [ctx, d]                                             */
    const float* ln_final_g; const float* ln_final_b;
    const uint16_t* proj;      /* bf16 [D, d]                                               */
    const tvc_layer_weights* layers;   /* HOST array of `text.layers` structs              */
} tvc_text_weights;

/* fp32 copies of the same weights for the fp32-grade tower mode (TVC_OPT_TOWER_PRECISION): identical field order,
 * every tensor fp32, nothing rounded to bf16.  patch_w is the UNPADDED conv weight [d, 3*patch*patch]. */
typedef struct {
    const float* ln1_g;  const float* ln1_b;
    const float* wqkv;   const float* bqkv;
    const float* wo;     const float* bo;
    const float* ln2_g;  const float* ln2_b;
    const float* w1;     const float* b1;
    const float* w2;     const float* b2;
} tvc_layer_weights_f32;

typedef struct {
    const float* patch_w;      /* fp32 [d, 3*patch*patch], columns ordered (c, ky, kx) */
    const float* cls;  const float* pos;
    const float* ln_pre_g;  const float* ln_pre_b;
    const float* ln_post_g; const float* ln_post_b;
    const float* proj;         /* fp32 [D, d] */
    const tvc_layer_weights_f32* layers;   /* HOST array of `vision.layers` structs */
} tvc_vision_weights_f32;

typedef struct {
    const float* tok_emb;  const float* pos;
    const float* ln_final_g; const float* ln_final_b;
    const float* proj;         /* fp32 [D, d] */
    const tvc_layer_weights_f32* layers;   /* HOST array of `text.layers` structs */
} tvc_text_weights_f32;

/* ---- lifetime -------------------------------------------------------- */

uint32_t tvc_abi_version(void);

/* Create a handle on the current HIP device.  `vision`/`text` may be NULL
 * (no tower of that kind: tvc_encode_* then fails with TVC_E_STATE; `desc`
 * may be NULL when both are).  The weight buffers are referenced, not copied:
 * the caller keeps them alive.
 * Replaces: constructing the (absent) src.models CLIPModel(CLIPConfig(...))
 * -- src/detector.py:258-271, src/retrieval.py:356-361. */
int tvc_create(const tvc_model_desc* desc, const tvc_vision_weights* vision,
               const tvc_text_weights* text, tvc_handle** out);
void tvc_destroy(tvc_handle* h);

/* Message of the last error on `h` (or of the last failed tvc_create when
 * h == NULL).  Never NULL. */
const char* tvc_last_error(tvc_handle* h);

/* Options.  TVC_OPT_TEXT_PACKING (default 1): the text tower processes only the
 * tokens up to and including EOT of every text (ragged, packed rows).  Under the
 * causal mask later positions cannot influence the pooled EOT row, so the output
 * is bit-identical to the dense [T, ctx] computation while the work drops by
 * ctx / mean length.  With packing on, tvc_encode_text synchronises `stream`
 * once per call (it reads back the packed row count that sizes the GEMM grids).
 * TVC_OPT_MAX_CHUNK_IMAGES / _TEXTS: rows of a batch processed per pass
 * (workspace bound; defaults 512 / 4608).
 * TVC_OPT_BANK_FILTER (default 1): when tvc_bank_search is called without a moments
 * buffer, the bank pass multiplies one bf16 product per element, keeps every row whose
 * similarity could exceed the running bound (Cauchy-Schwarz margin from the bank's
 * largest row norms) and re-scores the kept rows in fp32: the same top-k set, values at
 * least as accurate, 1/2 (bf16 bank) or 1/3 (fp32 bank) of the matrix-core work.  0 forces
 * the all-products pass.
 * TVC_OPT_TEXT_GROUP (default 0 = off): G >= 2 declares that the rows passed to tvc_encode_text
 * come in consecutive groups of G texts whose first text is the original and the others its
 * variants (the layout of pipeline.detect: original + N variants).  A causal tower gives two texts
 * identical hidden states on their common token prefix, so a variant keeps only the rows from its
 * first differing token on and attends to the original's rows for the shared prefix.  Outputs are
 * bit-identical; needs text packing and T % G == 0, otherwise it is ignored for that call.
 * TVC_OPT_POOLED_LAST_LAYER (default 1): both towers are pooled at ONE token (the class token / the EOT token), so
 * in their LAST layer only that token's attention output, out-projection, ln_2 and MLP are ever read.  With the
 * option on, those are computed for the pooled rows only (K and V still come from every token): the embeddings
 * are unchanged (same fp32 sums in the same order) while 10/12 of the last layer's GEMM work is not done.  0 runs
 * the last layer over every token like the others.
 * TVC_OPT_TOWER_PRECISION (default 0): 0 = the towers multiply bf16 x bf16 on the MFMA units with fp32 accumulation
 * (the benchmarked path: embeddings within ~1e-3 of an fp32 CPU tower).  1 = fp32-grade towers: tvc_encode_image /
 * tvc_encode_text / tvc_encode_text_hidden run every GEMM on the exact-f32 matrix instruction (v_mfma_f32_32x32x2_f32)
 * with the fp32 weights registered by tvc_set_weights_f32, fp32 activations and fp32 attention -- embeddings within
 * ~1e-6 of the reference's fp32 CPU path (src/detector.py:461-485; configs/attacks/pgd.yaml:80 asks for fp32), so the
 * consistency scores meet the 1e-4 bar END TO END.  About 10x slower; validation and attack-generation mode, never the
 * benchmarked one.  Needs tvc_set_weights_f32 first (TVC_E_STATE otherwise).  The input-gradient entry points
 * (tvc_encode_image_grad / _backward) do not follow this option: their precision is TVC_OPT_GRAD_PRECISION's.
 * 2 = split-bf16 towers, the FAST <= 1e-4 mode: every activation and weight travels to the matrix cores as hi | lo bf16
 * planes (x = hi + lo to ~2^-17) and every product is three bf16 MFMAs (hi hi + hi lo + lo hi, fp32 accumulation); fp32
 * residual stream, LayerNorm, softmax and QuickGELU.  Scores within 1e-4 of the reference's fp32 CPU path END TO END at
 * about a third of the bf16 mode's matrix rate (mode 1: 1/16); EOT packing and prefix sharing are kept, the pooled last
 * layer is not.  Needs tvc_set_weights_f32 first; setting the option builds the weight planes (synchronises the device).
 * 3 = fp16 towers: the bf16 mode's launches, tiles and workspaces with IEEE fp16 instead of bf16 -- the fp16 weights
 * registered by tvc_set_weights_f16, fp16 LayerNorm outputs, QKV, attention output, MLP hidden and residual deltas, the
 * products on v_mfma_f32_16x16x32_f16 (the bf16 rate) with fp32 accumulation; fp32 residual stream, LayerNorm statistics,
 * softmax, bias and activations.  fp16 keeps 10 mantissa bits to bf16's 7 but its range ends at 65504: a value beyond it
 * becomes +-inf (never clamped) and the embedding goes non-finite.  EOT packing, prefix sharing and the pooled last layer
 * are kept, each with its bf16 guarantee.  The reference runs its towers in fp16 (configs/defenses/tvc.yaml: precision).
 * Needs tvc_set_weights_f16 first (TVC_E_INVALID otherwise: without fp16 weights the handle offers no mode 3).
 * The input-gradient entry points run in TVC_OPT_GRAD_PRECISION's mode whatever this option is.
 * Geometry limits: head_dim 64 and sequences of at most 288 tokens in modes 0, 1 and 3 (tvc_create refuses other towers),
 * at most 272 tokens in mode 2 (TVC_E_INVALID when the option is set).
 * TVC_OPT_GRAD_PRECISION (default 0): the precision of tvc_encode_image_grad / tvc_encode_image_backward, independent of
 * TVC_OPT_TOWER_PRECISION (bf16 detection with fp32-grade attack gradients is a legal pair).  0 = the bf16 path.  2 =
 * split-bf16 (the number of the tower mode it shares its forward with): the vision tower runs forward AND backward at fp32
 * grade -- every GEMM is three bf16 MFMA products on hi | lo planes (hi hi + hi lo + lo hi, fp32 accumulation), activations,
 * kept state and gradients travel in fp32, the attention forward and backward form their products the same way with an fp32
 * softmax -- so the input gradient agrees with fp64 autograd to ~1e-5 relative where mode 0 gives ~1e-2.  Mode 2 keeps the
 * scope of mode 0: vision tower, QuickGELU, one pass (B <= TVC_OPT_MAX_CHUNK_IMAGES), the input gradient only, no atomics,
 * bit-reproducible from run to run; at most 272 tokens, as tower mode 2.  It needs tvc_set_weights_f32 and the split weight
 * planes: setting the option to 2 builds them when the fp32 vision weights are registered (as TVC_OPT_TOWER_PRECISION = 2
 * does; synchronises the device), otherwise it is only recorded and tvc_encode_image_grad returns TVC_E_STATE naming what is
 * missing.  The planes of the transposed weights are built by the first backward and freed with the others.  Any other
 * value: TVC_E_INVALID (1 and 3 are left for exact-f32 and fp16 gradient modes).  The mode is fixed per forward:
 * tvc_encode_image_backward runs in the mode of the last tvc_encode_image_grad on the handle and returns TVC_E_STATE,
 * computing nothing, when the option has changed in between.
 * TVC_OPT_SD_ARENA_BYTES (default 48 GiB): budget of the activation arena of ONE UNet evaluation inside tvc_sd_generate.
 * The arena grows linearly with the samples of an evaluation (about 0.75 GB per image at 64 x 64 latents: both halves of
 * classifier-free guidance); a batch that would exceed the budget is generated in chunks of whole sampling loops -- every
 * image is independent of its batch mates, so chunking changes no pixel -- instead of failing with TVC_E_NOMEM.
 * TVC_OPT_SD_STREAMS (default 2; 1 = off): inside tvc_sd_generate the unconditional and the conditional half of a UNet
 * evaluation run on two HIP streams (the caller's and one the handle owns, forked / joined by events), each in its own
 * half of the arena: a launch of one half fills the compute units the other half's partial tile round leaves idle.  Every
 * sample's arithmetic is independent of its batch mates, so the images are bit-identical with 1 and 2.
 * TVC_OPT_SD_PRECISION (default 0): the 16-bit format of the latent-diffusion model.  0 = bf16.  1 = IEEE fp16, the dtype the
 * reference runs Stable Diffusion in (src/sd_ref.py:222 torch_dtype "float16"): every 16-bit tensor given to tvc_sd_load holds
 * fp16 bits, every 16-bit activation between kernels is fp16, the products run on v_mfma_f32_16x16x32_f16 (the bf16 rate) with
 * fp32 accumulation; the same launches, tiles, arena, K splits, streams and chunking as mode 0, each with its bit-identity
 * guarantee.  fp32 as in mode 0: GroupNorm / LayerNorm statistics, softmax, SiLU, GEGLU, biases, the time embedding's sin / cos,
 * classifier-free guidance, the scheduler arithmetic; latents, text states and images cross the ABI as fp32 in both modes.
 * fp16 keeps 10 mantissa bits to bf16's 7 but its range ends at 65504: a weight or an activation beyond it becomes +-inf (never
 * clamped) and the output goes non-finite.  tvc_sd_attention / _ex read their operands in the handle's format.
 * Any other value: TVC_E_INVALID.  The tensors registered by tvc_sd_load are one format, so a DIFFERENT value while a model is
 * loaded on the handle returns TVC_E_STATE (set it before tvc_sd_load; the value it already has is always accepted).
 * Independent of TVC_OPT_TOWER_PRECISION: the text states arrive as fp32 whatever mode the towers ran in. */
enum { TVC_OPT_TEXT_PACKING = 1, TVC_OPT_MAX_CHUNK_IMAGES = 2, TVC_OPT_MAX_CHUNK_TEXTS = 3,
       TVC_OPT_BANK_FILTER = 4, TVC_OPT_TEXT_GROUP = 5, TVC_OPT_POOLED_LAST_LAYER = 6, TVC_OPT_TOWER_PRECISION = 7,
       TVC_OPT_SD_ARENA_BYTES = 8, TVC_OPT_SD_STREAMS = 9, TVC_OPT_SD_PRECISION = 10, TVC_OPT_GRAD_PRECISION = 11 };
int tvc_set_option(tvc_handle* h, int32_t option, int64_t value);

/* Register fp32 copies of the tower weights for TVC_OPT_TOWER_PRECISION = 1 (either may be NULL).  Referenced, not
 * copied: the caller keeps the buffers alive.  Geometry = the desc given to tvc_create.
 * Replaces: loading the fp32 checkpoint in the (absent) src.models CLIPModel -- src/detector.py:258-271. */
int tvc_set_weights_f32(tvc_handle* h, const tvc_vision_weights_f32* vision, const tvc_text_weights_f32* text);

/* Register IEEE fp16 tower weights for TVC_OPT_TOWER_PRECISION = 3 (either may be NULL): the structs and layout of
 * tvc_create with every uint16_t* weight holding fp16 bits (patch_w padded to Kp columns like the bf16 one); the fp32
 * fields may alias the bf16 set's buffers.  Referenced, not copied.  Geometry = the desc given to tvc_create. */
int tvc_set_weights_f16(tvc_handle* h, const tvc_vision_weights* vision, const tvc_text_weights* text);

/* Bytes of device workspace currently held by the handle. */
uint64_t tvc_workspace_bytes(tvc_handle* h);

/* ---- encoders (K1, K2, K3 of SURVEY.md 2.3) -------------------------- */

/* pix_dev: fp32 [B, 3, image_size, image_size] (already preprocessed);
 * out_dev: fp32 [B, D], L2-normalised when `normalize` != 0.
 * Replaces clip_model.encode_image / encode_image_tensor(x, requires_grad=False):
 * src/detector.py:626,633; experiments/defenses/detector.py:238;
 * src/retrieval.py:407,609. */
int tvc_encode_image(tvc_handle* h, const float* pix_dev, int32_t B,
                     float* out_dev, int32_t normalize, void* stream);

/* tok_dev: int32 [T, ctx] CLIP BPE ids (SOT ... EOT, 0-padded); pooled at the
 * arg-max id (the EOT token).  out_dev: fp32 [T, D].
 * Replaces clip_model.encode_text: experiments/defenses/detector.py:239,247;
 * experiments/defenses/retrieval_ref.py:238-244; src/retrieval.py:451,551. */
int tvc_encode_text(tvc_handle* h, const int32_t* tok_dev, int32_t T,
                    float* out_dev, int32_t normalize, void* stream);

/* ---- reference bank (K5) --------------------------------------------- */

/* A handle holds TVC_MAX_BANKS independent bank slots so that several owners sharing one engine (the
 * retriever's image index src/retrieval.py:225, a ReferenceBank src/ref_bank.py:86, the defense detector's
 * reference features retrieval_ref.py:99) cannot replace each other's rows.  tvc_bank_select picks the slot
 * that tvc_bank_set / _search / _search_dense / _gather address from then on (default: slot 0). */
int tvc_bank_select(tvc_handle* h, int32_t slot);

/* Register the bank: dense row-major [R, D], rows L2-normalised
 * (scripts/build_faiss_indices.py:108-109,138; retrieval_ref.py:99,156).
 * dtype TVC_DTYPE_BF16: used in place (caller keeps it alive).
 * dtype TVC_DTYPE_F32: split once into bf16 (hi, lo) planes inside the handle
 * (3-product split-bf16 GEMM, fp32-grade cosines).
 * Replaces faiss.IndexFlatIP(d).add(features): src/retrieval.py:225-226,
 * retrieval_ref.py:140,156. */
int tvc_bank_set(tvc_handle* h, const void* bank_dev, int64_t R, int32_t D,
                 int32_t dtype, void* stream);

/* Exact top-k inner-product search of M query rows against the bank, fused
 * with per-row moments; the [M, R] matrix is never materialised.
 *   rows_dev   fp32 [M, D] (L2-normalised by the caller when cosines are wanted)
 *   k          1..TVC_MAX_TOPK (128)
 *   topk_idx   int32 [M, k]  global row index (local + idx_offset), -1 = none
 *   topk_sim   fp32  [M, k]  descending; ties broken by ascending index
 *   moments    fp32  [M, 4]  sum, sum of squares, max, count(sim >= count_thr)
 *                            over ALL R rows (may be NULL)
 * Replaces index.search(q, k) / np.dot + argpartition + argsort:
 * src/retrieval.py:636-673, retrieval_ref.py:246-290, src/ref_bank.py:475-484.
 * Returns TVC_OK after enqueueing; overflow of the internal candidate lists is
 * reported by tvc_bank_status() after the stream has been synchronised. */
int tvc_bank_search(tvc_handle* h, const float* rows_dev, int32_t M, int32_t k,
                    float count_thr, int64_t idx_offset,
                    int32_t* topk_idx_dev, float* topk_sim_dev, float* moments_dev,
                    void* stream);

/* Same contract as tvc_bank_search, computed by brute force (the similarities of up to 64 query
 * rows at a time are materialised and reduced): the fallback for degenerate banks on which
 * tvc_bank_status reports TVC_E_OVERFLOW.  Orders of magnitude slower; never overflows. */
int tvc_bank_search_dense(tvc_handle* h, const float* rows_dev, int32_t M, int32_t k,
                          float count_thr, int64_t idx_offset,
                          int32_t* topk_idx_dev, float* topk_sim_dev, float* moments_dev,
                          void* stream);

/* Synchronises `stream` and returns TVC_E_OVERFLOW if the last
 * tvc_bank_search dropped candidates (degenerate banks, e.g. thousands of
 * identical rows); TVC_OK otherwise. */
int tvc_bank_status(tvc_handle* h, void* stream);

/* out_dev fp32 [n, D]: bank rows for LOCAL indices idx_dev[n] (global index -
 * idx_offset); rows with idx < 0 or >= R are zero-filled.
 * Replaces self.reference_features[idx] (retrieval_ref.py:262,286). */
int tvc_bank_gather(tvc_handle* h, const int32_t* idx_dev, int32_t n,
                    int64_t idx_offset, float* out_dev, void* stream);

/* Merge W per-shard partial results (the RCCL all-gather / all-to-all output)
 * into the global top-k: parts are [W, M, k] (idx, sim) each sorted descending,
 * feat_parts fp32 [W, M, kf, D] or NULL carries the rows of the first kf
 * entries of every part; outputs as tvc_bank_search plus feat_out [M, kf, D].
 * mom_parts [W, M, 4] / mom_out [M, 4] may be NULL.  Limits: W * k <= 256, kf <= min(k, 32).
 * Replaces dist.all_gather + host merge (src/utils/multi_gpu_processor.py:595-612). */
int tvc_topk_merge(tvc_handle* h, const int32_t* idx_parts_dev, const float* sim_parts_dev,
                   const float* feat_parts_dev, const float* mom_parts_dev,
                   int32_t W, int32_t M, int32_t k, int32_t kf, int32_t D,
                   int32_t* idx_out_dev, float* sim_out_dev, float* feat_out_dev,
                   float* mom_out_dev, void* stream);

/* ---- k-means over a bank slot ------------------------------------------ */

/* Both entries work on the rows of the currently selected bank slot (tvc_bank_select / tvc_bank_set): any [R, D]
 * matrix, bf16 used in place or fp32 held as (hi | lo) bf16 planes.  The rows need not be unit length: the
 * clustering is Euclidean.  One Lloyd iteration is one assign and one update; the driver loop, the initialisation
 * and the stop rule are the caller's.  Together they replace KMeans(n_clusters, random_state = 42, n_init = 10)
 * .fit_predict(vectors) of src/ref_bank.py:294-300 and the training half of faiss.IndexIVFFlat
 * (src/retrieval.py:101-103,124-126, retrieval_ref.py:141-160, scripts/build_faiss_indices.py:139-142).
 * Both return TVC_E_STATE when the slot holds no bank or R == 0, and TVC_E_INVALID for K < 1, K > R, K > 65536
 * or a NULL required buffer; nothing is launched then. */

/* Assign: for every bank row x, labels[r] = argmax_j (x . c_j - |c_j|^2 / 2), the Euclidean nearest centre.
 *   centroids_dev  fp32 [K, D]
 *   labels_dev     int32 [R]; ties go to the lowest centre index (equality of the fp32 scores); NaN scores never
 *                  win, a row whose scores are all NaN gets -1
 *   score_dev      fp32 [R] or NULL: the winning score (-inf for label -1)
 *   dist2_dev      fp32 [R] or NULL: max(0, |x|^2 - 2 score), the squared distance to the centre (0 for label -1)
 * The [R, K] score matrix is never written: it lives in MFMA accumulators tile by tile.  Products in the bank
 * search's split-bf16 form: exact bf16 products against (hi | lo) centre planes for a bf16 bank, hi.hi + lo.hi +
 * hi.lo for an fp32 bank; |c|^2 / 2 is taken from the fp32 centres. */
int tvc_kmeans_assign(tvc_handle* h, const float* centroids_dev, int32_t K,
                      int32_t* labels_dev, float* score_dev, float* dist2_dev, void* stream);

/* Update: centroids_out[j] = the mean of the bank rows labelled j (hi + lo of an fp32 bank), fp32 sums in a fixed
 * order -- a counting sort of the row indices by label, stable, then one workgroup per cluster.  No floating-point
 * atomics: the result is a pure function of the bank and the labels, bit for bit.
 *   labels_dev         int32 [R]; labels outside [0, K) (the -1 of assign) belong to no cluster
 *   centroids_in_dev   fp32 [K, D]: a cluster with no member copies its row unchanged
 *   centroids_out_dev  fp32 [K, D] (must not alias centroids_in_dev)
 *   counts_dev         int32 [K]
 *   offsets_dev        int32 [K + 1] or NULL: exclusive scan of counts
 *   order_dev          int32 [R] or NULL: row indices grouped by cluster, ascending inside each cluster; entries
 *                      [offsets[j], offsets[j + 1]) are cluster j's members (the inverted-list layout), entries
 *                      from offsets[K] on are not written */
int tvc_kmeans_update(tvc_handle* h, const int32_t* labels_dev, const float* centroids_in_dev, int32_t K,
                      float* centroids_out_dev, int32_t* counts_dev, int32_t* offsets_dev, int32_t* order_dev,
                      void* stream);

/* ---- radius graph of a bank slot, and DBSCAN on a radius graph ---------------------------------------------- */

/* DBSCAN(eps, min_samples).fit_predict(vectors) of src/ref_bank.py:302-315 is a pure function of the eps-graph
 * A[i, j] = (|x_i - x_j|^2 <= eps^2), self included:
 *   1. degree[i] = sum_j A[i, j]; row i is a CORE row iff degree[i] >= min_samples;
 *   2. clusters = the connected components of the core-core subgraph, numbered 0 .. C - 1 in ascending order of each
 *      component's lowest core index;
 *   3. a non-core row with a core neighbour (a BORDER row) takes the lowest cluster id among its core neighbours, every
 *      other non-core row is noise (-1).
 * The graph is a bitmask uint32 [R, W], W = round_up(R, 64) / 32 (W(R) below): bit (j & 31) of word j / 32 of row i is
 * A[i, j].  tvc_radius_graph builds it from the selected bank slot; the two component calls take ANY such bitmask (they
 * read no bank slot), so a caller may cluster a graph of its own.  The centres of the clusters are tvc_kmeans_update
 * with K = n_clusters on the labels (it ignores -1, and its sums are in a fixed order).  The driver loop over the sweeps
 * is the caller's. */
#define TVC_RADIUS_MAX_ROWS 131072   /* rows of a radius graph: 2 GiB of bits */

/* The eps-graph of the rows of the selected slot (any [R, D] matrix; the rows need not be unit length).
 *   eps         finite, > 0 (an fp32 value: the test is against its square in fp32)
 *   adj_dev     uint32 [R, W(R)], 8-byte aligned.  Symmetric bit for bit; the padding bits (j >= R) are zero; the
 *               diagonal bit of every row with a finite norm is set; a row whose squared norm is not finite (NaN, inf
 *               or fp32 overflow) has no neighbours, not even itself
 *   degree_dev  int32 [R]: the popcount of the row, self included
 * The [R, R] products live in MFMA accumulators tile by tile (a self-GEMM of the slot, upper triangle of 256 x 256
 * tiles, then adj |= adj^T): a bf16 slot multiplies its stored values (exact products), an fp32 slot all four hi / lo
 * plane products.  The test is  x_i . x_j >= h_i + h_j,  h = |x|^2 / 2 - eps^2 / 4, in fp32: a pair whose squared
 * distance is within ~1e-5 |x_i| |x_j| of eps^2 may fall on either side.
 * TVC_E_STATE when the slot holds no bank or R == 0; TVC_E_INVALID when eps is not finite and positive, R >
 * TVC_RADIUS_MAX_ROWS, a buffer is NULL or adj is misaligned.  Nothing is launched on a refusal. */
int tvc_radius_graph(tvc_handle* h, float eps, uint32_t* adj_dev, int32_t* degree_dev, void* stream);

/* One sweep of minimum-label propagation on the bitmask adj [R, W(R)] with degrees degree [R].
 *   comp_dev     int32 [R]: with init != 0 first set to i for core rows and R for the others.  The sweep lowers comp[i]
 *                and comp[comp[i]] to the lowest label among row i's core neighbours (integer atomicMin), then every
 *                core row follows its chain of labels to its end.  The fixed point -- every core row holds the lowest
 *                core index of its component -- is unique; the number of sweeps that reach it is not.
 *   changed_dev  int32 [1]: a sweep that lowered a label ORs 1 into it (the caller zeroes it).  The labels are final
 *                after a sweep that left it 0; R sweeps always suffice.
 * Set bits at j >= R and labels outside [0, R) are skipped, never dereferenced. */
int tvc_dbscan_sweep(tvc_handle* h, const uint32_t* adj_dev, const int32_t* degree_dev, int32_t R, int32_t min_samples,
                     int32_t* comp_dev, int32_t* changed_dev, int32_t init, void* stream);

/* comp at its fixed point -> the labels of rules 2 and 3.
 *   labels_dev      int32 [R]
 *   core_dev        uint8 [R]: 1 for core rows
 *   n_clusters_dev  int32 [1]: C
 * Both component calls return TVC_E_INVALID for R < 1, R > TVC_RADIUS_MAX_ROWS, min_samples < 1 or a NULL buffer;
 * nothing is launched then. */
int tvc_dbscan_finish(tvc_handle* h, const uint32_t* adj_dev, const int32_t* degree_dev, int32_t R, int32_t min_samples,
                      const int32_t* comp_dev, int32_t* labels_dev, uint8_t* core_dev, int32_t* n_clusters_dev,
                      void* stream);

/* ---- pair lists of a bitmask graph, and the cosine of listed pairs ------------------------------------------- */

/* The data validator's near-duplicate and leakage checks (src/evaluation/data_validator.py:353-543) are pure functions of
 * "which pairs i < j have cosine >= t, and what is that cosine".  On unit rows cosine >= t is |x_i - x_j|^2 <= 2 - 2t, a
 * radius graph; these calls turn such a graph into the reference's pair list and give the listed pairs an fp32-grade
 * cosine (the graph itself is decided to ~1e-5 only).  The graph calls take ANY bitmask uint32 [R, W(R)] in
 * tvc_radius_graph's layout, symmetric or not, and read no bank slot. */

/* The rows' pair counts, scanned.
 *   adj_dev      uint32 [R, W(R)]
 *   group_dev    int32 [R] or NULL
 *   offsets_dev  int64 [R + 1]: offsets[i] = the number of pairs of the rows before i, offsets[R] = the exact total (int64:
 *                it may exceed 2^31)
 * The count of row i is the number of set bits j with i < j < R; with group_dev a bit also needs group[i] >= 0,
 * group[j] >= 0 and group[i] != group[j].  The lower triangle, the diagonal and the padding bits j >= R never count. */
int tvc_graph_pair_count(tvc_handle* h, const uint32_t* adj_dev, int32_t R, const int32_t* group_dev, int64_t* offsets_dev,
                         void* stream);

/* The pairs themselves, with the same adj, R and group and the offsets tvc_graph_pair_count wrote.
 *   pairs_dev    int32 [P, 2]: row i writes its pairs (i, j) in ascending j from slot offsets[i], so the list is
 *                lexicographic in (i, j) -- the order of the reference's nested loops -- and a pure function of
 *                (adj, group): no atomics.  A slot outside [0, P) is never written: with P < offsets[R] exactly the first
 *                P pairs arrive and nothing behind them is touched.
 * P == 0 is legal and launches nothing (pairs_dev may then be NULL).
 * Both graph calls return TVC_E_INVALID for R < 1, R > TVC_RADIUS_MAX_ROWS, P < 0 or a NULL adj, offsets or (P > 0)
 * pairs; nothing is launched then. */
int tvc_graph_pair_fill(tvc_handle* h, const uint32_t* adj_dev, int32_t R, const int32_t* group_dev,
                        const int64_t* offsets_dev, int32_t* pairs_dev, int64_t P, void* stream);

/* sim[p] = x . y / sqrt(|x|^2 |y|^2) for the stored rows x = pairs[p, 0], y = pairs[p, 1] of the selected slot (a bf16
 * slot: its stored values; an fp32 slot: hi + lo of every element).
 *   pairs_dev    int32 [P, 2]; any pairs, not only a graph's
 *   sim_dev      fp32 [P]
 * The three sums are fp32 FMA chains in a fixed order that depends on D alone, reduced in a fixed order:
 *   |sim - cos64(stored rows)| <= 2^-24 (2 D + 16),
 * bit-identical between runs and for (i, j) and (j, i).  sim is 0 when either row is all zero (and the other is not NaN);
 * NaN propagates; a pair with an index outside [0, R) gets NaN and its rows are never dereferenced.
 * TVC_E_STATE when the slot holds no bank rows; TVC_E_INVALID for P < 0 or, with P > 0, a NULL buffer.  P == 0 is legal
 * and launches nothing. */
int tvc_pair_cosine(tvc_handle* h, const int32_t* pairs_dev, int64_t P, float* sim_dev, void* stream);

/* ---- the closest pair of a bank slot -------------------------------------------------------------------------- */

/* Similarity eviction (src/ref_bank.py:395-427) asks a full bank for its most similar pair of stored vectors, which the
 * reference finds with a double loop over i < j.  Here it is one upper-triangle self-GEMM of the selected slot (any [R, D]
 * matrix; the rows need not be unit length) whose scores never leave the MFMA accumulators: a bf16 slot multiplies its stored
 * values, an fp32 slot all four hi / lo plane products, as tvc_radius_graph.
 *   partner_dev   int32 [R]: partner[i] = the arg-max over j > i of cos(x_i, x_j), (value descending, j ascending); -1 where
 *                 row i has no admissible later row: the last row, a row whose squared norm is not finite, a row all of
 *                 whose later rows have a non-finite norm
 *   sim_dev       fp32 [R]: that cosine, (x_i . x_j) / |x_j| / |x_i| in fp32; -inf where partner is -1
 *   pair_dev      int32 [2]: (i, partner[i]) of the best row under (sim descending, i ascending): the first maximal pair in
 *                 lexicographic (i, j) order, the pair a strict `>` over the reference's loops keeps; (-1, -1) when no row has
 *                 a partner
 *   pair_sim_dev  fp32 [1]: its cosine; -inf for (-1, -1)
 * An all-zero row has cosine 0 with every row (the reference's _cosine_similarity).  A row of non-finite norm is never a
 * partner.  With c64 = the fp64 cosine of the stored rows and tau = 1e-6:  |sim[i] - c64(i, partner[i])| <= tau  and
 * c64(i, partner[i]) >= max_{j > i} c64(i, j) - 2 tau,  and the same for pair / pair_sim over all i < j; where the
 * arithmetic is exact (rows of one common norm with a power-of-two 1 / norm and small-integer dot products) every tie falls
 * as stated above.  No atomics and no floating-point reduction across workgroups: the outputs are a pure function of the
 * slot, bit-identical between runs.
 * TVC_E_INVALID when h is NULL, the slot holds no bank, R < 1, an output is NULL or D is not a multiple of 64.  R == 1 is
 * legal and yields partner = -1, pair = (-1, -1).  Nothing is launched on a refusal. */
int tvc_closest_pair(tvc_handle* h, int32_t* partner_dev /*[R]*/, float* sim_dev /*[R]*/, int32_t* pair_dev /*[2]*/,
                     float* pair_sim_dev /*[1]*/, void* stream);

/* ---- retrieval evaluation over a bank slot: the rank of every relevant row ------------------------------------ */

/* Recall@K, Precision@K, mAP, MRR and NDCG@K (src/utils/metrics.py:379-573) are pure functions of the POSITIONS of a query's
 * relevant rows in its ranking of the gallery.  The reference takes them from a dense [Q, N] similarity matrix, a dense
 * [Q, N] relevance matrix, an argsort of every row and Python loops over every query and rank; these calls take them from
 * counts, over the rows of the selected bank slot (the gallery: bf16 in place or fp32 as (hi | lo) planes), and never
 * hold a [Q, N] matrix.
 *   score      S[i, j] = q_i . x_j in tvc_kmeans_assign's arithmetic: the queries split into (hi | lo) bf16 planes, two
 *              products on a bf16 slot, three (hi.hi + hi.lo + lo.hi) on an fp32 slot.  The caller normalises when cosines
 *              are wanted, as for tvc_bank_search.
 *   relevance  (i, j) is relevant iff qlabel[i] == glabel[j] >= 0.  A negative glabel is a distractor, relevant to nobody; a
 *              negative qlabel, or a label no row carries, is a query with no relevant row.  A relevant row of a query is
 *              one of its TARGETS; T is the total over the queries.
 *   order      (score descending, row index ascending): np.argsort(-S, kind = "stable"), tvc_bank_search's rule.
 *   position   of a target t of query i, 0-based:
 *                  pos(t) = (targets of i ahead of t) + (irrelevant rows j with (S[i, j], j) ahead of (S[i, t], t)).
 *              A NaN score is ahead of nothing.
 * Three calls.  tvc_rank_targets emits every query's targets; the caller puts each query's list in rank order (two stable
 * sorts); tvc_rank_count counts, per target, the irrelevant rows whose first target behind them it is; tvc_rank_metrics
 * turns the counts into positions and per-query metric terms.  The means over the queries are the caller's.
 * All three return TVC_E_STATE when the selected slot holds no bank rows, and TVC_E_INVALID for M < 1, T < 0 or a NULL
 * required buffer (tvc_rank_metrics also: more than TVC_RANK_MAX_K values of k, or a k < 1); nothing is launched then.
 * T == 0 is legal: the two tile calls launch nothing, tvc_rank_metrics writes its per-query zeros. */
#define TVC_RANK_MAX_K 8

/* EMIT: one pass over the [M, R] score tiles; every relevant element writes its score and row.
 *   rows_dev     fp32 [M, D], D = the slot's
 *   qlabel_dev   int32 [M]
 *   glabel_dev   int32 [R]
 *   gpos_dev     int32 [R]: the place of row j among the rows of its label, in ascending row order (unused where
 *                glabel[j] < 0)
 *   tgt_off_dev  int64 [M + 1]: the exclusive scan over the queries of their target counts; tgt_off[M] = T
 *   tgt_sim_dev  fp32 [T], tgt_row_dev int32 [T]: target (i, j) goes to slot tgt_off[i] + gpos[j], so a query's list is in
 *                ascending row order and every slot is written exactly once: no atomics, bit-identical between runs.  A
 *                slot outside the query's list (a gpos that is not the group's) is never written. */
int tvc_rank_targets(tvc_handle* h, const float* rows_dev, int32_t M, const int32_t* qlabel_dev, const int32_t* glabel_dev,
                     const int32_t* gpos_dev, const int64_t* tgt_off_dev, int64_t T, float* tgt_sim_dev, int32_t* tgt_row_dev,
                     void* stream);

/* COUNT: the same pass with the lists back, every query's in rank order (score descending, row ascending; finite scores).
 *   tgt_sim_dev, tgt_row_dev   [T], sorted
 *   hist_dev     int32 [T], zeroed by the caller: hist[tgt_off[i] + b] += 1 for every irrelevant row of query i that is
 *                ahead of the query's b-th target and of none before it (integer atomics: the result does not depend on the
 *                scheduling).  Relevant rows never count: the mutual order of a query's targets is the list's.
 * An irrelevant element is first compared with the score of the query's last target; only those at or above it search
 * the list (a binary search) and add.  Cost: one tile pass, plus one search and one atomic per irrelevant element that
 * is not below every target of its query -- at worst M * R of them. */
int tvc_rank_count(tvc_handle* h, const float* rows_dev, int32_t M, const int32_t* qlabel_dev, const int32_t* glabel_dev,
                   const int64_t* tgt_off_dev, const float* tgt_sim_dev, const int32_t* tgt_row_dev, int64_t T,
                   int32_t* hist_dev, void* stream);

/* Metrics: per query, with P its target count and pos[c] = c + sum_{b <= c} hist[b] the position of its c-th target in
 * rank order, in fp64:
 *   pos_dev    int32 [T]
 *   ap_dev     fp64 [M]: mean over c of (c + 1) / (pos[c] + 1)
 *   rr_dev     fp64 [M]: 1 / (pos[0] + 1)
 *   k_values   HOST int32 [n_k], n_k <= TVC_RANK_MAX_K, each >= 1
 *   hits_dev   int32 [M, n_k]: the number of targets with pos < k
 *   dcg_dev    fp64 [M, n_k]: sum over those targets of 1 / log2(pos + 2)
 *   idcg_dev   fp64 [M, n_k]: sum over c < min(k, P) of 1 / log2(c + 2)
 * A query without targets gets zeros (src/utils/metrics.py:469-470,511-512,558).  Any P from 0 to R works.  Nothing is
 * reduced over the queries on the device.  Reads no bank row. */
int tvc_rank_metrics(tvc_handle* h, int32_t M, const int64_t* tgt_off_dev, const int32_t* hist_dev, int64_t T,
                     const int32_t* k_values, int32_t n_k, int32_t* pos_dev, double* ap_dev, double* rr_dev,
                     int32_t* hits_dev, double* dcg_dev, double* idcg_dev, void* stream);

/* ---- detection evaluation: the ROC sweep of N scores under B integer weightings --------------------------------- */

/* AUROC, average precision, the Youden threshold, the FPR at a TPR target, the ROC / PR curves and their bootstrap
 * (src/utils/metrics.py:286-376, 816-874) are functions of the cumulative (TP, FP) counts over the scores in descending
 * order.  The caller sorts the N scores ONCE (descending, stable in the original index; finite fp32; -0.0 and 0.0 are one tie
 * group) and passes
 *   scores_dev  fp32  [N] sorted
 *   labels_dev  uint8 [N] in sorted order, 0 / 1
 *   order_dev   int32 [N]: the original index of every sorted position (an entry outside [0, N) weighs nothing)
 * A ROW weights the N samples by integer multiplicities w >= 0 (total < 2^31); the full sample is w = 1, a bootstrap resample
 * only changes w.  The multiplicities of the call's B rows come from one of three sources:
 *   TVC_ROC_SRC_WEIGHTS  src_dev int32 [B, N] over the ORIGINAL indices; NULL = all ones; a negative entry counts as 0
 *   TVC_ROC_SRC_INDICES  src_dev int32 [B, N] draws in [0, N) (any host RNG: np.random.choice(n, size = n)); a draw outside
 *                        the range is dropped
 *   TVC_ROC_SRC_PHILOX   drawn in the kernel, src_dev unused: draw t of resample b = first + row is word t & 3 of
 *                        Philox4x32-10 with counter (t >> 2, b, 0, 0) and key (seed & 0xffffffff, seed >> 32), mapped to
 *                        (uint64(x) * N) >> 32 -- a bias of at most N / 2^32.  `first` numbers the resamples across calls,
 *                        so a call cut into pieces gives the same rows.
 * The POINTS of a row are the ends of the tie groups whose weight is > 0, in sorted order, each with its cumulative (TP, FP);
 * P and N are the totals.  A row with P == 0 or N == 0 is invalid: valid = 0 and every other output 0, not an error.
 *   auc2     int64: sum over the points of (FP_g - FP_{g-1}) * (TP_g + TP_{g-1}); auc = double(auc2) / (2.0 * P * N)
 *   ap       fp64: sum of ((TP_g - TP_{g-1}) / P) * (TP_g / (TP_g + FP_g)); a fixed order, identical between runs
 *   curve    sklearn's roc_curve(drop_intermediate = True): a point is KEPT iff it is the first, the last, or the second
 *            difference of FP or of TP over the points is non-zero at it; the origin (0, 0), threshold +inf, comes first;
 *            tpr = double(TP) / double(P), fpr = double(FP) / double(N)
 *   youden   the first arg-max of tpr - fpr over the curve (origin included): its J, sorted position (-1: the origin), TP, FP
 *   target   the first arg-min of |tpr - target_tpr| over the same curve: sorted position, TP, FP
 *   thr      for each of n_thr <= TVC_ROC_MAX_THR fp32 thresholds (a HOST array): (TP, FP) of `score >= thr`
 * Up to TVC_ROC_LDS_ROWS samples a row's multiplicities live in LDS; above, in a handle workspace of at most 1 GiB, and the
 * rows of the call run in chunks that fit it.  Results never depend on the chunking.  Integer atomics only.
 * All three calls return TVC_E_INVALID, and launch nothing, for N < 1, N > TVC_ROC_MAX_N, B < 1, first < 0, an unknown source,
 * n_thr outside [0, TVC_ROC_MAX_THR], a target outside [0, 1] or a NULL required buffer (src_dev with INDICES). */
#define TVC_ROC_MAX_THR 8
#define TVC_ROC_LDS_ROWS 36864
#define TVC_ROC_MAX_N 16777216
#define TVC_ROC_SRC_WEIGHTS 0
#define TVC_ROC_SRC_INDICES 1
#define TVC_ROC_SRC_PHILOX 2

typedef struct tvc_roc_rows {
    const float* scores_dev;
    const uint8_t* labels_dev;
    const int32_t* order_dev;
    int32_t N;
    int32_t source;          /* TVC_ROC_SRC_* */
    const int32_t* src_dev;
    int64_t B;
    int64_t first;           /* PHILOX: the resample number of row 0 */
    uint64_t seed;           /* PHILOX */
} tvc_roc_rows;

/* per row, device arrays of B entries (thr_*: [B, n_thr], required when n_thr > 0) */
typedef struct tvc_roc_out {
    int32_t *n_pos, *n_neg, *valid, *n_points, *n_kept;
    int64_t* auc2;
    double *auc, *ap, *youden_j;
    int32_t *youden_pos, *youden_tp, *youden_fp;
    int32_t *target_pos, *target_tp, *target_fp;
    int32_t *thr_tp, *thr_fp;
} tvc_roc_out;

/* Read-back: w_dev int32 [B, N], the multiplicities of every row over the SORTED positions (w_dev[b, pos] weighs the sample
 * order[pos]) -- what the sweep gathers, from any source. */
int tvc_roc_weights(tvc_handle* h, const tvc_roc_rows* rows, int32_t* w_dev, void* stream);

/* The per-row results of every row of the call. */
int tvc_roc_sweep(tvc_handle* h, const tvc_roc_rows* rows, double target_tpr, const float* thresholds, int32_t n_thr,
                  const tvc_roc_out* out, void* stream);

/* The points of ONE row (rows->B == 1): pt_tp / pt_fp / pt_pos / pt_kept int32 [N] (the first count_dev[0] entries are
 * written), count_dev int32 [2] = (points, kept points); an invalid row has (0, 0).  The caller forms fpr / tpr / thresholds
 * from the kept points and the PR arrays from all of them. */
int tvc_roc_curve(tvc_handle* h, const tvc_roc_rows* rows, int32_t* pt_tp_dev, int32_t* pt_fp_dev, int32_t* pt_pos_dev,
                  int32_t* pt_kept_dev, int32_t* count_dev, void* stream);

/* ---- similarity metrics of pairs of rows; top-k overlap --------------------------------------------------------- */

/* Cosine similarity, Euclidean and Manhattan distance, Pearson and Spearman correlation (src/utils/metrics.py:89-106,166-276;
 * src/retrieval.py:158-193) of PAIRS of rows: the metrics of (x[b, :], y[b, :]) for every b in one launch, one workgroup a pair.
 *   x_dev, y_dev  [B, D] at row pitches ldx, ldy >= D (in elements); fp32 (TVC_SIM_KEY_F32) or int32 (TVC_SIM_KEY_I32: index
 *                 lists; an element converts to fp64 exactly and is ordered as an integer).  1 <= D <= TVC_SIM_MAX_D, any D.
 *   out_dev       fp64 [B, TVC_SIM_COLS]: cosine, Euclidean, Manhattan, Pearson, Spearman; columns 5 .. 7 are 0.0
 *   ints_dev      int64 [B, TVC_SIM_INTS]: the sums of cx cy, cx cx and cy cy over the centred doubled ranks (below), then the
 *                 number of NaN elements of the pair (x's and y's); the three sums are 0 when that number is not 0
 * With n = D and the elements taken to fp64:
 *   float sums    fp64; a thread adds its elements i = t, t + T, ... in that order (T = 64 threads for n <= 256, else 256), the
 *                 threads' sums meet in a fixed tree: the order depends on n alone, there are no atomics, and the results
 *                 are bit-identical between runs, launches and batch sizes.  No multiply-add is contracted.
 *   cosine        sum(x y) / sqrt(sum(x x) * sum(y y));  0.0 when either row is all zero and the pair has no NaN
 *   Euclidean     sqrt(sum((x - y)^2));   Manhattan  sum(|x - y|)
 *   Pearson       two passes: mx = sum(x) / n, my = sum(y) / n, then with cx = x - mx, cy = y - my
 *                 r = sum(cx cy) / sqrt(sum(cx cx) * sum(cy cy)), clamped to [-1, 1] (a NaN stays).  NaN when n < 2 or when
 *                 min == max over either row (the explicit constant-input test of scipy.stats.pearsonr: the mean of a constant
 *                 row need not round to its value, so a centred sum is no such test).
 *   Spearman      exact integers.  The doubled 1-based average rank of an element is lo + hi + 1, lo = the number of the
 *                 row's elements strictly below it, hi = the number at or below it; -0.0 ties with 0.0, +-inf order as
 *                 values.  The doubled ranks of a row sum to n (n + 1), so the centred doubled rank c = lo + hi - n is an
 *                 integer with |c| <= n - 1.  rho = sum(cx cy) / sqrt((double)sum(cx cx) * (double)sum(cy cy)) on the int64
 *                 sums (no rounding before the conversions).  NaN when n < 2, when an integer sum of squares is 0 (a
 *                 constant row) or when the pair holds any NaN.
 *   specials      NaN and +-inf otherwise propagate as the arithmetic yields; every NaN written is 0x7ff8000000000000.  A
 *                 pair never changes another pair's bits.
 * Accuracy against the exact value on the given elements, u = 2^-53, kappa = max(mean|x| / sigma_x, mean|y| / sigma_y):
 *   interface     cosine within B(n) = 2^-52 (2 n + 16) absolute, Euclidean and Manhattan within B(n) relative, Pearson
 *                 within B(n) + (2^-52 n kappa)^2.  (Products of fp32 values are exact in fp64; an n-term fp64 sum errs by at
 *                 most (n - 1) u sum|terms|; the error of a mean enters Pearson at second order only.)
 *   kernel        the same with the kernel's chain length c(n) in place of n: a term passes through at most
 *                 c(n) = min(n - 1, ceil(n / T) + 8) rounding additions (ceil(n / T) - 1 in its thread, 6 in the wave, 3
 *                 across the waves): cosine within Bk(n) = 2^-52 (c(n) + 2) absolute (sum(x y) errs by c u sqrt(sum(x x)
 *                 sum(y y)), the two sums of squares by c u relative each, product, root and quotient add 2.5 u),
 *                 Manhattan and Euclidean within Bk(n) relative (a term carries 1 u, a squared one 3 u; the root halves),
 *                 Pearson within 2^-52 (c(n) + 5) + (2^-52 (c(n) + 1) kappa)^2 (centring and the product add 3 u a term; a
 *                 mean errs by (c + 1) u mean|x|, which shifts each centred sum by n delta_x delta_y).  c(4096) = 24.
 *                 The long form below: c(n) = min(n - 1, 33).
 * TVC_E_INVALID, and nothing is launched, when h is NULL, B < 0, D is outside [1, TVC_SIM_MAX_D], a pitch is below D, the key
 * type is unknown, or a buffer is NULL with B > 0.  B == 0 is legal and launches nothing. */
#define TVC_SIM_MAX_D 4096
#define TVC_SIM_MAX_N 1048576
#define TVC_SIM_COLS 8
#define TVC_SIM_INTS 4
#define TVC_SIM_KEY_F32 0
#define TVC_SIM_KEY_I32 1
int tvc_sim_rows(tvc_handle* h, const void* x_dev, const void* y_dev, int64_t B, int32_t D, int64_t ldx, int64_t ldy, int32_t key_type,
                 double* out_dev /*[B, 8]*/, int64_t* ints_dev /*[B, 4]*/, void* stream);

/* The long form: ONE pair of fp32 vectors of n elements, TVC_SIM_MAX_D < n <= TVC_SIM_MAX_N (any n >= 1 is accepted), with the
 * outputs, formulas and specials of one row of tvc_sim_rows.  The caller sorts each vector's values ascending with NaN last
 * (only the sorted values are needed, no permutation).
 *   tvc_sim_flat_rank   crank_dev int32 [n]: the centred doubled rank lo + hi - n of every element of v_dev, by a fixed-step
 *                       lower and upper bound of the element's own value in sorted_dev: no scan, no dependency between
 *                       workgroups.  nan_count_dev int64 [1] (may be NULL): the NaN elements of the vector.
 *   tvc_sim_flat        out_dev fp64 [TVC_SIM_COLS], ints_dev int64 [TVC_SIM_INTS] from x, y and their centred ranks.  Both
 *                       passes (sums and means; centred sums) run as a partial kernel, whose workgroup b owns the elements
 *                       [4096 b, 4096 (b + 1)), and a one-workgroup finish kernel that adds the partials in a fixed order: grid
 *                       and order are functions of n alone, never of the device, and every hand-off between workgroups
 *                       crosses a kernel boundary.  ws_dev: 8-byte aligned scratch of at least tvc_sim_flat_workspace(n) =
 *                       8 (16 + 20 ceil(n / 4096)) bytes (0 for an n outside the range), not shared by concurrent calls.
 * TVC_SIM_MAX_N = 2^20 is what keeps n (n - 1)^2, the bound of a sum of squared centred doubled ranks, inside int64.
 * TVC_E_INVALID, and nothing is launched, when h is NULL, n < 1, n > TVC_SIM_MAX_N, a buffer is NULL (nan_count_dev excepted),
 * or the workspace is too small or misaligned. */
uint64_t tvc_sim_flat_workspace(int64_t n);
int tvc_sim_flat_rank(tvc_handle* h, const float* v_dev, const float* sorted_dev, int64_t n, int32_t* crank_dev /*[n]*/,
                      int64_t* nan_count_dev /*[1] or NULL*/, void* stream);
int tvc_sim_flat(tvc_handle* h, const float* x_dev, const float* y_dev, const int32_t* cx_dev, const int32_t* cy_dev, int64_t n,
                 double* out_dev /*[8]*/, int64_t* ints_dev /*[4]*/, void* ws_dev, uint64_t ws_bytes, void* stream);

/* Top-k overlap of two retrievals (src/retrieval.py:179-184): count_dev int32 [M], count[i] = |set(a[i, :k]) & set(b[i, :k])|
 * for a_dev int32 [M, La] and b_dev int32 [M, Lb].  Set semantics: an id repeated inside a list counts once.  A list shorter
 * than k is taken whole, as a Python slice is.  No id is special (negative ids are ids).  One wave per query, no atomics.
 * TVC_E_INVALID, and nothing is launched, when h is NULL, M < 0, La < 0, Lb < 0, k is outside [1, TVC_TOPK_OVERLAP_MAX_K], or a
 * buffer is NULL with M > 0.  M == 0 is legal and launches nothing. */
#define TVC_TOPK_OVERLAP_MAX_K 1024
int tvc_topk_overlap(tvc_handle* h, const int32_t* a_dev, const int32_t* b_dev, int64_t M, int32_t La, int32_t Lb, int32_t k,
                     int32_t* count_dev /*[M]*/, void* stream);

/* ---- IVF search: probe + list scan over a bank slot ------------------------------------------------ */

/* An IVF index over R rows is four things:
 *   centroids     fp32 [nlist, D]
 *   the rows      stored IN LIST ORDER in a bank slot (tvc_bank_set of bank[order]; bf16 or fp32)
 *   list_offsets  int32 [nlist + 1]: list l = the stored rows [list_offsets[l], list_offsets[l + 1]); empty lists are legal
 *   row_ids       int32 [R]: the original index of every stored row, ascending inside a list (the `order` of
 *                 tvc_kmeans_update's stable counting sort); NULL = identity
 * Probe: the nprobe lists of a query are the nprobe largest q . c - |c|^2 / 2, ties to the lower list id, NaN scores never
 * win -- the score and order of tvc_kmeans_assign, so a row sits in the list this rule ranks first for it.
 * Scan: the exact top-k by inner product of the query with the rows of its probed lists, in tvc_bank_search's contract:
 * global index = row_ids[pos] + idx_offset, order (similarity desc, index asc by ORIGINAL index), -1 / -inf padded when the
 * probed lists hold fewer than k rows, NaN similarities never returned.  No moments: they are defined over all R rows.
 * Together they replace faiss.IndexIVFFlat.search (src/retrieval.py:101-103,496-498, retrieval_ref.py:141-160,
 * scripts/build_faiss_indices.py:139-142).  DIFFERENCE from the reference: it builds IndexIVFFlat(IndexFlatIP(d), d, nlist)
 * without a metric argument, so its in-list distances are squared L2, ascending, which its callers read as similarities.  On
 * unit rows the ranking is the same (d^2 = 2 - 2 cos); this library returns the cosines, as the flat search does, so the
 * callers' thresholds keep their meaning.
 * Both calls enqueue and return (no host synchronisation); a refusal launches nothing and allocates nothing. */

/* The nprobe best lists of every query row; needs no bank.
 *   rows_dev       fp32 [M, D], D % 64 == 0
 *   centroids_dev  fp32 [nlist, D]
 *   lists_dev      int32 [M, nprobe]: list ids, best first.  nprobe is clamped to nlist as faiss does: the ranks from nlist
 *                  on (and the ranks a query with NaN scores cannot fill) are -1, which tvc_ivf_scan skips
 *   score_dev      fp32 [M, nprobe] or NULL: the scores (-inf where lists_dev is -1)
 * TVC_E_INVALID: nprobe outside 1..TVC_MAX_TOPK, nlist outside 1..65536, D <= 0 or D % 64 != 0, M < 0, a NULL required buffer. */
int tvc_ivf_probe(tvc_handle* h, const float* rows_dev, int32_t M, int32_t D,
                  const float* centroids_dev, int32_t nlist, int32_t nprobe,
                  int32_t* lists_dev, float* score_dev, void* stream);

/* Exact top-k over the probed lists of the SELECTED slot, whose rows are stored in list order.
 *   rows_dev        fp32 [M, D], D = the slot's
 *   probes_dev      int32 [M, nprobe]: list ids, -1 (any id outside [0, nlist)) = skip; a list named twice in one row is
 *                   the caller's error
 *   max_list_rows   the longest list, known to whoever built the index.  A probed list that is longer is read up to its
 *                   first max_list_rows rows AND raises the overflow word: tvc_bank_status then reports TVC_E_OVERFLOW
 *                   (never a silent truncation)
 *   topk_idx_dev    int32 [M, k], topk_sim_dev fp32 [M, k]
 *   topk_pos_dev    int32 [M, k] or NULL: the stored position of each result (what tvc_bank_gather takes), -1 in the padding
 * The similarities of a chunk of queries with their probed lists go through a score workspace of at most 256 MiB
 * (nprobe x round_up(max_list_rows, 16) floats per query); the queries are chunked to fit.
 * TVC_E_STATE: the selected slot holds no bank rows.  TVC_E_INVALID: k or nprobe outside 1..TVC_MAX_TOPK, nlist outside
 * 1..65536, max_list_rows < 1, M < 0, a NULL required buffer, a slot whose D is not one of {128, 512, 768} (the widths the
 * row stream covers), or nprobe x round_up(max_list_rows, 16) x 4 bytes above the 256 MiB workspace. */
int tvc_ivf_scan(tvc_handle* h, const float* rows_dev, int32_t M, int32_t k,
                 const int32_t* probes_dev, int32_t nprobe,
                 const int32_t* list_offsets_dev, int32_t nlist, int32_t max_list_rows,
                 const int32_t* row_ids_dev, int64_t idx_offset,
                 int32_t* topk_idx_dev, float* topk_sim_dev, int32_t* topk_pos_dev, void* stream);

/* All-pairs cosine matrix out[n, m] = cos(x[n], y[m]), fp32-grade (both sides
 * L2-normalised on device, split into bf16 (hi, lo) planes, three MFMA products).
 * x fp32 [N, D], y fp32 [M, D], out fp32 [N, M]; D % 64 == 0.
 * Replaces sklearn cosine_similarity / F.normalize + mm:
 * src/retrieval.py:706 (compute_similarity_matrix), src/utils/metrics.py:144-164. */
int tvc_cosine_matrix(tvc_handle* h, const float* x_dev, int32_t N, const float* y_dev, int32_t M,
                      int32_t D, float* out_dev, void* stream);

/* Token-level output of the text tower: out fp32 [T, ctx, width] = ln_final(hidden states) at EVERY position
 * (no pooling, no projection, no EOT packing; causal mask as in tvc_encode_text) -- what a latent-diffusion
 * pipeline conditions its UNet on (`CLIPTextModel(...).last_hidden_state`; SURVEY.md 8f rank 1: the text encoder of
 * the SD reference generator, src/sd_ref.py:389-412 via StableDiffusionModel.generate_image). */
int tvc_encode_text_hidden(tvc_handle* h, const int32_t* tok_dev, int32_t T, float* out_dev, void* stream);

/* ---- input gradient of the vision tower -------- */

/* What `encode_image_tensor(x, requires_grad=True)` + `loss.backward()` give a white-box attack
 * (src/attacks/pgd_attack.py:456-486, src/attacks/hubness_attack.py:269-424, src/models/clip_model.py:200-221):
 * the embedding AND d(loss)/d(pixels).  Only the INPUT gradient exists -- the weights are frozen in every
 * attack of the reference -- so no weight-gradient GEMM is ever run.
 *
 * tvc_encode_image_grad: the tower of tvc_encode_image (every layer over every token; the FC1 pre-activation is
 *   rounded to bf16 before QuickGELU because it is kept: embeddings agree with tvc_encode_image within the tower's
 *   bf16 tolerance, ~1e-3, not bitwise; B must fit one pass, B <= TVC_OPT_MAX_CHUNK_IMAGES) and KEEPS, inside the handle, what the backward of each layer reads: its
 *   fp32 input rows, its QKV rows, its out-projection output and the FC1 pre-activation (20 * width bytes per
 *   token row and layer: 3.9 GB at ViT-L/14 and 32 images), plus the un-normalised embedding and the ln_post
 *   input.  pix_dev must stay valid and unchanged until the matching backward (the stem is recomputed from it).
 * tvc_encode_image_backward: grad_out fp32 [B, D] = d(loss)/d(out of the LAST tvc_encode_image_grad on this
 *   handle) -> grad_pix fp32 [B, 3, S, S] in the preprocessed (normalised) pixel space.  Four dX GEMMs per layer
 *   (= the forward's GEMM work once more) with fused row kernels between them and a two-pass attention backward;
 *   nothing of the forward is recomputed.  Gradients travel between GEMMs in bf16 and accumulate along the
 *   residual stream in fp32.  Deterministic (no atomics).  May be called repeatedly for different grad_out.
 * The above is TVC_OPT_GRAD_PRECISION = 0.  With 2 both calls run the split-bf16 tower instead: the forward is tower mode 2's
 *   over every token of every layer (embeddings as tvc_encode_image's in that mode), what it keeps is fp32 -- 4 * (5 * width +
 *   mlp) bytes per token row and layer, 7.3 GB at ViT-L/14 and 32 images --, and the backward runs the same steps with fp32
 *   gradients, each dX GEMM as three plane products against the transposed weight's hi | lo planes. */
int tvc_encode_image_grad(tvc_handle* h, const float* pix_dev, int32_t B, float* out_dev, int32_t normalize, void* stream);
int tvc_encode_image_backward(tvc_handle* h, const float* grad_out_dev, float* grad_pix_dev, void* stream);

/* One projected-gradient step on a batch of B images of n elements each, in place on adv_dev
 * (src/attacks/pgd_attack.py:500-521):
 *   momentum_dev != NULL:  m = mu * m + grad / |grad|_1 (per image);  step direction sign(m);  else sign(grad)
 *   adv = clamp(clean + clamp(adv +- alpha * sign - clean, -eps, eps), clip_min, clip_max)   ('-' when targeted) */
int tvc_pgd_step(tvc_handle* h, float* adv_dev, const float* clean_dev, const float* grad_dev, float* momentum_dev,
                 int32_t B, int64_t n, float eps, float alpha, float mu, float clip_min, float clip_max,
                 int32_t targeted, void* stream);

/* The L2-constrained step of the Hubness attack (src/attacks/hubness_attack.py:378-386), in place on adv_dev, per image:
 *   adv += (descent ? -1 : +1) * step * grad / (|grad|_2 + 1e-8);  d = adv - clean;  d *= min(|d|_2, eps) / (|d|_2 + 1e-8);
 *   adv = clamp(clean + d, clip_min, clip_max) */
int tvc_l2_step(tvc_handle* h, float* adv_dev, const float* clean_dev, const float* grad_dev, int32_t B, int64_t n, float eps,
                float step, float clip_min, float clip_max, int32_t descent, void* stream);

/* ---- FSTA / SMA attacks (src/attacks/fsta_attack.py, src/attacks/sma_attack.py) -------- */

#define TVC_ATTACK_METRIC_COSINE 0
#define TVC_ATTACK_METRIC_EUCLIDEAN 1
#define TVC_ATTACK_NORM_INF 0
#define TVC_ATTACK_NORM_L2 1

/* d(loss)/d(image embedding) of the feature loss both attacks share (fsta_attack.py:203-207,254-297, sma_attack.py:262-266,
 * 320-373).  f (image rows, as tvc_encode_image_grad wrote them), t (text rows), g (target rows): fp32 [B, D], rows of any
 * length.  With n_i = |f_i|, fh = f / n, vh = v / |v|, S = sum_j fh_j:
 *   L = a_tgt mean_i cos(f_i, g_i) + a_txt mean_i cos(f_i, t_i) + w_out mse(f, g) + w_div sum_{i != j} cos(f_i, f_j) / (B (B - 1))
 *   grad_i = a_tgt (gh_i - (fh_i.gh_i) fh_i) / (n_i B) + a_txt (th_i - (fh_i.th_i) fh_i) / (n_i B)
 *          + 2 w_out (f_i - g_i) / (B D) + 2 w_div ((S - fh_i) - (fh_i.S - 1) fh_i) / (n_i B (B - 1))
 * metric = TVC_ATTACK_METRIC_EUCLIDEAN: the two cosine terms are -a_tgt mean |f_i - g_i| - a_txt mean |f_i - t_i| instead,
 *   with gradient -a (f_i - v_i) / (|f_i - v_i| B), 0 where the distance is 0.
 * B = 1: the diversity term and its gradient are 0.  A weight of 0 switches its term off (a NaN row then cannot reach the
 * other rows).  grad is the exact gradient, not projected onto the tangent of the unit sphere: tvc_encode_image_backward's
 * own L2-normalise backward does that.
 * loss_rows fp32 [B, 4] = cos(f_i, g_i) | cos(f_i, t_i) | sum_c (f_ic - g_ic)^2 / D | sum_{j != i} cos(f_i, f_j)  (columns 0 and
 *   1 hold the distances under the Euclidean metric): every loss term is a mean of a column.
 * FSTA: a_tgt = -feature_weight, a_txt = +feature_weight, w_out = output_weight, w_div = diversity_weight.
 * SMA : a_tgt = -k, a_txt = +k, k = semantic_weight (1 + semantic_shift_strength), w_out = 0, w_div = diversity_weight.
 * Fixed summation order, no atomics: bit-identical from run to run.  B = 0 or D = 0: nothing is done. */
int tvc_attack_feature_grad(tvc_handle* h, const float* f_dev, const float* t_dev, const float* g_dev, int32_t B, int32_t D,
                            float a_tgt, float a_txt, int32_t metric, float w_out, float w_div, float* grad_dev,
                            float* loss_rows_dev, void* stream);

/* One step of the FSTA / SMA loops on B images of n elements, in place on adv_dev and mom_dev (fsta_attack.py:213-243,
 * sma_attack.py:272-302,701-731):
 *   g = grad + p (adv - clean);  clip > 0: g = clamp(g, -clip, clip);  m = mu m + g
 *   TVC_ATTACK_NORM_INF: a = adv - lr sign(m);  adv = clamp(clean + clamp(a - clean, -eps, eps), clip_min, clip_max)
 *   TVC_ATTACK_NORM_L2 : a = adv - lr m;  d = a - clean;  d *= min(1, eps / (|d|_2 + 1e-8)) per image;
 *                        adv = clamp(clean + d, clip_min, clip_max)
 * p = 2 perceptual_weight / (B n) is SMA's pixel-space term perceptual_weight mse(adv, clean), which never passes the tower;
 * p = 0 and clip <= 0 leave their operation out (the bits are those of a step without it).  mom_dev is required.
 * B = 0 or n = 0: nothing is done. */
int tvc_attack_step(tvc_handle* h, float* adv_dev, const float* clean_dev, const float* grad_dev, float* mom_dev, int32_t B,
                    int64_t n, float eps, float lr, float mu, float clip, float p, float clip_min, float clip_max, int32_t norm,
                    void* stream);

/* ---- per-query consistency (K4, K6, K7) ------------------------------ */

typedef struct {
    int32_t reference_count;      /* refs kept per text row, retrieval_ref.py:23 (5)   */
    float   similarity_threshold; /* retrieval_ref.py:24 (0.3)                         */
    int32_t retrieval_top_k;      /* experiments/defenses/detector.py:29 (10), <= 16   */
    float   dup_threshold;        /* experiments/defenses/detector.py:318 (0.95)       */
    float   w_text_variants;      /* src/detector.py:667 (0.4); 0 = method off.  With N == 0 and a weight > 0 the
                                     method still enters the weighted mean with score 0.0 (augmenter present but
                                     no variants, src/detector.py:375-378,457-458)                            */
    float   w_consistency;        /* src/detector.py:669 (0.2)                         */
    float   w_exp[4];             /* consistency_checker.py:61-66 (0.25 each): original,
                                     text_variant, retrieval, generative               */
} tvc_consistency_params;

/* Record layout, fp32 words per query (tvc_consistency writes rec_stride words):
 *  [0] original_similarity s0      [1] mean(sv)       [2] std(sv) (ddof 0)
 *  [3] text-variant score  (src/detector.py:479-485)
 *  [4] consistency score 1-s0 (src/detector.py:579)
 *  [5] aggregated src score (weighted_mean over the two, src/detector.py:664-680)
 *  [6] retrieval_consistency  [7] retrieval_std  [8] number of refs kept
 *  [9] cross_modal_variance (experiments/defenses/detector.py:295-300)
 * [10] overall score, weighted voting (consistency_checker.py:147-160)
 * [11] reserved
 * [12 .. 12+N)        sv[n]
 * [12+N .. +16)       kept reference indices (int32 bit patterns, -1 padded)
 * [12+N+16 .. +16)    cos(image, kept reference) */
#define TVC_REC_HEAD 12
#define TVC_REC_MAXREF 16
static inline int32_t tvc_rec_stride(int32_t N) { return TVC_REC_HEAD + N + 2 * TVC_REC_MAXREF; }

/* img_dev fp32 [B, D]; txt_dev fp32 [B, N+1, D] (row 0 = original text);
 * ref_idx/ref_sim [B*(N+1), ks] = bank search results of the text rows
 * (global indices), ref_feat fp32 [B*(N+1), kf, D] = rows of the first kf
 * (>= reference_count) results; pass ks = 0 / NULLs for "no bank".
 * To reproduce the reference's sort / filter / slice (retrieval_ref.py:206-216)
 * each ref_sim row must be non-increasing over its entries with ref_idx >= 0,
 * as tvc_bank_search and tvc_topk_merge return it.  The kernel does not sort: it
 * looks at the first min(reference_count, ks, kf) entries of each row, in order,
 * and keeps those with ref_idx >= 0 and ref_sim >= similarity_threshold; later
 * entries are never read, whatever their similarity.
 * Limits (TVC_E_INVALID otherwise, nothing is launched): N + 1 <= 40,
 * (N + 1) * reference_count <= 320, 0 <= retrieval_top_k <= 16, and ks > 0
 * needs all three ref_* buffers and kf >= 1.
 * rec_dev fp32 [B, tvc_rec_stride(N)].
 * Replaces src/detector.py:461-485,573-579,643-682 and
 * experiments/defenses/detector.py:184-204,228-300,302-325. */
int tvc_consistency(tvc_handle* h, const float* img_dev, const float* txt_dev,
                    int32_t B, int32_t N, int32_t D,
                    const int32_t* ref_idx_dev, const float* ref_sim_dev,
                    const float* ref_feat_dev, int32_t ks, int32_t kf,
                    const tvc_consistency_params* params, float* rec_dev, void* stream);

/* ---- in-process kernel timing (HIP events on the launch stream) ------- */

enum { TVC_PROF_GEMM = 0, TVC_PROF_ATTENTION = 1, TVC_PROF_BANK = 2, TVC_PROF_ROWOPS = 3, TVC_PROF_NCAT = 4 };

/* After tvc_profile_begin every kernel launch made through `h` is bracketed by
 * a pair of hipEvents on its stream.  tvc_profile_end synchronises, then fills
 * per category (index = TVC_PROF_*): ms[c] = summed kernel time, work[c] =
 * summed algorithmic FLOPs (GEMM, attention, bank) or bytes (row ops),
 * launches[c] = number of launches; profiling is switched off again.  big_gemm (double[3], may be NULL): over the GEMM
 * launches of >= 64 output tiles (the persistent ring kernels, the `roofline` kernel of bench.py) -- [0] their summed
 * COMPULSORY HBM bytes (every distinct operand plane read once, the output written once), [1] their count, [2] their ms:
 * the denominator that roofline.traffic (PMC bytes per launch) is compared with. */
int tvc_profile_begin(tvc_handle* h);
int tvc_profile_end(tvc_handle* h, double* ms, double* work, int64_t* launches, double* big_gemm);

/* ---- building blocks exported for parity tests and profiling --------- */

/* out[j, i] = sum_k a[i, k] * b[j, k]  (+ bias[i]); a bf16 [I, lda] ("weights"),
 * b bf16 [J, ldb] ("tokens"); K % 64 == 0; lda / ldb = row strides in elements (0 = K, i.e. dense rows;
 * otherwise >= K, a multiple of 8 and below 2^23); only the first K columns of a row are read.  out [J, ld_out],
 * ld_out >= I (any value): only out[j, i] for j < J, i < I is written (read too by epilogue 3).  a_dev, b_dev, out_dev
 * and a non-NULL bias_dev must be 16-byte aligned.  A call that breaks any of these returns TVC_E_INVALID and launches
 * nothing.  epilogue: 0 = fp32 store, 1 = bf16 store, 2 = bf16 quick-GELU, 3 = fp32 residual add (out += ...). */
int tvc_gemm_bf16(tvc_handle* h, const uint16_t* a_dev, const uint16_t* b_dev,
                  const float* bias_dev, void* out_dev, int32_t I, int32_t J, int32_t K,
                  int64_t lda, int64_t ldb, int32_t ld_out, int32_t epilogue, void* stream);

/* Multi-head attention over packed sequences: qkv bf16 [rows, 3*width]
 * (q | k | v), sequences of `seq_len` consecutive rows, out bf16 [rows, width]. */
int tvc_attention(tvc_handle* h, const uint16_t* qkv_dev, uint16_t* out_dev,
                  int32_t n_seq, int32_t seq_len, int32_t heads, int32_t causal, void* stream);

/* y bf16 [rows, d] = LayerNorm(x fp32 [rows, d]) * g + b, eps 1e-5. */
int tvc_layernorm(tvc_handle* h, const float* x_dev, const float* g_dev, const float* b_dev,
                  uint16_t* y_dev, int32_t rows, int32_t d, void* stream);

/* fp16 twins of the three blocks above (TVC_OPT_TOWER_PRECISION = 3): every 16-bit operand and output is IEEE fp16
 * (tvc_gemm_f16: the arguments and preconditions of tvc_gemm_bf16; epilogues 1 / 2 store fp16, an output beyond 65504
 * becomes +-inf).  tvc_attention_f16 also takes
 * starts_dev: int32 [n_seq + 1] = packed sequences of at most seq_len rows, or NULL = n_seq x seq_len dense rows. */
int tvc_gemm_f16(tvc_handle* h, const uint16_t* a_dev, const uint16_t* b_dev,
                 const float* bias_dev, void* out_dev, int32_t I, int32_t J, int32_t K,
                 int64_t lda, int64_t ldb, int32_t ld_out, int32_t epilogue, void* stream);
int tvc_attention_f16(tvc_handle* h, const uint16_t* qkv_dev, uint16_t* out_dev, const int32_t* starts_dev,
                      int32_t n_seq, int32_t seq_len, int32_t heads, int32_t causal, void* stream);
int tvc_layernorm_f16(tvc_handle* h, const float* x_dev, const float* g_dev, const float* b_dev,
                      uint16_t* y_dev, int32_t rows, int32_t d, void* stream);

/* The tower attention kernel with every launch option (parity tests): qkv / out bf16, or IEEE fp16 when f16 != 0.
 * starts_dev: int32 [n_seq + 1] = packed sequences of at most seq_len rows, or NULL = n_seq x seq_len dense rows.
 * pfx_dev (optional, causal packed rows only), int32 [2 * n_seq]: sequence s = pfx[s] rows starting at packed row
 * pfx[n_seq + s] (shared prefix, keys only) followed by its own rows [starts[s], starts[s+1]) (keys + queries); pfx[s] is
 * the prefix length, pfx[n_seq + s] the packed row of the prefix's position 0, and seq_len bounds prefix + own rows.
 * pool_mode 0: out [rows, width], every own row's output.  1 / 2: only the pooled token's output per sequence (1 = its
 * first token, 2 = its EOT token: the last packed row, or packed row pool_row_dev[s] (int32 [n_seq]) for dense rows),
 * written to the compact row s of out [n_seq, width].
 * Returns TVC_E_INVALID and launches nothing for: pfx without starts or without causal, pool_mode 2 on dense rows without
 * pool_row, pool_mode outside 0..2, seq_len outside 1..288, heads < 1, NULL qkv / out. */
int tvc_attention_ex(tvc_handle* h, const uint16_t* qkv_dev, uint16_t* out_dev, const int32_t* starts_dev,
                     const int32_t* pfx_dev, int32_t n_seq, int32_t seq_len, int32_t heads, int32_t causal,
                     int32_t pool_mode, const int32_t* pool_row_dev, int32_t f16, void* stream);

/* Backward of tvc_attention (non-causal, fixed-length sequences, head_dim 64): qkv as the forward saw it,
 * dout bf16 [rows, width] = gradient w.r.t. the attention output, dqkv bf16 [rows, 3*width] (dq | dk | dv).
 * Launches nothing and returns TVC_E_INVALID for a NULL buffer or a negative count, TVC_E_HIP for seq_len outside
 * 1..288 or heads < 1 with n_seq > 0; n_seq = 0 is TVC_OK and writes nothing. */
int tvc_attention_backward(tvc_handle* h, const uint16_t* qkv_dev, const uint16_t* dout_dev, uint16_t* dqkv_dev,
                           int32_t n_seq, int32_t seq_len, int32_t heads, void* stream);

/* LayerNorm input gradient: x fp32 [rows, d] (the forward's input), dy bf16 [rows, d], gamma fp32 [d],
 * dres fp32 [rows, d] or NULL (added: the residual path's gradient), dx fp32 [rows, d]. */
int tvc_layernorm_backward(tvc_handle* h, const float* x_dev, const uint16_t* dy_dev, const float* g_dev,
                           const float* dres_dev, float* dx_dev, int32_t rows, int32_t d, void* stream);

/* ---- latent-diffusion reference generator (BASELINE configs[4]) -------------------------
 * What src/sd_ref.py:389-399 (StableDiffusionModel.generate_image) and experiments/defenses/generative_ref.py:139-147
 * (sd_model.generate) reach through diffusers.StableDiffusionPipeline: the UNet2DConditionModel denoising loop with
 * classifier-free guidance under the PNDM (PLMS) scheduler, then AutoencoderKL.decode.  Geometry = the config.json
 * files the reference holds (cache/sd/models--runwayml--stable-diffusion-v1-5/snapshots/<rev>/{unet,vae,scheduler}), or
 * Stable Diffusion 2.x (src/__init__.py:110-113 lists stable-diffusion-2-1): per-level head counts, linear proj_in /
 * proj_out ([C, C] weights -- a 1 x 1 convolution on token rows is the same GEMM), cross-attention width 1024,
 * optionally v-prediction.
 * Activations are 16-bit token-major (NHWC) between GEMMs -- bf16, or IEEE fp16 with TVC_OPT_SD_PRECISION = 1 --, statistics /
 * softmax / scheduler arithmetic fp32. */
typedef struct {
    int32_t in_channels, out_channels;           /* 4, 4                                            */
    int32_t n_blocks;                            /* 4                                               */
    int32_t block_out_channels[4];               /* 320, 640, 1280, 1280                            */
    int32_t down_block_attn[4];                  /* 1, 1, 1, 0 (CrossAttnDownBlock2D x3, DownBlock2D) */
    int32_t layers_per_block;                    /* 2                                               */
    int32_t heads;                               /* 8 ("attention_head_dim": 8 = the head count)    */
    int32_t heads_per_block[4];                  /* SD 2.x: 5, 10, 20, 20 (head dim 64 at every level); all 0 = `heads` everywhere */
    int32_t prediction_type;                     /* 0 = epsilon (SD 1.x, 2.1-base), 1 = v_prediction (2.1 at 768 px)  */
    int32_t cross_attention_dim;                 /* 768                                             */
    int32_t norm_groups;                         /* 32                                              */
    float   norm_eps;                            /* 1e-5                                            */
    int32_t vae_n_blocks;                        /* 4                                               */
    int32_t vae_block_out_channels[4];           /* 128, 256, 512, 512                              */
    int32_t vae_layers_per_block;                /* 2                                               */
    int32_t latent_channels;                     /* 4                                               */
    float   vae_scaling;                         /* 0.18215                                         */
    int32_t ctx;                                 /* 77                                              */
    float   beta_start, beta_end;                /* 0.00085, 0.012 (scaled_linear)                  */
    int32_t num_train_timesteps, steps_offset;   /* 1000, 1                                         */
} tvc_sd_desc;

typedef struct { const char* name; const void* ptr; } tvc_named_tensor;

/* Register the model.  `tensors` = device pointers keyed by the diffusers state-dict names (UNet names as they are,
 * VAE names as in AutoencoderKL: "decoder....", "post_quant_conv...."), prepared by the host as follows:
 *   3x3 conv weight [Co, Ci, 3, 3]  -> bf16 [Co, 9 * Ci], column (ky * 3 + kx) * Ci + ci ("conv_in": zero padded to 64 columns)
 *   1x1 conv / linear weight        -> bf16 [Co, Ci]
 *   attn1.to_q|to_k|to_v            -> one bf16 "....attn1.to_qkv.weight" [3C, C];  attn2.to_k|to_v -> "....attn2.to_kv.weight" [2C, 768]
 *   VAE query|key|value             -> "....to_qkv.weight" bf16 [3C, C] and "....to_qkv.bias" fp32 [3C]
 *   biases, norm gains / offsets, post_quant_conv.weight [4, 4]  -> fp32
 *   every bf16 matrix must be READABLE up to the next multiple of 256 rows (zero rows appended by the host): the GEMM
 *   stages whole 256-row tiles of it even where Co (320, 640, 4 ...) is not a multiple of 256
 * With TVC_OPT_SD_PRECISION = 1 (set BEFORE this call) every tensor listed as bf16 above holds IEEE fp16 bits instead, same
 * shapes and padding; a weight beyond 65504 is +-inf in that format (never clamped) and the outputs go non-finite.
 * Referenced, not copied (the caller keeps them alive), except the resnets' time projections, which are gathered into
 * one matrix inside the handle.  Either half may be absent (UNet-only / VAE-only handles). */
int tvc_sd_load(tvc_handle* h, const tvc_sd_desc* desc, const tvc_named_tensor* tensors, int32_t n_tensors, void* stream);

/* One UNet evaluation: latents fp32 [n, 4, H, W], ctx fp32 [n, ctx, cross_attention_dim] (tvc_encode_text_hidden of
 * the CLIP ViT-L/14 text tower), scalar timestep -> predicted noise fp32 [n, 4, H, W].  H, W multiples of 8. */
int tvc_sd_unet(tvc_handle* h, const float* latents_dev, int32_t n, int32_t H, int32_t W, float timestep,
                const float* ctx_dev, float* eps_dev, void* stream);

/* AutoencoderKL.decode(latents / scaling_factor) -> images fp32 [n, 3, 8H, 8W], (x / 2 + 0.5) clamped to [0, 1]. */
int tvc_sd_vae_decode(tvc_handle* h, const float* latents_dev, int32_t n, int32_t H, int32_t W, float* images_dev, void* stream);

/* The whole sampling loop for n images: cond / uncond fp32 [n, ctx, cross_attention_dim], latents fp32 [n, 4, H, W]
 * (in: the initial noise; out: the final latents), `steps` PNDM steps (steps + 1 UNet evaluations on 2n samples each),
 * guidance scale as in the pipeline; images_dev may be NULL (latents only). */
int tvc_sd_generate(tvc_handle* h, const float* cond_dev, const float* uncond_dev, float* latents_dev, int32_t n, int32_t H,
                    int32_t W, int32_t steps, float guidance, float* images_dev, void* stream);

/* One block of the model on fp32 NCHW tensors (parity tests): kind 0 = ResnetBlock2D, 1 = Transformer2DModel, 2 = the
 * VAE AttentionBlock, 3 = 3x3 conv (stride 1), 4 = stride-2 downsample conv, 5 = nearest-2x upsample + conv;
 * `prefix` = the block's state-dict prefix with the trailing dot (conv kinds: up to and including "conv." / "conv_in.").
 * x [n, Cin, H, W]; temb fp32 [n, time_dim] (resnets of the UNet; NULL for the VAE's); ctx as tvc_sd_unet (kind 1);
 * out [n, Cout, H', W'] with H', W' = H, W; kind 4: (H + 1) / 2, (W + 1) / 2 (stride 2, padding 1: odd sizes round up);
 * kind 5: 2H, 2W.  vae != 0 uses the VAE's eps (1e-6).  Cin must be a multiple of 64 (every GEMM behind a block reads
 * whole 64-column K-tiles): any other Cin is TVC_E_INVALID for every kind, and nothing is launched. */
int tvc_sd_block(tvc_handle* h, int32_t kind, const char* prefix, const float* x_dev, int32_t n, int32_t Cin, int32_t H,
                 int32_t W, const float* temb_dev, const float* ctx_dev, int32_t Cout, int32_t vae, float* out_dev, void* stream);

/* Streaming attention of the UNet (parity tests): q [n * Tq, heads * dh], k / v [n * Tk, heads * dh], out like q; 16-bit in
 * the handle's SD format: bf16, or IEEE fp16 after TVC_OPT_SD_PRECISION = 1 (products on the f16 MFMA, fp16 probabilities and
 * outputs; an operand beyond 65504 is +-inf, never clamped, and its rows come out non-finite). */
int tvc_sd_attention(tvc_handle* h, const uint16_t* q_dev, const uint16_t* k_dev, const uint16_t* v_dev, uint16_t* out_dev,
                     int32_t n, int32_t heads, int32_t Tq, int32_t Tk, int32_t dh, void* stream);
/* The same with one row stride (in elements) per operand, as the model's fused projections pass them: head h of a row
 * occupies its columns [h * dh, (h + 1) * dh), columns beyond heads * dh are neither read nor written.  ldq / ldk / ldv
 * multiples of 8, ldo a multiple of 4, each >= heads * dh, q / k / v 16-byte and out 8-byte aligned; anything else
 * returns TVC_E_INVALID and launches nothing.  The operands are in the handle's SD format, as for tvc_sd_attention. */
int tvc_sd_attention_ex(tvc_handle* h, const uint16_t* q_dev, int64_t ldq, const uint16_t* k_dev, int64_t ldk,
                        const uint16_t* v_dev, int64_t ldv, uint16_t* out_dev, int64_t ldo, int32_t n, int32_t heads,
                        int32_t Tq, int32_t Tk, int32_t dh, void* stream);

/* One row kernel of the generator on the caller's device buffers (parity tests): everything between its GEMMs.  Each op is
 * exactly ONE kernel launcher, with no copy and no relayout in between; no model needs to be loaded; the 16-bit format
 * ("16" below) is the handle's SD format, as for tvc_sd_attention.  Layouts: "tokens" = [n * H * W, C] rows (NHWC, dense);
 * "padded" = every image an (H + 2) x (W + 2) grid of rows, pixel (y, x) at row (y + 1) * (W + 2) + (x + 1), whose border
 * rows a convolution reads as its zero padding (a padded OUTPUT has its borders written as zeros, the borders of a padded
 * INPUT are never read).  Slots of tvc_sd_op_args per op (unused slots are ignored; flags are 0 / 1):
 *   GROUPNORM        in0 x 16, in1 tadd fp32 [n, ld_t] or NULL (x + tadd[img, c] is what is normalised), in2 gamma, in3 beta
 *                    fp32 [C]; out0 y 16; i = n, H, W, C, groups, silu, in_pad, out_pad, ld_t; f0 = eps.  C % 8 == 0,
 *                    C <= 4096, groups <= 32, C % groups == 0.  Its statistics scratch is the handle's.
 *   LAYERNORM        in0 x 16 [rows, C], in1 g, in2 b fp32 [C], in3 add 16 or NULL; out0 y, out1 sum_out 16 (given exactly
 *                    when add is: sum_out = x + add, y = LayerNorm(sum_out)); i = rows (0 is allowed: nothing is written),
 *                    C; f0 = eps.  C % 8 == 0, C <= 1536.
 *   GEGLU            in0 16 [rows, 2 * Ch] (value | gate); out0 16 [rows, Ch] = value * gelu_erf(gate); i = rows, Ch (% 8).
 *   ADD              in0, in1 16 [n]; out0 16 = in0 + in1; i = n (% 8).
 *   ADD_PADDED       in0 16 tokens, in1 16 padded; out0 16 tokens; i = n, H, W, C (% 8).
 *   RELAYOUT         in0 16; out0 16; i = n, H, W (the OUTPUT's extent), C (% 8), in_pad, out_pad, up (the input is
 *                    (H / 2) x (W / 2), nearest-2x upsampled; H, W even).
 *   IM2COL3X3        in0 16 tokens [n, Hi, Wi, C]; out0 16 [n * Ho * Wo, 9 * C], column (ky * 3 + kx) * C + c, padding 1,
 *                    Ho = (Hs - 1) / stride + 1 with Hs = Hi (2 * Hi with up); i = n, Hi, Wi, C (% 8), stride (1, 2), up (stride 1).
 *   IM2COL_IN        in0 fp32 NCHW [n, Cin, H, W]; out0 16 [n * H * W, Kp], column tap * Cin + ci of in0 * scale, zeros from
 *                    column 9 * Cin on; i = n, Cin, H, W, Kp (>= 9 * Cin); f0 = scale.
 *   CONCAT           in0 16 [tokens, Ca], in1 16 [tokens, Cb]; out0 16 [tokens, Ca + Cb]; i = Ca, Cb (% 8), tokens.
 *   CAST_SILU        in0 fp32 [n]; out0 16 [n]; i = n, silu.
 *   TOKENS_TO_NCHW   in0 fp32 rows of pitch ld (first C columns; dense, or padded with in_pad); out0 fp32 NCHW
 *                    = in0 * mul + add, clamped to [0, 1] with clamp; i = n, C, H, W, ld, clamp, in_pad; f0 = mul, f1 = add.
 *   POINTWISE_SMALL  in0 fp32 NCHW [n, C, HW], in1 w fp32 [C, C], in2 bias fp32 [C]; out0 fp32 NCHW
 *                    = bias[c] + sum_ci w[c, ci] * (in0[n, ci, p] * in_scale); i = n, C (<= 8), HW; f0 = in_scale.
 *   CFG              in0 fp32 [2 * n] (unconditional | conditional); out0 fp32 [n] = eu + g * (ec - eu); i = n; f0 = g.
 *   LINCOMB          in0 sample fp32 [n], in1 .. in4 e0 .. e3 fp32 [n] (e1 .. e3 may be NULL); out0 fp32 [n] (may be in0)
 *                    = cs * sample - ce * (c0 e0 + c1 e1 + c2 e2 + c3 e3); i = n; f = cs, ce, c0, c1, c2, c3.
 *   SOFTMAX_ROWS     in0 fp32 [rows, T]; out0 16 [rows, T] = softmax(in0 * scale) per row; i = rows, T; f0 = scale (> 0).
 *   NCHW_TO_TOKENS   in0 fp32 NCHW [n, C, HW]; out0 16 tokens; i = n, C, HW.
 *   TOKENS16_TO_NCHW in0 16 tokens; out0 fp32 NCHW; i = n, C, HW.
 *   TIMESTEP_EMBED   out0 16 [n, dim] = [cos | sin](t * 10000^(-j / (dim / 2))), every row the same; i = n, dim (even); f0 = t.
 *   TRANSPOSE        in0 16 [R, C]; out0 16 [C, R]; i = R, C.
 * A NULL args or required pointer, a pointer the kernel's vector accesses need aligned (16 bytes for 16-bit tensors read or
 * written in pieces of 8, 4 for fp32) and is not, an extent that is not positive, extents whose product leaves int32, an
 * unknown op: TVC_E_INVALID; an argument the launcher rejects: TVC_E_HIP.  Either way
 * nothing is launched. */
enum { TVC_SD_OP_GROUPNORM = 0, TVC_SD_OP_LAYERNORM = 1, TVC_SD_OP_GEGLU = 2, TVC_SD_OP_ADD = 3, TVC_SD_OP_ADD_PADDED = 4,
       TVC_SD_OP_RELAYOUT = 5, TVC_SD_OP_IM2COL3X3 = 6, TVC_SD_OP_IM2COL_IN = 7, TVC_SD_OP_CONCAT = 8, TVC_SD_OP_CAST_SILU = 9,
       TVC_SD_OP_TOKENS_TO_NCHW = 10, TVC_SD_OP_POINTWISE_SMALL = 11, TVC_SD_OP_CFG = 12, TVC_SD_OP_LINCOMB = 13,
       TVC_SD_OP_SOFTMAX_ROWS = 14, TVC_SD_OP_NCHW_TO_TOKENS = 15, TVC_SD_OP_TOKENS16_TO_NCHW = 16,
       TVC_SD_OP_TIMESTEP_EMBED = 17, TVC_SD_OP_TRANSPOSE = 18, TVC_SD_OP_COUNT = 19 };
typedef struct { const void* in[6]; void* out[2]; int64_t i[12]; float f[12]; } tvc_sd_op_args;
int tvc_sd_op(tvc_handle* h, int32_t op, const tvc_sd_op_args* a, void* stream);

/* One row kernel of the CLIP towers on the caller's device buffers (parity tests): the LayerNorm family forward and
 * backward, the stem's gathers, the activations, the split-mode plane kernels, the row gathers and the text length / embedding
 * kernels.  Each op is exactly ONE kernel launcher, with no copy in between; no weights are needed and no handle state is
 * read.  "16" = a 16-bit tensor: bf16, or IEEE fp16 where the op has an f16 flag and it is 1.  Strides are in elements.
 * Slots of tvc_tower_op_args per op (unused slots are ignored; flags are 0 / 1; "or NULL" marks the optional pointers):
 *   LAYERNORM        in0 x fp32 (row r at in0 + src(r) * x_row_stride, src(r) = row_idx[r], or r without row_idx; WRITTEN
 *                    with write_x and a delta), in1 row_idx int32 [rows] or NULL, in2 delta, in3 delta2 16 or NULL (row r at
 *                    src(r) * x_row_stride -- x's layout --, or at r * d with delta_compact), in4 g, in5 b fp32 [d];
 *                    out0 y 16 [rows, d] or NULL, out1 y32 fp32 [rows, d] or NULL (one of the two is required; y is the
 *                    rounding of y32), out2 xsum fp32 [rows, d] or NULL = (x + delta) + delta2 in fp32, which is also what
 *                    write_x stores to x and what is normalised; i = rows, d, x_row_stride (>= d, % 4), write_x,
 *                    delta_compact, f16.  d % 4 == 0, d <= 1024.
 *   LAYERNORM_BWD    in0 x fp32 (row r at r * x_row_stride), in1 delta bf16 or NULL (row r at r * x_row_stride: x's layout),
 *                    in2 dy [rows, d] dense, bf16 or fp32 with dy_fp32, in3 gamma fp32 [d], in4 dres fp32 or NULL (row r at
 *                    r * out_row_stride; may be out0: in place); out0 dx fp32, out1 dx16 bf16 or NULL = bf16(dx) (rows at
 *                    r * out_row_stride both; elements between the rows are not written);
 *                    dx = rstd * (g - mean(g) - xhat * mean(g * xhat)) + dres with g = dy * gamma and xhat of x + delta;
 *                    i = rows, d, x_row_stride, out_row_stride (>= d, % 4), dy_fp32.  d % 4 == 0, d <= 1024.
 *   LNPRE_BWD        in0 patch_out fp32 [B * (T - 1), d], in1 pos fp32 [T, d], in2 gamma fp32 [d], in3 dy fp32 [B * T, d] (its
 *                    class rows t = 0 are not read); out0 bf16 [B * (T - 1), d] = LayerNorm backward at patch_out + pos[t];
 *                    i = B, T (>= 2), d.
 *   ASSEMBLE_LNPRE   in0 patch_out fp32 [B * (T - 1), d] (NULL allowed with T = 1), in1 cls fp32 [d], in2 pos fp32 [T, d], in3 g,
 *                    in4 b fp32 [d]; out0 x fp32 [B * T, d] = LayerNorm((t == 0 ? cls : patch_out[b, t - 1]) + pos[t]); i = B, T, d.
 *   IM2COL           in0 pix fp32 [B, 3, image, image]; out0 16 [B * P, Kp], P = (image / patch)^2, column (c, ky, kx), zeros
 *                    from column 3 * patch^2 on; i = B, image, patch, Kp (>= 3 * patch^2, % 8), f16.  in0 16-byte aligned
 *                    when image % 4 == 0.
 *   IM2COL_F32       in0 pix fp32; out0 fp32 [B * P, 3 * patch^2]; i = B, image, patch.
 *   COL2IM           in0 dcols fp32 [B * P, Kp] (columns from 3 * patch^2 on are not read); out0 dpix fp32 [B, 3, S, S];
 *                    i = B, S, patch, Kp.
 *   GELU_FWD         in0 u bf16 [n]; out0 bf16 [n] = u * sigmoid(1.702 u) (fast exponential and reciprocal); i = n (% 8).
 *   GELU_BWD         in0 u bf16 [n]; out0 dm bf16 [n], in place: dm *= s + 1.702 u s (1 - s), s = sigmoid(1.702 u); i = n (% 8).
 *   GELU_ERF_16      out0 x 16 [n], in place: 0.5 x (1 + erf(x / sqrt 2)); i = n (% 8), f16.
 *   GELU_ERF_F32     out0 x fp32 [n], in place; i = n (% 4).
 *   L2NORM_ROWS      out0 x fp32 [rows, d], in place: x / |x| (no epsilon); i = rows, d.
 *   L2NORM_BWD       in0 x fp32 [rows, d] (not read, may be NULL, with normalize 0), in1 dy fp32 [rows, d]; out0 bf16 [rows, d]
 *                    = (dy - y (y . dy)) / |x| with y = x / |x|, or bf16(dy) with normalize 0; i = rows, d, normalize.
 *   LN_SPLIT         in0 x fp32, in1 row_idx, in4 g, in5 b as LAYERNORM; in2 d1, in3 d2 fp32 or NULL (always x's layout);
 *                    out0 planes bf16 [rows, 2 * d] or NULL (hi = bf16(y32) | lo = bf16(y32 - hi)), out1 y32 fp32 [rows, d] or
 *                    NULL (one of the two is required); i = rows, d, x_row_stride, write_x.
 *   ROWS_SPLIT       in0 x fp32 [rows, ld_in]; out0 bf16 [rows, 2 * Kp]: hi | lo planes of act(x[:, :K]), zeros in columns
 *                    K .. Kp of both; i = rows, K, Kp (>= K; both % 4), ld_in (>= K, % 4), gelu (0 none, 1 QuickGELU with expf and
 *                    an IEEE division, 2 erf GELU).
 *   SPLIT_PLANES     in0 x fp32 [rows, d]; out0 bf16 [rows, planes * d]; i = rows, d (% 4), planes (1: hi only, 2).
 *   GATHER_ROWS      in0 bank bf16 [R, ld], in1 idx int32 [n]; out0 fp32 [n, D] = bank[idx - idx_offset, :D] (+ [D : 2 D] with
 *                    planes 2), zeros where idx < 0 or idx - idx_offset is outside [0, R); i = n, D, R, ld (>= planes * D),
 *                    planes (1, 2), idx_offset (>= 0).
 *   GATHER_F32_ROWS  in0 x fp32 rows of pitch ld, in1 idx int32 [n] or NULL; out0 fp32 [n, d] = x[idx[r]] or, without idx,
 *                    x[r * idx_mul]; i = n, d (% 4), ld (>= d, % 4), idx_mul (>= 0).
 *   TEXT_LENS_SCAN   in0 tok int32 [n_text, ctx]; out0 starts int32 [n_text + 2], out1 pfx int32 [2 * n_text] or NULL, out2
 *                    scratch int32 [n_text] (required without pfx); len = position of the first maximum id + 1; with pfx
 *                    (groups of G consecutive texts, the first is the base) pfx[n] = min(first mismatch with the base, len,
 *                    the base's len), 0 for a base, and pfx[n_text + n] = starts[base]; starts = exclusive scan of len - pfx,
 *                    starts[n_text] = total, starts[n_text + 1] = the largest len; i = n_text, ctx, G (>= 2 with pfx).
 *   TEXT_EMBED       in0 tok int32 [n_text, ctx], in1 tok_emb fp32 [vocab, d], in2 pos fp32 [ctx, d], in3 starts or NULL, in4 pfx
 *                    or NULL (needs starts), both as TEXT_LENS_SCAN writes them; out0 x fp32 rows of d = tok_emb[clamp(id, 0,
 *                    vocab - 1)] + pos[t] at row n * ctx + t (dense) or starts[n] + t - pfx[n] for the text's own positions
 *                    (packed; other rows are not written), out1 eot_row int32 [n_text] = the row of the first maximum id
 *                    (a text with no own rows: its base's row pfx[n_text + n] + pfx[n] - 1); i = n_text, ctx, d (% 4), vocab.
 * A NULL args or required pointer; a pointer or a row stride that is not aligned for the kernel's vector accesses (16 bytes
 * for fp32 rows read or written as 4-vectors and for 16-bit tensors in pieces of 8, 8 bytes for 16-bit rows in pieces of 4,
 * the element size for the scalar kernels: the im2col / col2im fp32 forms, the L2 kernels, GATHER_ROWS, the text kernels' int32);
 * a stride below the row's width; an extent that is not positive; extents whose product leaves int32; image % patch != 0; a flag
 * that is neither 0 nor 1; planes or gelu outside the values listed; an unknown op: TVC_E_INVALID.  What a launcher rejects
 * (d % 4, d > 1024, n % 8, Kp < K, G < 2 with pfx): TVC_E_HIP.  Either way nothing is launched. */
enum { TVC_TOWER_OP_LAYERNORM = 0, TVC_TOWER_OP_LAYERNORM_BWD = 1, TVC_TOWER_OP_LNPRE_BWD = 2, TVC_TOWER_OP_ASSEMBLE_LNPRE = 3,
       TVC_TOWER_OP_IM2COL = 4, TVC_TOWER_OP_IM2COL_F32 = 5, TVC_TOWER_OP_COL2IM = 6, TVC_TOWER_OP_GELU_FWD = 7,
       TVC_TOWER_OP_GELU_BWD = 8, TVC_TOWER_OP_GELU_ERF_16 = 9, TVC_TOWER_OP_GELU_ERF_F32 = 10, TVC_TOWER_OP_L2NORM_ROWS = 11,
       TVC_TOWER_OP_L2NORM_BWD = 12, TVC_TOWER_OP_LN_SPLIT = 13, TVC_TOWER_OP_ROWS_SPLIT = 14, TVC_TOWER_OP_SPLIT_PLANES = 15,
       TVC_TOWER_OP_GATHER_ROWS = 16, TVC_TOWER_OP_GATHER_F32_ROWS = 17, TVC_TOWER_OP_TEXT_LENS_SCAN = 18,
       TVC_TOWER_OP_TEXT_EMBED = 19, TVC_TOWER_OP_COUNT = 20 };
/* as tvc_sd_op_args with four output slots: LAYERNORM has three outputs */
typedef struct { const void* in[6]; void* out[4]; int64_t i[12]; float f[12]; } tvc_tower_op_args;
int tvc_tower_op(tvc_handle* h, int32_t op, const tvc_tower_op_args* a, void* stream);

/* Image preprocessing on the device: images fp32 [n, 3, H, W] with values in [0, 1] -> out fp32 [n, 3, S, S]:
 * antialiased resize of the short side to S (filter 0 = bilinear: torchvision Resize as in
 * experiments/defenses/generative_ref.py:55-59 -- which resizes BOTH sides to S; 1 = bicubic: the CLIP preprocess of
 * src/attacks/hubness_attack.py:223), centre crop, (x - mean[c]) / std[c].  keep_aspect 0 resizes both sides to S.
 * The size rule (the contract; CLIPModel.preprocess follows it): the short side becomes S, the long side
 * floor(long * S / short + 1/2) -- a half rounds up: 449 x 448 -> 225 x 224 -- and never less than S; the crop starts at
 * (resized - S) / 2, rounded down.  The filter: scale = in / resized per axis, f = max(scale, 1), support (bilinear 1,
 * bicubic 2 with a = -0.5) * f around the centre (o + 0.5) * scale, tap argument (i + 0.5 - centre) / f, the taps clipped to
 * the image and normalised per output pixel, on float pixels (no uint8 rounding). */
int tvc_preprocess_images(tvc_handle* h, const float* images_dev, int32_t n, int32_t H, int32_t W, int32_t S, int32_t filter,
                          int32_t keep_aspect, const float* mean3, const float* std3, float* out_dev, void* stream);

/* Building blocks of the fp32-grade tower mode (TVC_OPT_TOWER_PRECISION = 1), exported for parity tests:
 * out[j, i] (op)= sum_k x[j, k] * w[i, k] + bias[i] on the exact-f32 matrix instruction; w fp32 [I, K], x fp32 [J, K],
 * out fp32 [J, ld_out]; K % 4 == 0; epilogue 0 = store, 1 = QuickGELU, 2 = out += (residual add). */
int tvc_gemm_f32(tvc_handle* h, const float* w_dev, const float* x_dev, const float* bias_dev, float* out_dev,
                 int32_t I, int32_t J, int32_t K, int32_t ld_out, int32_t epilogue, void* stream);
/* fp32 multi-head attention, head_dim 64, seq_len <= 288: qkv fp32 [n_seq * seq_len, 3 * width], out fp32 [rows, width]. */
int tvc_attention_f32(tvc_handle* h, const float* qkv_dev, float* out_dev, int32_t n_seq, int32_t seq_len,
                      int32_t heads, int32_t causal, void* stream);

/* Building blocks of the split-bf16 tower mode (TVC_OPT_TOWER_PRECISION = 2), exported for parity tests:
 * tvc_gemm_split: out fp32 [J, ld_out] = x [J, K] w[I, K]^T + bias with both operands split into hi | lo bf16 planes and
 * three MFMA products per element (K % 4 == 0).
 * tvc_attention_split: qkv fp32 [rows, 3 * width] (head_dim 64, seq_len <= 272; starts_dev int32 [n_seq + 1] = packed
 * sequences of at most seq_len rows, or NULL = n_seq x seq_len dense rows) -> the attention output as hi | lo bf16 planes
 * [rows, 2 * width] (value = hi + lo); seq_len <= 272. */
int tvc_gemm_split(tvc_handle* h, const float* w_dev, const float* x_dev, const float* bias_dev, float* out_dev,
                   int32_t I, int32_t J, int32_t K, int32_t ld_out, void* stream);
int tvc_attention_split(tvc_handle* h, const float* qkv_dev, uint16_t* out_planes_dev, const int32_t* starts_dev,
                        int32_t n_seq, int32_t seq_len, int32_t heads, int32_t causal, void* stream);
/* tvc_attention_split plus prefix sharing: pfx_dev (optional, causal packed rows only), int32 [2 * n_seq], as in
 * tvc_attention_ex -- pfx[s] is the prefix length, pfx[n_seq + s] the packed row of the prefix's position 0, and seq_len
 * (<= 272) bounds prefix + own rows.  pfx without starts or without causal returns TVC_E_INVALID and launches nothing. */
int tvc_attention_split_ex(tvc_handle* h, const float* qkv_dev, uint16_t* out_planes_dev, const int32_t* starts_dev,
                           const int32_t* pfx_dev, int32_t n_seq, int32_t seq_len, int32_t heads, int32_t causal,
                           void* stream);

/* Building blocks of the split-bf16 input gradient (TVC_OPT_GRAD_PRECISION = 2), exported for parity tests.
 * tvc_attention_split_backward: the attention backward on fp32 operands.  qkv fp32 [n_seq * seq_len, 3 * width] (q | k | v, head_dim 64), dout fp32 [rows, width] =
 * d(loss)/d(attention output) -> dqkv fp32 [rows, 3 * width].  Non-causal dense sequences, 1 <= seq_len <= 288.  Scores
 * and probabilities are recomputed from qkv; every product (S, dP, dQ, dK, dV) is three bf16 MFMAs on hi | lo operands,
 * the softmax and the row sums are fp32.  Buffers 16-byte aligned.  Deterministic. */
int tvc_attention_split_backward(tvc_handle* h, const float* qkv_dev, const float* dout_dev, float* dqkv_dev, int32_t n_seq,
                                 int32_t seq_len, int32_t heads, void* stream);
/* One fp32 row kernel of the split-bf16 input gradient on the caller's device buffers (parity tests), under tvc_tower_op's
 * rules: one launcher per op, no weights, no handle state, the slots of tvc_tower_op_args, the same refusals (TVC_E_INVALID
 * for a NULL / misaligned pointer, a bad stride, extent or flag and an unknown op; TVC_E_HIP for what a launcher rejects).
 *   GELU_BWD       in0 u fp32 [n]; out0 dm fp32 [n], in place: dm *= s + 1.702 u s (1 - s), s = 1 / (1 + exp(-1.702 u)) (expf and
 *                  an IEEE division); i = n (% 4).
 *   L2NORM_BWD     in0 x fp32 [rows, d] (not read, may be NULL, with normalize 0), in1 dy fp32 [rows, d]; out0 fp32 [rows, d]
 *                  = (dy - y (y . dy)) / |x| with y = x / |x|, or dy with normalize 0; i = rows, d, normalize.
 *   LNPRE_BWD      in0 patch_out fp32 [B * (T - 1), d], in1 pos fp32 [T, d], in2 gamma fp32 [d], in3 dy fp32 [B * T, d] (its
 *                  class rows are not read); out0 fp32 [B * (T - 1), d] = LayerNorm backward at patch_out + pos[t]; i = B, T (>= 2), d.
 *   ROWS_SPLIT_T   in0 w fp32 [I, ld]; out0 bf16 [K, 2 * Ip]: row k = hi | lo planes of w[0 .. I - 1][k] (the planes of w^T);
 *                  columns I .. Ip of both planes are NOT written (the caller zeroes the padding); i = I, K, Ip (>= I), ld (>= K).
 *   LAYERNORM_BWD  in0 x fp32 (row r at r * x_row_stride), in1 delta fp32 or NULL (x's layout), in2 dy fp32 [rows, d] dense,
 *                  in3 gamma fp32 [d], in4 dres fp32 or NULL (row r at r * out_row_stride; may be out0: in place); out0 dx fp32
 *                  = rstd * (g - mean(g) - xhat * mean(g * xhat)) + dres, g = dy * gamma, xhat of x + delta;
 *                  i = rows, d, x_row_stride, out_row_stride (>= d, % 4).  d % 4 == 0, d <= 1024. */
enum { TVC_GRAD_SPLIT_OP_GELU_BWD = 0, TVC_GRAD_SPLIT_OP_L2NORM_BWD = 1, TVC_GRAD_SPLIT_OP_LNPRE_BWD = 2,
       TVC_GRAD_SPLIT_OP_ROWS_SPLIT_T = 3, TVC_GRAD_SPLIT_OP_LAYERNORM_BWD = 4, TVC_GRAD_SPLIT_OP_COUNT = 5 };
int tvc_grad_split_op(tvc_handle* h, int32_t op, const tvc_tower_op_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TVC_H_ */
