/* lightglue_amd — C ABI of the MI355X-native LightGlue matcher forward path.
 *
 * The reference (cvg/LightGlue) has no FFI / plugin boundary: its matcher is the Python class
 * `lightglue.LightGlue` (lightglue/lightglue.py:321, exported at lightglue/__init__.py:4).  This
 * header is the boundary a binding of that class's hot path would sit on: one opaque engine that
 * replaces `LightGlue.__init__` weight handling (lightglue.py:376-437) and `LightGlue._forward`
 * (lightglue.py:483-629).  Plain pointers and sizes only; every data pointer is a DEVICE pointer
 * owned by the caller unless stated otherwise; kernels are enqueued on the caller's HIP stream.
 * Python binding: lightglue_amd/_cabi.py (ctypes).  See INTEGRATION.md.
 */
#ifndef LIGHTGLUE_AMD_H
#define LIGHTGLUE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Operand precision of the matrix-core contractions (accumulation is always fp32). */
enum {
    LG_PREC_F32 = 0,    /* v_mfma_f32_16x16x4_f32: exact fp32 products (parity anchor)                              */
    LG_PREC_BF16 = 1,   /* v_mfma_f32_16x16x32_bf16, one MFMA per product: fast, does NOT hold the 1e-3 score bar    */
    LG_PREC_F16 = 2,    /* v_mfma_f32_16x16x32_f16, one MFMA per product: fast, does NOT hold the 1e-3 score bar     */
    /* 3 was split-bf16 (rounds 1-2): same cost as LG_PREC_F16X3 at 3x its score error — removed in round 3            */
    LG_PREC_F16X3 = 4   /* DEFAULT.  split f16: x = hi + lo (both f16, 22 bits), 3 MFMAs per product, for every linear
                           layer, the similarity matrix AND — with attn_precision = LG_PREC_F16X3, the default — for q k^T
                           and P V of the attention (q / k / v and the probabilities kept as hi + lo planes).  Holds the
                           bar also when attention logits are sharp (recipe-D fixtures).  Needs |x| < 65504, like the
                           reference's own fp16 mode.  attn_precision = LG_PREC_F16 is the fast opt-in: q / k / v as ONE f16
                           plane (what the reference's GPU path feeds its fp16 SDPA, lightglue.py:119), 2 MFMAs per
                           product in the q/k/v projections — within the bar only while attention is diffuse            */
};

#define LG_OK 0
#define LG_ERR_INVALID 1   /* bad argument (the Python shim raises AssertionError/ValueError)      */
#define LG_ERR_HIP 2       /* a HIP runtime call failed; see lg_last_error()                       */
#define LG_ERR_STATE 3     /* call order violated (e.g. forward before weights were finalised)     */
/* per-pair codes of lg_forward_io.status (device array; the call itself returned LG_OK): */
#define LG_ERR_RANGE 4     /* LG_FLAG_CHECK_FINITE: a value of this pair's residual stream or of its q / k / v left the f16 operand range
                              (|x| >= 65504, inf or NaN: the input domain of LG_PREC_F16X3 / _F16 / _BF16); its scores are not to be trusted */
#define LG_ERR_DEVICE 5    /* an internal device-side wait expired (adaptive compaction): results of this forward are invalid */
#define LG_ERR_INDEX 6     /* LG_FLAG_INDEXED: index0[b] or index1[b] of this pair lies outside [0, images): nothing was read through it and the pair came
                              back as an empty pair (stop 1, matches -1, scores 0).  Reported before LG_ERR_RANGE; LG_ERR_DEVICE stays on top */

/* Envelope of one lg_engine_forward / lg_engine_reserve call (round 6).  Inside it every index of every kernel fits the integer type it is
 * computed in, and the largest shapes are covered by GPU tests (N = M = 8192, B = 1; N = M = 4096, B = 32); a call outside it returns
 * LG_ERR_INVALID with a message instead of writing past 32-bit offsets.  Split larger batches across calls (pairs are independent).
 *   keypoints per image                  n0, n1 <= LG_MAX_KEYPOINTS
 *   rows of one forward                  B * (cap0 + cap1) <= LG_MAX_ROWS          (cap = n rounded up to 128; X is then <= 2 GiB)
 *   similarity-matrix elements           B * cap0 * cap1  <= LG_MAX_SIM_ELEMS
 * Input domain of the score bar (|d score| <= 1e-3 against the fp32 reference, LG_PREC_F16X3): descriptors of norm <= ~30 (unit-norm extractor
 * output times up to 10 x the recipes' norm spread of [0.5, 3]); beyond that the network's own fp32 evaluation differs by more than the bar
 * (DESIGN.md section 1).  Values that leave the f16 operand range are reported per pair as LG_ERR_RANGE when LG_FLAG_CHECK_FINITE is set. */
#define LG_WIRE_WIDTH(n0, n1) (3LL * (n0) + 3LL * (n1) + 2)   /* elements of one lg_forward_io.wire row */
#define LG_MAX_KEYPOINTS 8192
#define LG_MAX_ROWS 2097152            /* 2^21 */
#define LG_MAX_SIM_ELEMS 2147483647LL  /* 2^31 - 1 */

/* Mirrors LightGlue.default_conf (lightglue.py:322-335) for the keys the forward path reads. */
typedef struct lg_config {
    int32_t input_dim;          /* 256 SuperPoint, 128 DISK/ALIKED/SIFT (lightglue.py:351-374)   */
    int32_t descriptor_dim;     /* must be 256                                                    */
    int32_t n_layers;           /* 9                                                              */
    int32_t num_heads;          /* must be 4 (head_dim 64)                                        */
    int32_t add_scale_ori;      /* 0/1: 4-D positional input (lightglue.py:495-501)               */
    double depth_confidence;    /* early stop, <= 0 disables (lightglue.py:528)                   */
    double width_confidence;    /* point pruning, <= 0 disables (lightglue.py:529)                */
    double filter_threshold;    /* lightglue.py:592                                               */
    int32_t pruning_min_kpts;   /* resolved LightGlue.pruning_min_kpts() (lightglue.py:658-662)   */
    int32_t precision;          /* LG_PREC_*                                                      */
    int32_t attn_precision;     /* -1 = `precision`; or LG_PREC_F16 together with LG_PREC_F16X3   */
} lg_config;

typedef struct lg_engine lg_engine;

/* Everything one forward reads and writes.  Inputs are dense [B][n][..] fp32, exactly the tensors of
 * the reference's input dict (lightglue.py:460-468); outputs are the fixed-shape tensors of its output
 * dict (lightglue.py:619-629) in int32 (the Python shim widens to int64) plus a device-built compact
 * match list replacing the per-pair torch.where loop (lightglue.py:593-602). */
#define LG_FLAG_NO_PRUNING 1u /* skip point pruning for this call: the reference's padded/compiled
                                 path does the same (lightglue.py:529 `and not do_compile`)        */
#define LG_FLAG_EXT 2u        /* the caller's struct carries the round-5 extension fields (everything after `log_assignment`); without
                                 the flag the engine never reads them (callers built against the round-4 header keep working)          */
#define LG_FLAG_CHECK_FINITE 4u /* range guard (needs LG_FLAG_EXT and `status`): every fused tail and q/k/v projection also tests the
                                 values it is about to split into f16 planes — one compare per value — and flags the pair           */

#define LG_FLAG_INDEXED 8u    /* the inputs are feature STORES and `index0` / `index1` (the last fields of the struct) say which image of them each pair
                                 reads: see there.  Needs LG_FLAG_EXT and `status`                                      */

/* Descriptors STORED as IEEE binary16 (the format hloc and most SfM tooling write feature files in): with a flag set, desc0 / desc1 point to binary16 rows
 * [B or images][n][input_dim] instead of fp32 ones, read in place and widened exactly (every binary16 value, subnormals included) where the descriptors enter the
 * engine — the forward is bit-identical to one on the same values converted to fp32 by the caller, in every mode (LG_FLAG_INDEXED, ragged num0 / num1,
 * LG_FLAG_CHECK_FINITE, every precision).  Per side: a pair list may join an f16 store and an fp32 one.  Each flag needs LG_FLAG_EXT, and its pointer must be
 * 16-byte aligned; otherwise the call returns LG_ERR_INVALID before the GPU is touched.  Rounding descriptors to binary16 is the CALLER's choice of storage format,
 * not a precision mode of the engine: the 1e-3 score bar is stated for fp32 descriptors only (README: measured drift of f16-stored descriptors). */
#define LG_FLAG_DESC0_F16 16u
#define LG_FLAG_DESC1_F16 32u

/* SIFT feature stores as COLMAP / pycolmap / OpenCV write them: uint8 descriptors, and the RootSIFT transform the SIFT LightGlue weights expect.  Per side, like
 * the binary16 flags, and composing with everything they compose with (LG_FLAG_INDEXED, ragged num0 / num1, LG_FLAG_CHECK_FINITE, every precision; a pair list may
 * join a uint8 store with an fp32 or binary16 one).
 *   LG_FLAG_DESC0_U8 / _DESC1_U8: desc0 / desc1 point to uint8 rows [B or images][n][input_dim], read in place and widened exactly (0 .. 255 -> fp32): the forward
 *     is bit-identical to one on the same values converted to fp32 by the caller.
 *   LG_FLAG_ROOTSIFT0 / _ROOTSIFT1: after widening from its storage type (fp32, binary16 or uint8) every row is replaced by its RootSIFT before anything else reads
 *     it — r = x / max(sum |x|, 1e-6); r = sqrt(max(r, 1e-6)); r / max(|r|_2, 1e-6), in fp32 (the reference's sift_to_rootsift, sift.py:53-56) — bit-identical to
 *     a forward on the fp32 rows lg_rootsift() writes.
 * LG_ERR_INVALID with a message, before the GPU is touched: any of the four without LG_FLAG_EXT; _U8 and _F16 on one side; a uint8 pointer that is not 16-byte
 * aligned; input_dim % 4 != 0; RootSIFT with input_dim > 256.  With input_dim == 256 such a call prepares the keypoints in a launch of its own instead of inside the
 * first projection (same bits).  Quantising descriptors to uint8 is the CALLER's storage format, outside the 1e-3 score bar like binary16. */
#define LG_FLAG_DESC0_U8 64u
#define LG_FLAG_DESC1_U8 128u
#define LG_FLAG_ROOTSIFT0 256u
#define LG_FLAG_ROOTSIFT1 512u
#define LG_SIFT_STORE_FLAGS (LG_FLAG_DESC0_U8 | LG_FLAG_DESC1_U8 | LG_FLAG_ROOTSIFT0 | LG_FLAG_ROOTSIFT1)

typedef struct lg_forward_io {
    int32_t batch, n0, n1;
    uint32_t flags;                        /* LG_FLAG_*                                           */
    const float *kpts0, *kpts1;            /* [B][n][2] pixel (x, y)                              */
    const float *desc0, *desc1;            /* [B][n][input_dim]; binary16 / uint8 rows behind the same pointer with LG_FLAG_DESC0_F16 / _DESC1_F16 / LG_FLAG_DESC0_U8 / _DESC1_U8 */
    const float *size0, *size1;            /* [B][2] (w, h) or NULL -> bounding-box normalisation */
    const float *scales0, *oris0, *scales1, *oris1; /* [B][n] iff add_scale_ori, else NULL        */
    int32_t *matches0, *matches1;          /* [B][n0], [B][n1]; -1 = unmatched                    */
    float *scores0, *scores1;              /* [B][n0], [B][n1]                                    */
    int32_t *stop;                         /* [B] number of layers executed per pair              */
    int32_t *prune0, *prune1;              /* [B][n] layer counters; required iff pruning enabled */
    int32_t *matches;                      /* [B][min(n0,n1)][2] sorted by index0                 */
    float *match_scores;                   /* [B][min(n0,n1)]                                     */
    int32_t *n_matches;                    /* [B]                                                 */
    /* Ragged batches (replaces the reference's pad_to_length ones-padding + masks,
     * lightglue.py:46-55, :512-520): optional per-pair keypoint counts, num0[b] <= n0, num1[b] <= n1.
     * Rows >= num of the dense inputs are never read; their outputs are -1 / 0 (prune counters 0).
     * Each pair behaves exactly as a separate B=1 call on its first num rows.  NULL = all rows live. */
    const int32_t *num0, *num1;            /* [B] or NULL (LG_FLAG_INDEXED: [images])             */
    /* Optional side output: the full log-assignment matrix of
     * sigmoid_log_double_softmax (lightglue.py:265-277) INCLUDING the dustbin row / column, in ORIGINAL
     * keypoint index space: [B][n0+1][n1+1] fp32.  Rows / columns of keypoints that were pruned (or are
     * padding of a ragged batch) hold -inf; the corner is 0 as in the reference.  NULL = not produced
     * (the match outputs never need the matrix materialised). */
    float *log_assignment;
    /* ---- round-5 extension: read only when flags & LG_FLAG_EXT; every pointer optional (NULL = not produced) ----
     * The reference's output dict holds int64 indices and, without pruning, float `prune0/1` (lightglue.py:616-629); the fields
     * below let the engine write those dtypes itself (one kernel at the end of the forward) instead of the caller widening /
     * filling them with framework kernels.  The int32 outputs above stay required: they are what the engine computes in. */
    int64_t *matches0_i64, *matches1_i64;  /* [B][n0], [B][n1]                                                        */
    int64_t *matches_i64;                  /* [B][min(n0,n1)][2] (rows >= n_matches[b] are not written)               */
    int64_t *stop_i64;                     /* [B]                                                                     */
    int64_t *prune0_i64, *prune1_i64;      /* pruning enabled: the final layer counters (lightglue.py:555-558, :605-614) */
    float *prune0_f32, *prune1_f32;        /* pruning disabled: n_layers for live rows (lightglue.py:616-617), 0 for the
                                              padding rows of a ragged batch                                          */
    /* One packed int32 row per pair, the wire format of the pair-sharded multi-GPU path (lightglue_amd/parallel.py, DESIGN.md
     * section 6) — everything the reference's output dict holds for the pair, so that every rank can rebuild the SAME dict for the whole batch:
     *   [matches0 (n0) | scores0 bit patterns (n0) | matches1 (n1) | scores1 bit patterns (n1) | stop | status | prune0 (n0) | prune1 (n1)]
     * prune0/1 are the int32 counters when this forward prunes, else the bit patterns of the reference's float fill (n_layers, lightglue.py:616-617; 0 on
     * the padding rows of a ragged batch).  Row stride wire_stride >= LG_WIRE_WIDTH(n0, n1) elements.  lg_unpack_wire() is the inverse on the receiving side. */
    int32_t *wire; int64_t wire_stride;
    int32_t *status;                       /* [B] LG_OK / LG_ERR_RANGE / LG_ERR_DEVICE / LG_ERR_INDEX per pair        */
    /* ---- indexed inputs: read only when flags & LG_FLAG_INDEXED (together with LG_FLAG_EXT; callers built against the header without them keep working) ----
     * A pair list over feature stores, matched in place.  With the flag set, kpts0 / desc0 / scales0 / oris0 are [images0][n0][..], size0 is [images0][2] and num0 is
     * [images0]: per IMAGE, not per pair, and pair b reads image index0[b] of them; side 1 likewise through index1 / images1 (both sides may point at the same
     * store).  `batch` stays the number of PAIRS of the call and the envelope above applies to batch, n0, n1 as before; offsets into a store are 64-bit, so the
     * number of images is not limited.  Every output stays per pair.  The engine checks 0 <= index < images on the device before it reads through an index: a pair
     * that fails on either side is an empty pair with status LG_ERR_INDEX, so no index value can make the engine read outside a store.  The forward is bit-identical
     * to one on the gathered [batch][n][..] tensors. */
    const int32_t *index0, *index1;        /* [B] image of the store that pair b reads on side 0 / side 1             */
    int32_t images0, images1;              /* images in the store of side 0 / side 1, >= 1                            */
} lg_forward_io;

/* Last error message of the calling thread (never NULL). */
const char* lg_last_error(void);
/* Library / ABI version string. */
const char* lg_version(void);

/* Create an engine on the current HIP device.  Replaces the module construction of
 * LightGlue.__init__ (lightglue.py:388-413). */
int lg_engine_create(const lg_config* cfg, lg_engine** out);
void lg_engine_destroy(lg_engine* e);

/* Stage one state-dict tensor (HOST fp32 pointer, row-major) under its reference name
 * (e.g. "transformers.3.self_attn.Wqkv.weight"; names/shapes: SURVEY.md §8a, lightglue.py:388-407).
 * Replaces load_state_dict (lightglue.py:421/434). */
int lg_engine_set_weight(lg_engine* e, const char* name, const float* host_data, const int64_t* shape, int32_t ndim);
/* Re-pack all staged tensors into kernel layouts / operand precision and upload them. */
int lg_engine_finalize_weights(lg_engine* e);

/* Pre-size the device workspace (otherwise grown on demand inside forward, which synchronises). */
int lg_engine_reserve(lg_engine* e, int32_t max_batch, int32_t max_n0, int32_t max_n1);

/* Enqueue one forward (lightglue.py:483-629) on `hip_stream` (a hipStream_t, NULL = default stream).
 * Asynchronous: no host synchronisation when the workspace is already large enough. */
int lg_engine_forward(lg_engine* e, const lg_forward_io* io, void* hip_stream);

/* Inverse of lg_forward_io.wire on gathered rows (stateless; device pointers; ONE kernel; replaces the slice / widen / index_select chain and the per-pair
 * torch.where of an all-gather consumer): row r of `wire` goes to output pair order[r] (NULL = r; negative = skip the row: the padding rows of a short shard).
 * Writes the reference's output dtypes (lightglue.py:604-629): int64 indices / stop, fp32 scores, prune0/1 as int64 counters (with_prune) or as the float fill,
 * the sorted match list of lightglue.py:593-602 per pair ([pairs_out][kmax][2] int64 + [pairs_out][kmax] scores, kmax = min(n0, n1)) — and `info`,
 * [3][pairs_out] int32 = stop | number of matches | status per OUTPUT pair: the one small block a caller copies to the host (list lengths, B = 1's int stop, and
 * the status every rank must raise on).  Any output pointer may be NULL. */
typedef struct lg_unpack_io {
    const int32_t *wire; int64_t wire_stride; int32_t rows;   /* gathered rows                                           */
    int32_t n0, n1, with_prune, pairs_out;                    /* pairs_out: leading extent of the outputs / of info's rows */
    const int32_t *order;                                     /* [rows] destination pair, or NULL                        */
    int64_t *matches0, *matches1, *stop;                      /* [pairs_out][n0], [pairs_out][n1], [pairs_out]            */
    float *scores0, *scores1;
    int64_t *prune0_i64, *prune1_i64; float *prune0_f32, *prune1_f32;   /* with_prune: the i64 pair, else the f32 pair    */
    int64_t *matches; float *match_scores;                    /* [pairs_out][kmax][2], [pairs_out][kmax]                 */
    int32_t *info;                                            /* [3][pairs_out]: stop, n_matches, status                 */
} lg_unpack_io;
int lg_unpack_wire(const lg_unpack_io* io, void* hip_stream);

/* Engine options (defaults are the product configuration; the others exist for tests, A/B measurements and profiling):
 *   "fused_tail"   1  out_proj + ffn + LayerNorm + GELU + residual as one kernel (lg_tail.hip); 0 = per-op GEMM kernels
 *   "fused_next"   1  the tail kernel also runs the NEXT block's q/k/v projection on the x tile it has just produced
 *                     (bit-identical to the separate kernel; needs fused_tail and 16-bit operand precisions)
 *   "fused_prep"   1  input_dim == 256: keypoint normalisation, Fourier rotary rows, index set and the descriptor copy run inside the first
 *                     projection launch instead of their own kernel (bit-identical; debug stops use the separate kernel)
 *   "attn_rows"    -  query rows per attention wave: 16 | 32 | 64 (bit-identical outputs; the split attention has 16 | 32).  Unset:
 *                     32, and 16 when a launch has fewer 128-row workgroups than the chip has CUs (single pairs); setting it pins
 *                     the shape
 *   "adapt_gather" 1  adaptive width: the SelfBlock projection behind a pruning step gathers its rows through the decide kernel's index map and writes
 *                     them compacted into a second buffer set (no compaction launch; bit-identical to 0 = the in-place compaction kernel)
 *   "sim_planes"   1  precision f16x3: the final projection stores its rows as f16 hi / lo planes and the similarity matrix is multiplied straight from an LDS-DMA
 *                     ring (lg_sim.hip); 0 = fp32 rows + the generic GEMM that splits them per K stage (bit-identical)
 *   "sim_chunk"    0  image-1 rows per workgroup of that kernel: 0 = by grid fill (512 for batches that fill the chip, down to 64 for single pairs), or a multiple of 64
 *   "attn_dma"     1  single-plane 16-bit attention, 32 rows per wave: K / V^T tiles reach LDS by DMA (two buffers, one barrier per
 *                     tile, 4 waves per SIMD); 0 = the register-staged kernel (bit-identical).  The split attention is always DMA
 *   "tail_row_tiles" 0  16-row tiles per fused-tail workgroup: 4 (64 rows) | 2 | 1, 0 = by grid fill (small grids take the
 *                     smaller shapes; bit-identical outputs; the exact fp32 mode always uses 4)
 *   "profile_only" -1 restrict the HIP-event timing of lg_engine_profile_enable to one kernel class (index of
 *                     lg_profile_class_name), -1 = all classes
 *   "tail_timing"  0  shader-clock taps: 1 tail kernel (+ wall-clock life span and CU of every workgroup, tools/tail_wall.py),
 *                     2 self projection, 3 attention (LG_ATTN_TIMING / LG_ATTN_WALL builds) */
int lg_engine_set_option(lg_engine* e, const char* key, int32_t value);

/* ---- test / profiling taps (not used by the product path) ---- */
/* What the matrix pipe sustains on this box: dense bf16 MFMA spin on every SIMD for ~25 ms -> achieved TFLOP/s and the shader
 * clock it ran at (the nominal 2.5 PFLOP/s assumes 2.4 GHz; explains box-to-box throughput differences of one binary). */
int lg_debug_mfma_sustained(double* tflops, double* mhz, void* hip_stream);
/* Stop the next forwards after pipeline step `step` (-1 = run everything).  Step numbering:
 * 0 = prep (+input projection); 1 + 12*layer + k, k = 0 self-QKV, 1 self-attention, 2 out_proj,
 * 3 ffn.0, 4 LayerNorm+GELU, 5 ffn.3+residual, 6 cross-QK/V, 7 cross-attention, 8 to_out, 9 ffn.0,
 * 10 LayerNorm+GELU, 11 ffn.3+residual. */
int lg_engine_debug_stop_after(lg_engine* e, int32_t step);
/* Copy an internal buffer to host (synchronises the device).  Names: X CTX MSG H1 G Q K VT COS SIN MD
 * SIM LS LSNEG CONF MSCORE LSE_R LSE_C IND LEN FINAL_LAYER.  *nbytes_out receives the buffer's byte size;
 * at most max_bytes are copied. */
int lg_engine_debug_read(lg_engine* e, const char* name, void* host_dst, int64_t max_bytes, int64_t* nbytes_out);
/* Row capacities chosen for the last forward (multiples of 128) -> global row = pair*(cap0+cap1) + image*cap0 + r */
int lg_engine_debug_caps(lg_engine* e, int32_t* cap0, int32_t* cap1);

/* ---- per-kernel-class timing with HIP events on the caller's stream (bench.py roofline leg) ---- */
int32_t lg_profile_num_classes(void);
const char* lg_profile_class_name(int32_t cls);
int lg_engine_profile_enable(lg_engine* e, int32_t on);
/* Accumulated milliseconds and launch-site counts per class since the last read (resets). */
int lg_engine_profile_read(lg_engine* e, double* ms, int64_t* count, int32_t n_classes);

/* ------------------------------------------------------------------------------------------------
 * The extractor stages (SuperPoint: encode, detect, sample descriptors; ALIKED: encode, detect, describe): ONE entry point per stage,
 *   int lg_<stage>(const lg_<stage>_io* io, void* hip_stream)
 * in the form of lg_forward_io / lg_nn_io: the arguments are named fields of one struct and the variants of a stage are bits of `flags`, shared by the six:
 *   LG_EXTRACT_RAGGED    images of DIFFERENT sizes in one call: `sizes` is read — a device array int32 [batch][2] = (w_b, h_b) — the arrays of the call are
 *                        CANVASES and image b their top-left corner.  Which (w, h) a stage's `sizes` holds is said at its struct.  Rule of every kernel: addresses
 *                        and strides come from the canvas, every bound (zero padding, stores, pooling, NMS padding, borders, grid normalisation) from the image,
 *                        so nothing outside an image is read — the canvas padding may hold anything, NaN included — and for every image the outputs are
 *                        BIT-IDENTICAL to the batch-1 call on its h_b x w_b crop.  The kernels clamp `sizes` into the canvas (a bad value cannot address outside a buffer);
 *                        validating them (8 <= size <= canvas) is the caller's job, who has them as host integers.  Without the flag `sizes` is never read.
 *   LG_EXTRACT_DESC_F16  lg_sp_sample_descriptors / lg_aliked_describe: the descriptor output is IEEE binary16 instead of fp32 — the last kernel rounds its fp32
 *                        result once, to nearest even, on store: bit-identical to converting the fp32 output, zero padding rows included, at half the bytes written
 *                        (and read by the matcher: LG_FLAG_DESC0_F16 / _DESC1_F16).
 *   LG_EXTRACT_SPLIT     lg_sp_encode: the conv stack on split-f16 operands (see there).
 * Refused with LG_ERR_INVALID and a message before the GPU is touched, by every stage alike: a null `io`; a flag bit the stage does not define (LG_EXTRACT_SPLIT
 * on anything but lg_sp_encode, LG_EXTRACT_DESC_F16 on an encode or detect stage, any other bit); LG_EXTRACT_RAGGED with sizes == NULL ("null pointer").
 * All data pointers are device pointers; kernels are enqueued on the caller's stream; no stage allocates or synchronises. */
#define LG_EXTRACT_RAGGED   1u   /* `sizes` is read: the arrays are canvases, image b their top-left corner */
#define LG_EXTRACT_DESC_F16 2u   /* the descriptor output is binary16, rounded once on the last kernel's store */
#define LG_EXTRACT_SPLIT    4u   /* SuperPoint conv stack on split-f16 operands */

/* ---- SuperPoint descriptor head: the producer of the matcher's descriptor tensors ----
 * Replaces, for descriptor_dim 256 and cell size s (8), the tail of SuperPoint.forward
 * (lightglue/superpoint.py:216-228): optional dense L2 normalisation of the descriptor map (:218),
 * sample_descriptors (:80-95: bilinear grid_sample with align_corners=True and zero padding + L2
 * normalisation) and the transpose to [B][N][256] (:228).  Stateless.
 * LG_EXTRACT_RAGGED: `desc_map` is a descriptor canvas [batch][256][h][w] (as lg_sp_encode wrote it for the same batch) and `sizes` holds the IMAGES' (w_b, h_b):
 * the map of image b is its top-left (h_b / cell, w_b / cell) corner, which alone is read; the grid normalisation and the zero padding of the sampling are that map's. */
typedef struct lg_sp_sample_io {
    int32_t batch, channels, h, w;         /* of desc_map; channels must be 256                                      */
    uint32_t flags;                        /* LG_EXTRACT_RAGGED | LG_EXTRACT_DESC_F16                                 */
    const float *desc_map;                 /* [B][256][h][w] fp32 (NCHW)                                              */
    const int32_t *sizes;                  /* LG_EXTRACT_RAGGED: [B][2] (w, h) of the IMAGES                          */
    const float *keypoints;                /* [B][N][2] fp32 pixel (x, y)                                             */
    const int32_t *num;                    /* [B] live keypoints per image or NULL; rows >= num[b] of `out` are zero-filled */
    int32_t n, cell, normalize_dense;      /* N; cell size s; != 0: the dense L2 normalisation                        */
    float *workspace;                      /* [B][h][w][256] fp32 scratch                                             */
    void *out;                             /* [B][N][256] fp32, or binary16 with LG_EXTRACT_DESC_F16                  */
} lg_sp_sample_io;
int lg_sp_sample_descriptors(const lg_sp_sample_io* io, void* hip_stream);

/* ---- SuperPoint conv stack (replaces superpoint.py:127-141 layers and :159-184, :213-214 of forward) ----
 * lg_sp_pack_conv_weight: repack one nn.Conv2d weight [cout][cin][k][k] (device fp32) into the layout the kernels read,
 *   [k*k][cout][cin] (conv1a: [9][64]); dst holds cout*cin*k*k floats.
 * lg_sp_encode: image [batch][1][h][w] fp32 (grayscale, any h, w >= 8: the 2x2 max-pools floor like nn.MaxPool2d) ->
 *   scores   [batch][h/8*8][w/8*8]    keypoint probabilities after softmax / dustbin removal / depth-to-space (ref :176-184),
 *                                      i.e. cropped to whole 8 x 8 cells like the reference's; the input of lg_sp_detect
 *   desc_map [batch][256][h/8][w/8]   RAW convDb output (NCHW), the input of lg_sp_sample_descriptors(normalize_dense = 1)
 *   params: 24 device pointers = (packed weight, bias) of conv1a, conv1b, conv2a, conv2b, conv3a, conv3b, conv4a, conv4b,
 *           convPa, convPb, convDa, convDb; workspace: lg_sp_encode_workspace_bytes(batch, h, w) bytes.
 * Exact fp32 arithmetic (f32 MFMA): scores agree with an fp32 convolution to round-off.
 * LG_EXTRACT_SPLIT, the opt-in split-f16 form of the same stack (SuperPoint(conv_precision="f16x3")): every MFMA convolution multiplies hi + lo f16 planes of its operands (22 bits) with three
 * v_mfma_f32_16x16x32_f16 per product and fp32 accumulation — the dropped lo x lo term is 2^-24-class, i.e. below the summation-order noise of an fp32 convolution — at a
 * multiple of the f32 MFMA rate.  Values must lie inside the f16 range (|x| < 65504); conv1a (K = 9) stays fp32.  For images — with LG_EXTRACT_RAGGED: a canvas — of
 * h * w < 2^25 pixels (32-bit element offsets inside one image, whose strides are the canvas's; larger ones are refused); params[0..1] (conv1a) packed by
 * lg_sp_pack_conv_weight, the weights of the other eleven layers by lg_sp_pack_conv_weight_split.
 * lg_sp_pack_conv_weight_split: [cout][cin][k][k] fp32 -> hi / lo f16 planes in the order the kernels read (k = 1: [2 planes][cout][cin]; k = 3: MFMA-fragment order
 *   [cout / 64][cin / 32][tap][4 n-tiles][2 planes][64 lanes][8], cout % 64 == 0); dst holds cout*cin*k*k*4 BYTES (as the fp32 form).  cin % 32 == 0.
 * LG_EXTRACT_RAGGED: the batch is a canvas [batch][1][h][w]; image b is its top-left h_b x w_b corner, 8 <= h_b <= h, 8 <= w_b <= w, and `sizes` holds the IMAGES'
 * (w_b, h_b).  Nothing outside an image is read — the canvas padding may hold anything, NaN included; every bound (zero padding, stores, pooling) is the image's.
 * Extents: pyramid level k (h_b >> k, w_b >> k) inside the canvas (h >> k, w >> k); score map ((h_b >> 3) << 3, (w_b >> 3) << 3); descriptor map (h_b >> 3, w_b >> 3).
 * The workspace is lg_sp_encode_workspace_bytes(batch, h, w) of the canvas.  scores [batch][h/8*8][w/8*8]: 0 outside an image's score map; desc_map
 * [batch][256][h/8][w/8]: unspecified outside an image's map (and never read by lg_sp_sample_descriptors under the same flag).
 * Null pointers (a null layer parameter among them), batch < 1, an image or canvas below 8 x 8 and a workspace too small are refused before the GPU is touched. */
int lg_sp_pack_conv_weight(const float* src, int32_t cout, int32_t cin, int32_t k, float* dst, void* hip_stream);
int lg_sp_pack_conv_weight_split(const float* src, int32_t cout, int32_t cin, int32_t k, void* dst, void* hip_stream);
int64_t lg_sp_encode_workspace_bytes(int32_t batch, int32_t h, int32_t w);
typedef struct lg_sp_encode_io {
    int32_t batch, h, w;                   /* of `image` (LG_EXTRACT_RAGGED: the canvas)                              */
    uint32_t flags;                        /* LG_EXTRACT_RAGGED | LG_EXTRACT_SPLIT                                    */
    const float *image;                    /* [batch][1][h][w] fp32                                                   */
    const int32_t *sizes;                  /* LG_EXTRACT_RAGGED: [batch][2] (w, h) of the IMAGES                      */
    const float *const *params;            /* HOST array of the 24 device pointers                                    */
    void *workspace; int64_t workspace_bytes;
    float *scores, *desc_map;              /* [batch][h/8*8][w/8*8], [batch][256][h/8][w/8]                           */
} lg_sp_encode_io;
int lg_sp_encode(const lg_sp_encode_io* io, void* hip_stream);

/* Keypoint extraction from SuperPoint's dense score map: replaces simple_nms (lightglue/superpoint.py:52-70), the
 * border removal, thresholding, per-image split (:186-204), top_k_keypoints (:73-77, :207-215) and the (y, x) -> (x, y)
 * float conversion (:218).  Bit-identical to the reference (all comparisons are exact; ties inside top-k, which
 * torch.topk leaves unspecified, go to the lower row-major index).
 *   scores [B][H][W] fp32 (H, W < 32768); nms_radius <= 4; max_keypoints <= 0 keeps every detection in row-major
 *   order, otherwise (<= 4096) the max_keypoints best sorted by score when more were found (the reference's rule).
 *   keypoints [B][capacity][2] (x, y), kp_scores [B][capacity], counts [B] rows written per image;
 *   totals [B] or NULL: detections above the threshold before top-k / clipping (> max_candidates = overflow).
 *   workspace: lg_sp_detect_workspace_bytes(...) bytes of device scratch.
 * LG_EXTRACT_RAGGED: `scores` is a score canvas [batch][h][w], h, w >= 8, and here `sizes` holds the (w, h) of the SCORE maps (after lg_sp_encode under the same
 * flag: whole cells, (w_b >> 3) << 3).  Pixels outside a map are max_pool2d's -inf padding — not zeros, which would be maxima of their own and suppress real maxima
 * next to the far border — and never pass the threshold; the far borders are the map's.  Keypoints are (x, y) in the image's own frame (the corner is the origin). */
int64_t lg_sp_detect_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t max_candidates);
typedef struct lg_sp_detect_io {
    int32_t batch, h, w;                   /* of `scores`                                                             */
    uint32_t flags;                        /* LG_EXTRACT_RAGGED                                                       */
    const float *scores;                   /* [B][h][w] fp32                                                          */
    const int32_t *sizes;                  /* LG_EXTRACT_RAGGED: [B][2] (w, h) of the SCORE maps                      */
    int32_t nms_radius, remove_borders;
    float detection_threshold;
    int32_t max_keypoints, capacity, max_candidates;
    void *workspace; int64_t workspace_bytes;
    float *keypoints, *kp_scores;          /* [B][capacity][2] (x, y), [B][capacity]                                  */
    int32_t *counts, *totals;              /* [B]; totals may be NULL                                                 */
} lg_sp_detect_io;
int lg_sp_detect(const lg_sp_detect_io* io, void* hip_stream);

/* ---- ALIKED extractor (aliked-n16 / n16rot / n32; lightglue/aliked.py:612-760) ----
 * Exact fp32 arithmetic throughout.  `n_pos` selects the model: 16 (aliked-n16, aliked-n16rot) or 32 (aliked-n32); anything else is
 * refused.  Images: h, w >= 8 and a padded size (h, w rounded up to multiples of 32) below 2^25 pixels.  Device pointers, caller's stream.
 * lg_aliked_pack_weights: the 68 fp32 state tensors of the module in the order
 *     block1: conv1.weight, bn1.{weight, bias, running_mean, running_var}, conv2.weight, bn2.{...}
 *     block2: conv1.weight, bn1.{...}, conv2.weight, bn2.{...}, downsample.{weight, bias}
 *     block3, block4: conv1.offset_conv.{weight, bias}, conv1.regular_conv.weight, bn1.{...}, conv2.offset_conv.{weight, bias},
 *                     conv2.regular_conv.weight, bn2.{...}, downsample.{weight, bias}
 *     conv1 .. conv4 .weight, score_head.{0, 2, 4, 6}.weight,
 *     desc_head: offset_conv.0.{weight, bias}, offset_conv.2.{weight, bias}, sf_conv.weight, agg_weights
 *   -> one packed buffer of lg_aliked_packed_bytes(n_pos) bytes (BatchNorm folded into weights and biases, eps 1e-5).
 * lg_aliked_encode: image [batch][channels = 1 | 3][h][w] -> scores [batch][h][w] (sigmoid score map, unpadded) and the four 32-channel
 *   level maps of x1234 (levels: lg_aliked_levels_bytes bytes, read by lg_aliked_describe); workspace: lg_aliked_workspace_bytes.
 * lg_aliked_detect: DKD (sub-pixel) on the score map.  top_k > 0: the top_k best positive NMS maxima, sorted by score (fewer when the map has
 *   fewer); else threshold mode: scores > scores_th, or > the image's mean score if no pixel of the batch passes (or scores_th <= 0), the
 *   n_limit best sorted by score when more pass, raster order otherwise.  top_k, n_limit <= 20000, capacity >= top_k / n_limit.
 *   image_size [batch][2] (w, h) or NULL.  keypoints [batch][capacity][2] pixel (x, y), kp_scores [batch][capacity], kp_norm [batch][capacity][2]
 *   (the (-1, 1) frame lg_aliked_describe reads), counts [batch]; rows >= counts[b] are zero.  workspace: lg_aliked_detect_workspace_bytes.
 * lg_aliked_describe: SDDH descriptors [batch][n][128] for kp_norm [batch][n][2] (rows >= counts[b] give zero rows); n <= 20000;
 *   workspace: lg_aliked_describe_workspace_bytes(batch * n, n_pos).
 *
 * LG_EXTRACT_RAGGED, for all three: `sizes` holds the IMAGES' (w_b, h_b) and h, w are the CANVAS.  The kernels clamp every size into [1, canvas], so a bad size
 * cannot address outside a buffer; validation proper (8 <= size <= canvas) is the caller's, who has the sizes as host integers.  Geometry:
 *   * image b is the top-left h_b x w_b corner of image[b] ([batch][channels][h][w]); nothing outside it is read (the canvas padding may hold anything).
 *   * each image keeps its OWN InputPadder(divis_by = 32) geometry: Hp_b, Wp_b (h_b, w_b rounded up to 32), pt_b = (Hp_b - h_b) / 2, pl_b = (Wp_b - w_b) / 2,
 *     centred, replicated from the image's own border pixels.
 *   * the padded frame Hp_b x Wp_b of image b is the top-left corner of a padded canvas Hpc x Wpc = the padded size of (h, w); the padding is monotone, so
 *     Hp_b <= Hpc.  lg_aliked_levels_bytes(batch, h, w) / lg_aliked_workspace_bytes(batch, h, w, n_pos) and the level layout are those of the canvas: level
 *     s = 0, 1, 3, 5 is [batch][Hpc >> s][Wpc >> s][32] and image b's part of it the top-left (Hp_b >> s) x (Wp_b >> s).
 *   * addresses and strides come from the canvas, every bound from the image: on no level is anything outside an image's padded frame read (workspace and
 *     level rows there are never written either).  The one exception: scores [batch][h][w] is written 0 outside each image, so it is defined everywhere.
 * Inside the image every output is bit-identical to the uniform call with batch = 1 on the crop.
 * lg_aliked_detect under the flag: the far borders, the soft-argmax window's zero padding, the (w - 1, h - 1) factors and the mean are image b's; keypoints are in
 *   its own frame.  The fallback "no pixel passes scores_th -> the image's mean score" is decided PER IMAGE (the uniform call keeps the reference's whole-batch
 *   rule): a ragged batch is a set of independent images, each equal to its own batch of one.  image_size: as without the flag (NULL: the sizes).
 * lg_aliked_describe under the flag: `levels` as lg_aliked_encode wrote them under it for the same batch, h, w, sizes. */
int64_t lg_aliked_packed_bytes(int32_t n_pos);
int lg_aliked_pack_weights(int32_t n_pos, const float* const* tensors, int32_t n_tensors, void* packed, int64_t packed_bytes, void* hip_stream);
int64_t lg_aliked_levels_bytes(int32_t batch, int32_t h, int32_t w);
int64_t lg_aliked_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t n_pos);
typedef struct lg_aliked_encode_io {
    int32_t batch, channels, h, w, n_pos;  /* of `image` (LG_EXTRACT_RAGGED: the canvas); the model                   */
    uint32_t flags;                        /* LG_EXTRACT_RAGGED                                                       */
    const float *image;                    /* [batch][channels = 1 | 3][h][w] fp32                                    */
    const int32_t *sizes;                  /* LG_EXTRACT_RAGGED: [batch][2] (w, h) of the IMAGES                      */
    const void *packed;                    /* lg_aliked_pack_weights' buffer                                          */
    void *levels;                          /* lg_aliked_levels_bytes(batch, h, w) bytes                               */
    void *workspace; int64_t workspace_bytes;
    float *scores;                         /* [batch][h][w]                                                           */
} lg_aliked_encode_io;
int lg_aliked_encode(const lg_aliked_encode_io* io, void* hip_stream);
int64_t lg_aliked_detect_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t capacity);
typedef struct lg_aliked_detect_io {
    int32_t batch, h, w;                   /* of `scores`                                                             */
    uint32_t flags;                        /* LG_EXTRACT_RAGGED                                                       */
    const float *scores;                   /* [batch][h][w]                                                           */
    const int32_t *sizes;                  /* LG_EXTRACT_RAGGED: [batch][2] (w, h) of the IMAGES                      */
    const float *image_size;               /* [batch][2] (w, h) or NULL                                               */
    int32_t nms_radius;
    float scores_th;
    int32_t top_k, n_limit, capacity;
    void *workspace; int64_t workspace_bytes;
    float *keypoints, *kp_scores, *kp_norm;   /* [batch][capacity][2], [batch][capacity], [batch][capacity][2]        */
    int32_t *counts;                       /* [batch]                                                                 */
} lg_aliked_detect_io;
int lg_aliked_detect(const lg_aliked_detect_io* io, void* hip_stream);
int64_t lg_aliked_describe_workspace_bytes(int32_t rows, int32_t n_pos);
typedef struct lg_aliked_describe_io {
    int32_t batch, h, w, n_pos;            /* of the images `levels` was encoded from (LG_EXTRACT_RAGGED: the canvas); the model */
    uint32_t flags;                        /* LG_EXTRACT_RAGGED | LG_EXTRACT_DESC_F16                                 */
    const void *levels;                    /* as lg_aliked_encode wrote them                                          */
    const int32_t *sizes;                  /* LG_EXTRACT_RAGGED: [batch][2] (w, h) of the IMAGES                      */
    const void *packed;
    const float *kp_norm;                  /* [batch][n][2]                                                           */
    const int32_t *counts;                 /* [batch]                                                                 */
    int32_t n;
    void *workspace; int64_t workspace_bytes;
    void *descriptors;                     /* [batch][n][128] fp32, or binary16 with LG_EXTRACT_DESC_F16 (rows >= counts[b] are zero) */
} lg_aliked_describe_io;
int lg_aliked_describe(const lg_aliked_describe_io* io, void* hip_stream);

/* ---- ImagePreprocessor (lightglue/utils.py:12-38): the resize in front of the extractors, one fused kernel (lg_preprocess.hip) ----
 * What the reference computes through kornia.geometry.transform.resize (always bilinear: `interpolation` is not forwarded):
 *   target size   `resize` = one edge length s + side, with ar = w / h in double: VERT (s, int(s ar)); HORZ (int(s / ar), s); LONG / SHORT:
 *                 (s, int(s ar)) if (side == SHORT) ^ (ar < 1) else (int(s / ar), s) — or an explicit (h, w) pair.  Target == input: identity.
 *   antialias     only if requested and max(h / h_out, w / w_out) > 1: per axis sigma = max((factor - 1) / 2, 0.001), ks = int(max(4 sigma, 3))
 *                 made odd, normalised Gaussian taps, separable blur x then y on the image reflect-padded by ks / 2
 *   bilinear      ATen's float rule: scale = float(in) / out (align_corners: (in - 1) / (out - 1)); src = max(scale (dst + 0.5f) - 0.5f, 0);
 *                 i0 = int(src), i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1 — in fp32, the coordinate expression not contracted
 * lg_preprocess_plan is host-only arithmetic (no GPU, no HIP call): it fills the plan or refuses.  resize_w = LG_RESIZE_EDGE: resize_h is the
 *   edge length and `side` applies; otherwise (resize_h, resize_w) is the target and `side` is ignored (it must still be a valid value).
 * lg_preprocess_resize: src [batch][channels][h][w] addressed through four ELEMENT strides (a channels-last view or a crop is read in place),
 *   float32 or uint8 (converted as float(v) / 255.0f, a true division: the reference's numpy_image_to_torch bit for bit) ->
 *   dst [batch][channels][h_out][w_out] float32 contiguous.  An identity plan is a strided copy / conversion.  Asynchronous on `hip_stream`,
 *   no allocation, no workspace.
 * Envelope — anything outside returns LG_ERR_INVALID with a message before the GPU is touched:
 *   channels 1 or 3; batch <= 65535; every side (input and target) in [1, LG_PREPROCESS_MAX_SIDE];
 *   ks <= LG_PREPROCESS_MAX_TAPS per axis (antialiased downscale factors up to ~17; without antialias any factor);
 *   ks / 2 < the axis length (torch's reflect-pad rule);  strides >= 0 and one image spanning fewer than 2^31 elements (32-bit offsets). */
#define LG_PREPROCESS_MAX_TAPS 33
#define LG_PREPROCESS_MAX_SIDE 8388608   /* 2^23: dst + 0.5f is exact in fp32 below it */
#define LG_RESIZE_EDGE (-1)
enum { LG_SIDE_LONG = 0, LG_SIDE_SHORT = 1, LG_SIDE_VERT = 2, LG_SIDE_HORZ = 3 };
enum { LG_DTYPE_F32 = 0, LG_DTYPE_U8 = 1 };
typedef struct lg_resize_plan {
    int32_t h_in, w_in, h_out, w_out;
    int32_t ks_y, ks_x;          /* blur taps per axis, odd; 1 = no blur                                   */
    int32_t align_corners;
    int32_t identity;            /* target == input size (the reference returns its input)                 */
    double sigma_y, sigma_x;     /* 0 where ks = 1                                                         */
    double scale_x, scale_y;     /* w_out / w_in, h_out / h_in: the `scale` ImagePreprocessor returns      */
} lg_resize_plan;
int lg_preprocess_plan(int32_t h, int32_t w, int32_t resize_h, int32_t resize_w, int32_t side, int32_t antialias, int32_t align_corners,
                       lg_resize_plan* plan);
int lg_preprocess_resize(const void* src, int32_t dtype, int32_t batch, int32_t channels, int32_t h, int32_t w, int64_t stride_b,
                         int64_t stride_c, int64_t stride_y, int64_t stride_x, const lg_resize_plan* plan, float* dst, void* hip_stream);

/* ---- The ragged form: a set of images of DIFFERENT sizes, dtypes and plans into one canvas, ONE launch ----
 * Image b (source b under plan b) is written into the top-left h_out_b x w_out_b corner of plane b of `canvas` [batch][c_out][hc][wc], float32 contiguous;
 * nothing outside that corner is written.  Source channels -> canvas channels: equal counts as they are; 1 -> 3 writes the one result to all three planes;
 * 3 -> 1 is the gray value r * 0.299f + g * 0.587f + b * 0.114f of the three resized channels (three rounded products added in that order, fp32, nothing
 * contracted: what a float32 tensor expression `0.299 * r + 0.587 * g + 0.114 * b` gives).  A plan with `identity` set copies / converts the source values as
 * they are.  Every other pixel equals what the uniform call gives for that image and plan, bit for bit.
 * Split like plan / resize above:
 *   lg_preprocess_ragged_table_bytes: size of the table for `batch` images (0 outside [1, LG_PREPROCESS_RAGGED_MAX_BATCH]).
 *   lg_preprocess_ragged_plan: host-only arithmetic, no HIP call.  Fills `table_host` (caller-owned, `table_bytes` >= the size above) with one record per image
 *     and returns the launch geometry: *total_tiles (the grid: every image's output tiles back to back) and *lds_bytes (the largest image's tile).  Optional
 *     outputs, each [batch] or NULL: tile_prefix (tiles of the images before b: exclusive) and image_lds (LDS bytes of image b's tile shape).
 *   lg_preprocess_resize_ragged: `table_dev` is the caller's DEVICE copy of the same bytes (uploaded by the caller, on `hip_stream` or ordered before it);
 *     `table_host` is read for the geometry only.  zero_fill != 0: the whole canvas is cleared first (hipMemsetAsync on the stream).  Asynchronous, no allocation.
 * Envelope (LG_ERR_INVALID with a message before the GPU is touched): per image exactly that of lg_preprocess_resize; 1 <= batch <=
 *   LG_PREPROCESS_RAGGED_MAX_BATCH; c_out 1 or 3; every target fits (hc, wc); hc * wc < 2^31; total tiles < 2^31; the table buffer large enough; no null pointer. */
#define LG_PREPROCESS_RAGGED_MAX_BATCH 256
typedef struct lg_image_source {
    const void* data;            /* device pointer to the image's first element                            */
    int32_t dtype, channels, h, w;
    int64_t stride_b, stride_c, stride_y, stride_x;   /* element strides as in the uniform call; stride_b is validated and otherwise unused (one image) */
} lg_image_source;
int64_t lg_preprocess_ragged_table_bytes(int32_t batch);
int lg_preprocess_ragged_plan(const lg_image_source* sources, const lg_resize_plan* plans, int32_t batch, int32_t c_out, int32_t hc, int32_t wc,
                              void* table_host, int64_t table_bytes, int64_t* total_tiles, int64_t* lds_bytes, int32_t* tile_prefix, int32_t* image_lds);
int lg_preprocess_resize_ragged(const void* table_host, const void* table_dev, int32_t batch, float* canvas, int32_t zero_fill, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * SIFT helpers (the reference's sift.py:17-56; the detector itself is out of scope).
 *
 * lg_rootsift: dst[r] = RootSIFT of src[r] for `rows` rows of `dim` values — the transform of LG_FLAG_ROOTSIFT0 / _ROOTSIFT1, from the same device code.
 *   src_kind 0: float32, 1: binary16, 2: uint8 rows (contiguous, widened exactly); dst float32, or binary16 with dst_f16 != 0 (the fp32 result rounded once, to
 *   nearest even).  dim a multiple of 4 in [4, 256]; src / dst aligned to the 16 / 8 / 4 bytes of four elements.  One launch on `hip_stream`, no workspace;
 *   rows == 0 is a no-op.
 *
 * lg_sift_filter: the reference's filter_dog_point for `images` images of up to `n` detections each, on the device.
 *   points [images][n][2] (x, y), scales / angles / scores [images][n] float32 (scores NULL: the scales decide), num [images] detections per image (NULL: n),
 *   sizes [images][2] int32 (h, w) on the device, clamped into (max_h, max_w).  With s = scores or scales and pixel p_i = (round_half_even(y_i - 0.5),
 *   round_half_even(x_i - 0.5)):  1. keep i iff s_i == max(0, max s at p_i);  2. of those, iff |angle_i| == min |angle| at p_i;  3. nms_radius > 0: iff the
 *   value kept at p_i equals the maximum over the (2 r + 1)^2 window clipped to the image.  All comparisons exact; the maxima go through integer atomics on the
 *   bit patterns, so the result does not depend on any order.  A detection whose pixel lies outside its image is dropped (the reference wraps or raises).  NaN
 *   inputs are outside the contract.
 *   Outputs: keep [images][n] int64 — the kept indices in ascending order (np.where's), then -1 — and counts [images] int32.
 *   workspace: lg_sift_filter_workspace_bytes(images, n, max_h, max_w) bytes (two max_h x max_w rasters per image and n flags; 0 for arguments outside the
 *   envelope), 256-byte aligned.  Envelope: images in [1, 65535], n in [0, 2^24], max_h x max_w in [1, 2^31 - 1] pixels, nms_radius in [0, 64]. */
int lg_rootsift(const void* src, int32_t src_kind, int64_t rows, int32_t dim, void* dst, int32_t dst_f16, void* hip_stream);
int64_t lg_sift_filter_workspace_bytes(int32_t images, int32_t n, int32_t max_h, int32_t max_w);
int lg_sift_filter(const float* points, const float* scales, const float* angles, const float* scores, const int32_t* num, const int32_t* sizes, int32_t images,
                   int32_t n, int32_t max_h, int32_t max_w, int32_t nms_radius, void* workspace, int64_t workspace_bytes, int64_t* keep, int32_t* counts,
                   void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Nearest-neighbour matcher: mutual nearest neighbour with Lowe's ratio test and a distance threshold, over the same feature stores, pair lists and storage
 * formats as lg_engine_forward — without weights, so without an engine: the two functions below are stateless.  The reference has no such matcher; this is the
 * definition.
 *   rows      a_i (i < num0 of the pair's image 0, else n0) and b_j of image 1, widened exactly from fp32 / binary16 / uint8, RootSIFT first where the side's
 *             LG_FLAG_ROOTSIFT* is set, then L2-normalised in fp32: x / max(|x|_2, 1e-12)
 *   sim[i][j] the dot product of the two normalised rows on fp32 operands with fp32 accumulation, k ascending (v_mfma_f32_16x16x4_f32: an fmaf chain).  The
 *             matrix is never written to memory, and nothing of a call is bounded by LG_MAX_SIM_ELEMS
 *   row i     j1 = the column of the largest sim[i][.], the lowest index among equal values; s1 its value, s2 the largest over j != j1; d = max(2 (1 - s), 0).
 *             kept iff (ratio off, or fewer than two columns, or d1 <= ratio^2 d2) and (distance off or d1 <= distance^2): raw0[i] = j1 if kept, else -1.
 *             Columns likewise with the roles swapped (raw1): the same fp32 sim in both directions.
 *   matches   LG_FLAG_NN_MUTUAL: matches0[i] = raw0[i] if raw0[i] = j >= 0 and raw1[j] == i, else -1 (matches1 likewise); without the flag matches = raw.
 *             scores0[i] = (s1 + 1) / 2 where matches0[i] > -1, else 0.  The list holds the rows (i, matches0[i]) in ascending i and their scores.
 *   Rows at or beyond num0 / num1 come back as -1 / 0 and are never read (they may hold anything); an empty side gives all -1.  NaN / inf inside live rows is
 *   outside the contract (no fault, nothing written out of bounds).
 * Pairs: with LG_FLAG_INDEXED exactly as in lg_forward_io: desc / num are per image of a store and pair p reads images index0[p], index1[p] (an index outside its store:
 *   status LG_ERR_INDEX, the pair is not matched); without it pair p reads image p of either side (images0 / images1 are not read).  Any number of pairs runs in
 *   one call.  The per-side bits LG_FLAG_DESC*_F16, LG_FLAG_DESC*_U8, LG_FLAG_ROOTSIFT* mean what they mean to the engine (LG_FLAG_EXT is not needed).
 * Workspace: lg_nn_workspace_bytes(images0, images1, n0, n1, dim, flags) bytes, 256-byte aligned — the normalised fp32 rows of both stores (each row of an image
 *   the pair list touches is prepared once per call) plus one byte per image: it does not depend on the number of pairs.  -1 for arguments outside the envelope.
 * Envelope (LG_ERR_INVALID with a message before the GPU is touched): dim a multiple of 16 in [16, 256]; n0, n1 in [0, LG_MAX_KEYPOINTS]; a store of at most
 *   2^31 - 1 rows; descriptor pointers 16-byte aligned; ratio_threshold <= 1; no unknown flag; no null pointer among the required ones.
 * A workgroup of the matching kernel owns LG_NN_ROWS_PER_WORKGROUP rows of one side and streams the other side through LDS LG_NN_TILE rows at a time. */
#define LG_FLAG_NN_MUTUAL 1024u
#define LG_NN_ROWS_PER_WORKGROUP 128
#define LG_NN_TILE 64
typedef struct lg_nn_io {
    int32_t pairs, n0, n1, dim;
    uint32_t flags;                        /* LG_FLAG_INDEXED | LG_FLAG_DESC*_F16 | LG_FLAG_DESC*_U8 | LG_FLAG_ROOTSIFT* | LG_FLAG_NN_MUTUAL */
    float ratio_threshold;                 /* in (0, 1]; <= 0: no ratio test                                           */
    float distance_threshold;              /* > 0; <= 0: no distance test                                             */
    const void *desc0, *desc1;             /* [pairs or images][n][dim] in the side's storage format                  */
    const int32_t *num0, *num1;            /* [pairs or images] live rows, or NULL = n                                */
    const int32_t *index0, *index1;        /* [pairs], LG_FLAG_INDEXED                                                */
    int32_t images0, images1;              /* LG_FLAG_INDEXED: images in either store, >= 1                           */
    void *workspace; int64_t workspace_bytes;
    int32_t *raw0, *raw1;                  /* [pairs][n0], [pairs][n1]: the one-directional result; rows >= num are not written */
    int64_t *matches0, *matches1;          /* [pairs][n0], [pairs][n1]                                                */
    float *scores0, *scores1;              /* [pairs][n0], [pairs][n1]                                                */
    int64_t *matches; float *match_scores; /* [pairs][list_rows][2], [pairs][list_rows]; rows >= n_matches[p] are not written */
    int32_t list_rows;                     /* >= min(n0, n1) with LG_FLAG_NN_MUTUAL, else >= n0                       */
    int32_t *n_matches;                    /* [pairs]                                                                 */
    int32_t *status;                       /* [pairs] LG_OK / LG_ERR_INDEX                                            */
    /* optional (NULL = not written): the fields of the matcher's output dict that are constant here, so that no other kernel has to fill them */
    int32_t *stop; int64_t *stop_i64;      /* [pairs] zeros                                                           */
    float *prune0, *prune1;                /* [pairs][n0], [pairs][n1] zeros                                          */
} lg_nn_io;
int64_t lg_nn_workspace_bytes(int64_t images0, int64_t images1, int32_t n0, int32_t n1, int32_t dim, uint32_t flags);
/* Enqueue the whole call on `hip_stream`: asynchronous, no allocation, no host synchronisation. */
int lg_nn_match(const lg_nn_io* io, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Two-view geometric verification of match lists: hypothesise-and-verify RANSAC with a FIXED hypothesis budget, one call for any number of pairs, reading what
 * a matcher leaves on the device (keypoint stores, the pair index, matches0).  Stateless like the nearest-neighbour matcher.  The reference has no such step;
 * this is the definition (tests/twoview_oracle.py restates it in numpy).
 *   correspondences  row i of matches0[p] is a correspondence (kpts0[i], kpts1[m]), m = matches0[p][i], unless m < 0, i >= num0 of the pair's image 0, m >= n1 or
 *             m >= num1 of its image 1: such an entry is unmatched and nothing is read through it.  The S_p correspondences are numbered 0 .. S_p - 1 in ascending i.
 *   models    LG_TWOVIEW_HOMOGRAPHY: x1 ~ H x0, from 4 correspondences.  LG_TWOVIEW_FUNDAMENTAL: x1^T F x0 = 0, from 7, up to 3 real roots per sample (root
 *             index 0 .. 2).  Both map image 0 to image 1 in the keypoints' own units; a model is 9 floats, row-major.
 *   sampling  mix(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16 (uint32 arithmetic).
 *             hash(seed, hypothesis, slot) = mix(mix(seed + 0x9E3779B9 * (hypothesis + 1)) + 0x85EBCA6B * (slot + 1)).
 *             Slot s = 0, 1, .. of hypothesis h draws d = hash(seed, h, s) mod (S_p - s) and skips past the earlier picks: for every earlier pick e in ascending
 *             order, d += 1 if d >= e.  The picks are distinct.  The pair's position in the list is not part of the key.
 *   solving   in Hartley-normalised coordinates, computed once per pair and side over all S_p correspondences: x' = (x - centroid) * sqrt(2) / mean distance
 *             (scale 1 if that distance is 0).  H: the map through the projective basis of the first three picks, valid iff the four triple determinants of
 *             either side all exceed 1e-3 in magnitude.  F: Gauss-Jordan elimination with row pivoting of the 7 x 9 system, columns F21 and F22 free, valid iff
 *             every pivot exceeds 1e-4 in magnitude; the cubic det(N1 + z N2) = 0 in closed form, every root polished by two Newton steps and valid iff
 *             |p'(z)| > 1e-2 (|3 z^2| + |2 A z| + |B|) on the monic cubic p = z^3 + A z^2 + B z + C (a nearly double root is lost to rounding).  The model is
 *             denormalised and scaled to Frobenius norm 1; a model with a non-finite entry is invalid.  An invalid sample scores 0.
 *   scoring   division-free, fp32, threshold t in keypoint units.  F: (x1^T F x0)^2 <= t^2 (|(F x0)_{1,2}|^2 + |(F^T x1)_{1,2}|^2) (squared Sampson distance).
 *             H: with w = h3 . x0, (x1 w - h1 . x0)^2 + (y1 w - h2 . x0)^2 <= t^2 w^2 and w > 0 under the representative +H or -H that gives more inliers:
 *             the sign of a homography matrix carries no meaning.  On a tie it is the representative in output form (below).  The score of a hypothesis is its
 *             inlier count.
 *   winner    most inliers, then the lowest hypothesis index, then the lowest root index (one integer maximum; independent of the launch geometry).
 *   refit     LG_TWOVIEW_REFINE: once, by least squares over the winner's inliers in the pair's normalised coordinates (DLT for H with >= 4 inliers, 8-point
 *             for F with >= 8): the 9 x 9 normal matrix in fp64 summed in a fixed order, its smallest eigenvector by cyclic Jacobi in fp64; F is forced to
 *             rank 2 by F - (F v3) v3^T, v3 the smallest eigenvector of F^T F.  The refit model is kept iff its inlier count is not below the winner's.
 *   outputs   models[p] in output form: Frobenius norm 1, the entry of largest magnitude positive (the first such entry among equals).  inliers0[p][i] = 1 iff row i is an inlier
 *             correspondence; num_inliers[p] their number; matches0_out = matches0 on the inliers, -1 elsewhere; best_hypothesis[p] the winner's hypothesis
 *             index.  An empty result (count 0, zero model, all-false mask, best_hypothesis -1, status LG_OK, nothing non-finite) comes back for S_p below the
 *             sample size and for a pair whose every hypothesis is invalid or without inliers.
 *   LG_TWOVIEW_GIVEN_MODELS skips sampling and solving: hypothesis h of pair p is models_in[p][h] as it stands (invalid iff non-finite or all zero).
 * Pairs: LG_FLAG_INDEXED as in the nearest-neighbour matcher's io (an index outside its store: status LG_ERR_INDEX, an empty result, nothing read through it); without it pair p reads image p.
 * Every pair's result is a function of its own correspondences, the configuration and the seed alone.
 * Workspace: lg_twoview_workspace_bytes bytes (below; -1 outside the envelope), 256-byte aligned: the pair's correspondence list and a 32-byte record.
 * Envelope (LG_ERR_INVALID with a message before the GPU is touched): null io; undefined flag bits; both or neither model bit; n0, n1 in [0, LG_MAX_KEYPOINTS];
 *   num_hypotheses a multiple of 256 in [256, 65536]; threshold > 0; the workspace size and alignment; no null pointer among the required ones.
 * A workgroup of the scoring kernel holds 256 hypotheses, one per lane, and streams the correspondences through LDS LG_TWOVIEW_TILE at a time. */
#define LG_TWOVIEW_HOMOGRAPHY 2048u
#define LG_TWOVIEW_FUNDAMENTAL 4096u
#define LG_TWOVIEW_REFINE 8192u
#define LG_TWOVIEW_GIVEN_MODELS 16384u
#define LG_TWOVIEW_TILE 256
typedef struct lg_twoview_io {
    int32_t pairs, n0, n1, images0, images1;   /* images0 / images1: LG_FLAG_INDEXED only, >= 1                    */
    uint32_t flags;                        /* LG_FLAG_INDEXED | one of LG_TWOVIEW_HOMOGRAPHY, _FUNDAMENTAL | LG_TWOVIEW_REFINE | LG_TWOVIEW_GIVEN_MODELS */
    float threshold;                       /* t > 0, in keypoint units                                                */
    int32_t num_hypotheses;                /* a multiple of 256 in [256, 65536]                                       */
    uint32_t seed;
    const float *kpts0, *kpts1;            /* [pairs or images][n][2], read in place                                  */
    const int32_t *num0, *num1;            /* [pairs or images] live rows, or NULL = n                                */
    const int32_t *index0, *index1;        /* [pairs], LG_FLAG_INDEXED                                                */
    const int64_t *matches0;               /* [pairs][n0]: the matcher's output, read in place                        */
    const float *models_in;                /* [pairs][num_hypotheses][9], LG_TWOVIEW_GIVEN_MODELS only                */
    void *workspace; int64_t workspace_bytes;
    float *models;                         /* [pairs][9]                                                              */
    uint8_t *inliers0;                     /* [pairs][n0]                                                             */
    int32_t *num_inliers;                  /* [pairs]                                                                 */
    int64_t *matches0_out;                 /* [pairs][n0], may be NULL                                                */
    int32_t *best_hypothesis;              /* [pairs], may be NULL                                                    */
    int32_t *status;                       /* [pairs] LG_OK / LG_ERR_INDEX                                            */
} lg_twoview_io;
int64_t lg_twoview_workspace_bytes(int64_t pairs, int32_t n0, uint32_t flags);
/* Enqueue the whole call on `hip_stream`: asynchronous, no allocation, no host synchronisation. */
int lg_twoview_verify(const lg_twoview_io* io, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Relative pose of calibrated pairs: 5-point essential-matrix RANSAC with a FIXED hypothesis budget, then the pose (R, t) of camera 1 against camera 0, one call
 * for any number of pairs, reading the same things the two-view verifier reads plus one pinhole camera per image.  Stateless.  The reference has no such step;
 * this is the definition (tests/relpose_oracle.py restates it in float64 numpy, with a solver of its own).
 * History: added to ABI 0.6 without a version bump; the addition is backward compatible (no existing struct, flag, refusal or formula changed).
 *   correspondences, sampling, pairs, independence: exactly the two-view verifier's (above); a sample is 5 correspondences, slots 0 .. 4 of the hash.
 *   cameras   cameras0[i] / cameras1[j] = (fx, fy, cx, cy), float32, of image i of store 0 / image j of store 1.  A pair whose fx or fy (either side) is not
 *             finite or not > 0, or whose cx or cy is not finite, comes back empty with status LG_ERR_CAMERA (an index outside its store wins: LG_ERR_INDEX,
 *             and no camera is read through it).
 *   bearings  xh = (x - cx) / fx, yh = (y - cy) / fy, formed in float32 (one subtraction, one division, both correctly rounded) and widened to fp64.
 *   model     x1h^T E x0h = 0, E = [t]x R, X1 = R X0 + t, |t| = 1.
 *   solving   fp64 throughout.  Gauss-Jordan elimination with row pivoting of the 5 x 9 system (columns E12, E20, E21, E22 free; invalid if a pivot is not above
 *             1e-9), the four null vectors orthonormalised by modified Gram-Schmidt in that order: E = x X + y Y + z Z + W.  The nine equations
 *             2 E E^T E - tr(E E^T) E = 0 and det E = 0 as a 10 x 20 system in the monomials of (x, y, z), eliminated (row pivoting, invalid if a pivot is not
 *             above 1e-12) down to a 3 x 3 matrix of polynomials in the hidden variable z acting on (x, y, 1) (Nister 2004); its determinant is a polynomial
 *             of degree 10 whose real roots are bracketed between the roots of its derivative (recursively from the 9th derivative up, inside the Cauchy
 *             bound of the polynomial), bisected 64 times and polished by 3 Newton steps that may not leave the bracket.  ROOT ORDER: ascending z, root index
 *             0 .. 9.  (x, y) come from the cross product of the two rows of the 3 x 3 matrix at z whose cross product is longest.
 *   candidate F = K1^-T E K0^-1 in fp64 (pixel units), rounded to float32, scaled to Frobenius norm 1 and put in output form exactly as the verifier's models;
 *             a candidate with a non-finite entry or a zero norm is invalid and all zero, and so are the root slots past a sample's last root.
 *   scoring   THE inlier test of LG_TWOVIEW_FUNDAMENTAL on that F (one piece of code for both entry points): squared Sampson distance, fp32, division-free,
 *             threshold t in pixels.
 *   winner    most inliers, then the lowest hypothesis, then the lowest root: one 64-bit integer maximum per pair,
 *             count << 20 | (65535 - hypothesis) << 4 | (15 - root).  num_hypotheses is a multiple of 256 in [256, 65536].
 *   refit     LG_RELPOSE_REFINE: once, if the winner has >= 8 inliers: linear least squares for E over them in Hartley-normalised bearings (centroid and
 *             sqrt(2) / mean distance per side over ALL S_p bearings of the pair, fp64 sums in the fixed block order, the six numbers rounded to float32), the
 *             9 x 9 normal matrix in fp64 summed in the fixed block order, its smallest eigenvector by cyclic Jacobi; denormalised; projected onto the essential
 *             manifold E <- E (v1 v1^T + v2 v2^T) with v1, v2 the two largest eigenvectors of E^T E and both columns scaled to singular value 1; then
 *             the candidate F as above.  Kept iff its inlier count is not below the winner's.
 *   outputs   models[p]: the pixel-space F of the result (unit norm, output form); inliers0, num_inliers, matches0_out, best_hypothesis as the verifier's.
 *             essentials[p]: K1^T F K0 computed in fp64 from the returned float32 F, scaled to Frobenius norm 1, rounded to float32, in output form.
 *   pose      from essentials[p] as returned (float32 widened to fp64) scaled to Frobenius norm sqrt(2): t0 = the eigenvector of E E^T of smallest eigenvalue
 *             (cyclic Jacobi), its entry of largest magnitude (the first among equals) positive, v3 = that of E^T E; R_a = -[t0]x E + s t0 v3^T,
 *             R_b = +[t0]x E + s t0 v3^T, s = +1 or -1 so that the determinant is positive (with E = U diag(s1, s2, s3) V^T these are U W^T diag(s1, s2, 1) V^T
 *             and U W diag(s1, s2, 1) V^T: the singular values of E do not enter the rotation), each followed by one orthonormalising step
 *             R <- R (3 I - R^T R) / 2.  The four decompositions in the order
 *             (R_a, +t0), (R_a, -t0), (R_b, +t0), (R_b, -t0).  An inlier with bearings b0 = (x0h, y0h, 1), b1 counts for (R, t) iff, with a = R b0, both
 *             (a.b1)(b1.t) - (b1.b1)(a.t) > 0 and (a.a)(b1.t) - (a.b1)(a.t) > 0 (the two depths of the midpoint triangulation, up to their common positive
 *             denominator), in fp64.  The decomposition with the highest count wins, the first in the order above on a tie: rotations[p] (row-major), translations[p]
 *             (unit norm) and num_in_front[p] in float32 / int32.
 *   empty     S_p < 5, no valid candidate with an inlier, LG_ERR_INDEX or LG_ERR_CAMERA: the verifier's empty form, and essentials, rotations, translations all zero,
 *             num_in_front 0.
 *   candidates (optional, may be NULL) [pairs][num_hypotheses][10][9]: the candidate F of every root of every hypothesis, all zero where there is none.
 * Workspace: lg_relpose_workspace_bytes bytes (below; -1 outside the envelope), 256-byte aligned: the verifier's 32-byte record, a 48-byte record (key, cameras),
 *   the correspondence list and its rows per pair, and 360 bytes per hypothesis and pair for the candidates.
 * Envelope (LG_ERR_INVALID with a message before the GPU is touched): the verifier's, with the flag bits LG_FLAG_INDEXED | LG_RELPOSE_REFINE, and null cameras.
 * Four launches: compaction (with the cameras), solve (one hypothesis per lane, 64 lanes per workgroup), score (one candidate per lane, LG_TWOVIEW_TILE
 * correspondences per LDS tile), finalise (one workgroup per pair). */
#define LG_ERR_CAMERA 7    /* per-pair status of the relative-pose estimator: a focal length that is not finite and > 0, or a non-finite principal point */
#define LG_RELPOSE_REFINE 32768u
#define LG_RELPOSE_ROOTS 10
typedef struct lg_relpose_io {
    int32_t pairs, n0, n1, images0, images1;   /* images0 / images1: LG_FLAG_INDEXED only, >= 1                    */
    uint32_t flags;                        /* LG_FLAG_INDEXED | LG_RELPOSE_REFINE                                     */
    float threshold;                       /* t > 0, in pixels                                                        */
    int32_t num_hypotheses;                /* a multiple of 256 in [256, 65536]                                       */
    uint32_t seed;
    const float *kpts0, *kpts1;            /* [pairs or images][n][2], read in place                                  */
    const int32_t *num0, *num1;            /* [pairs or images] live rows, or NULL = n                                */
    const int32_t *index0, *index1;        /* [pairs], LG_FLAG_INDEXED                                                */
    const int64_t *matches0;               /* [pairs][n0]: the matcher's output, read in place                        */
    const float *cameras0, *cameras1;      /* [pairs or images0][4], [pairs or images1][4]: (fx, fy, cx, cy)          */
    void *workspace; int64_t workspace_bytes;
    float *rotations;                      /* [pairs][9]                                                              */
    float *translations;                   /* [pairs][3]                                                              */
    float *essentials;                     /* [pairs][9]                                                              */
    float *models;                         /* [pairs][9]: the pixel-space F                                           */
    float *candidates;                     /* [pairs][num_hypotheses][10][9], may be NULL                             */
    uint8_t *inliers0;                     /* [pairs][n0]                                                             */
    int32_t *num_inliers;                  /* [pairs]                                                                 */
    int64_t *matches0_out;                 /* [pairs][n0], may be NULL                                                */
    int32_t *best_hypothesis;              /* [pairs], may be NULL                                                    */
    int32_t *num_in_front;                 /* [pairs]                                                                 */
    int32_t *status;                       /* [pairs] LG_OK / LG_ERR_INDEX / LG_ERR_CAMERA                            */
} lg_relpose_io;
int64_t lg_relpose_workspace_bytes(int64_t pairs, int32_t n0, int32_t num_hypotheses, uint32_t flags);
/* Enqueue the whole call on `hip_stream`: asynchronous, no allocation, no host synchronisation. */
int lg_relpose_estimate(const lg_relpose_io* io, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Absolute pose of a query camera against a known model: P3P RANSAC with a FIXED hypothesis budget over 2-D - 3-D matches, one call for any number of pairs,
 * reading what a matcher leaves on the device plus one world point per database keypoint and one pinhole camera per query image.  Stateless.  The reference
 * has no such step; this is the definition (tests/abspose_oracle.py restates it in float64 numpy, with a solver of its own).
 * History: added to ABI 0.6 without a version bump; the addition is backward compatible (no existing struct, flag, refusal or formula changed).
 *   sides     side 0 is the query image: kpts0, num0, index0 and cameras0[i] = (fx, fy, cx, cy) of image i (the relative pose's camera rule).  Side 1 is a
 *             database image whose keypoint ROWS carry world points: points3d1[j][m] = (X, Y, Z), float32; a row with a non-finite coordinate has no point.
 *             The keypoints of side 1 are never read.
 *   correspondences  row i of matches0[p] is a correspondence (kpts0[i], points3d1[m]), m = matches0[p][i], unless the verifier's rules make it unmatched
 *             (m < 0, i >= num0, m >= n1, m >= num1) or the point has a non-finite coordinate; nothing is read through an unmatched entry beyond the point's
 *             three floats.
 *   problems  without LG_ABSPOSE_GROUPED problem g is pair g (groups is not read).  With it group_offsets [groups + 1] (ascending, 0 .. pairs) and group_pairs
 *             [pairs] (a permutation of the pairs) define problem g: the pairs group_pairs[group_offsets[g] .. group_offsets[g + 1]) in that order.  The
 *             problem's list is the concatenation of its pairs' lists, each in ascending i, numbered 0 .. S_g - 1.  Every pair reads keypoints through its own
 *             index: grouping pairs of different queries is meaningless but memory safe (offsets are clamped into their range, an entry of group_pairs outside
 *             [0, pairs) is passed over).  A pair with an index outside its store contributes nothing and gets status LG_ERR_INDEX; its problem goes on
 *             without it.  The camera of a problem is that of image 0 of its first pair whose indices lie inside the stores; a problem whose camera fails the
 *             camera rule is empty and each of its pairs (but those with LG_ERR_INDEX) gets LG_ERR_CAMERA.  The same world point reached through several
 *             database images is kept as often as it comes.
 *   centring  c = the centroid of the S_g points, sums in fp64 in the fixed block order, times 1 / S_g, rounded to float32; the list holds X' = X - c (one
 *             float32 subtraction per coordinate).  Solving, scoring and refinement work on X' with t' = t + R c.
 *   sampling  the verifier's hash and skip rule; a sample is 3 correspondences, slots 0 .. 2.  The problem's position in the call is not part of the key.
 *   solving   fp64 throughout.  Bearings f_k = (xh, yh, 1) / |.| with xh = (x - cx) / fx, yh = (y - cy) / fy formed in float32 as in the relative pose, then
 *             widened.  a = |P2 - P3|, b = |P1 - P3|, c = |P1 - P2| of the centred world points; cos A = f2.f3, cos B = f1.f3, cos G = f1.f2.  With depths s1,
 *             s2 = u s1, s3 = v s1 along the bearings the law of cosines gives Grunert's quartic A4 v^4 + .. + A0 = 0; with k = (a^2 - c^2) / b^2 and
 *             m = (a^2 + c^2) / b^2:
 *               A4 = (k - 1)^2 - 4 (c^2 / b^2) cos^2 A
 *               A3 = 4 [k (1 - k) cos B - (1 - m) cos A cos G + 2 (c^2 / b^2) cos^2 A cos B]
 *               A2 = 2 [k^2 - 1 + 2 k^2 cos^2 B + 2 ((b^2 - c^2) / b^2) cos^2 A - 4 m cos A cos B cos G + 2 ((b^2 - a^2) / b^2) cos^2 G]
 *               A1 = 4 [-k (1 + k) cos B + 2 (a^2 / b^2) cos^2 G cos B - (1 - m) cos A cos G]
 *               A0 = (1 + k)^2 - 4 (a^2 / b^2) cos^2 G
 *             u = [(k - 1) v^2 - 2 k cos B v + 1 + k] / (2 (cos G - v cos A)), s1^2 = c^2 / (1 + u^2 - 2 u cos G).  The real roots by the relative pose's
 *             method at degree 4 (brackets between the roots of the derivative inside the Cauchy bound, 64 bisections, 3 Newton steps that may not leave the
 *             bracket).  ROOT ORDER: ascending v, root index 0 .. 3 — the depth ratio of the third pick to the first, a geometric quantity.  A root is
 *             invalid if b^2 = 0, the triangle's normal |(P2 - P1) x (P3 - P1)| <= 1e-12 b c, |A4| = 0 or a coefficient is not finite; if v <= 0,
 *             |cos G - v cos A| <= 1e-12, u <= 0 or 1 + u^2 - 2 u cos G <= 0; or if the pose has a non-finite entry.
 *   pose      of a root: camera points C_k = s_k f_k; the frame e1 = (P2 - P1) / |.|, e3 = e1 x (P3 - P1) normalised, e2 = e3 x e1 of the centred world
 *             points and the same frame of the C_k; R = [e1 e2 e3]_cam [e1 e2 e3]_world^T, t' = mean(C) - R mean(P').  A candidate is (R | t'): 12 floats,
 *             row-major 3 x 4, rounded to float32; an invalid slot is all zero.
 *   scoring   fp32, division-free, explicit fmaf, one piece of code for every entry point: p = R X' + t', each row fmaf(r0, X', fmaf(r1, Y', fmaf(r2, Z', t')));
 *             ex = fmaf(fx, px, (cx - x) pz), ey likewise; inlier iff pz > 0 and fmaf(ex, ex, ey ey) <= t^2 (pz pz): the squared reprojection error in
 *             pixels against t^2.  The score of a candidate is its inlier count.
 *   winner    the relative pose's: most inliers, then the lowest hypothesis, then the lowest root, one 64-bit integer maximum per problem.
 *   refine    LG_ABSPOSE_REFINE: once, if the winner has >= 4 inliers: five Gauss-Newton steps in fp64 from the winner's float32 candidate on the sum of
 *             squared pixel reprojection errors over the WINNER's inlier set (fixed through the steps).  Per inlier, p = R X' + t': residual
 *             r = (fx px / pz + cx - x, fy py / pz + cy - y), Jacobian [[fx / pz, 0, -fx px / pz^2], [0, fy / pz, -fy py / pz^2]] [-[p]x | I] for the
 *             camera-frame twist (w, d); an inlier with pz <= 0 at a step is passed over in that step.  J^T J (21 numbers) and J^T r (6) are summed in the
 *             fixed block order, the 6 x 6 system (J^T J) (w, d) = -J^T r is solved by Gaussian elimination with row pivoting (abandoned, the winner stays,
 *             if a pivot is not above 1e-12 times the largest diagonal entry); R <- Rodrigues(w) R, t' <- Rodrigues(w) t' + d.  The result, rounded to
 *             float32, is kept iff its inlier count is not below the winner's.
 *   outputs   rotations[g] = R and translations[g] = t' - R c formed in fp64 and rounded to float32 (X_cam = R X_world + t).  What comes back is consistent
 *             with itself: num_inliers[g], inliers0, pair_num_inliers and matches0_out are those of the RETURNED pose, re-centred as LG_ABSPOSE_GIVEN_POSES
 *             re-centres a pose, so scoring the returned pose again gives the same bits.  inliers0 / matches0_out / pair_num_inliers / status are per pair,
 *             in the caller's pair order; best_hypothesis[g] is the winner's hypothesis.  The verifier's empty form (zeros, all-false masks, -1, LG_OK)
 *             comes back for S_g < 3 (< 1 with LG_ABSPOSE_GIVEN_POSES) and for a problem without a valid candidate that has an inlier.
 *   candidates (optional, may be NULL) [groups][num_hypotheses][4][12]: every root's candidate in the world frame (t as above), zero where there is none; not written
 *             with LG_ABSPOSE_GIVEN_POSES.
 *   LG_ABSPOSE_GIVEN_POSES skips sampling and solving: hypothesis h of problem g is poses_in[g][h], 12 floats (R | t) in the world frame, root index 0;
 *             t' = t + R c in fp64, rounded to float32; invalid iff non-finite or all zero.
 * Workspace: lg_abspose_workspace_bytes bytes (below; -1 outside the envelope), 256-byte aligned: a 64-byte record per pair and 28 bytes per row of matches0
 *   (six floats and the row's place in its problem).  No candidate is stored: the finalising workgroup solves the winner's sample again.
 * Envelope (LG_ERR_INVALID with a message before the GPU is touched): the verifier's, with the flag bits LG_FLAG_INDEXED | LG_ABSPOSE_REFINE | LG_ABSPOSE_GROUPED
 *   | LG_ABSPOSE_GIVEN_POSES; null points3d1 or cameras0 (poses_in with LG_ABSPOSE_GIVEN_POSES); with LG_ABSPOSE_GROUPED null group arrays, groups outside
 *   [1, pairs] or pairs x n0 above LG_MAX_ROWS.
 * Three launches: compaction with centring (one workgroup per problem), solve + score fused (one hypothesis per lane: its <= 4 candidates stay in registers
 * while the list streams through LDS LG_TWOVIEW_TILE correspondences at a time), finalise (one workgroup per problem). */
#define LG_ABSPOSE_REFINE 65536u
#define LG_ABSPOSE_GROUPED 131072u
#define LG_ABSPOSE_GIVEN_POSES 262144u
#define LG_ABSPOSE_ROOTS 4
typedef struct lg_abspose_io {
    int32_t pairs, n0, n1, images0, images1;   /* images0 / images1: LG_FLAG_INDEXED only, >= 1                    */
    int32_t groups;                        /* LG_ABSPOSE_GROUPED only: problems, in [1, pairs]                        */
    uint32_t flags;                        /* LG_FLAG_INDEXED | LG_ABSPOSE_REFINE | LG_ABSPOSE_GROUPED | LG_ABSPOSE_GIVEN_POSES */
    float threshold;                       /* t > 0, in pixels                                                        */
    int32_t num_hypotheses;                /* a multiple of 256 in [256, 65536]                                       */
    uint32_t seed;
    const float *kpts0;                    /* [pairs or images0][n0][2], read in place                                */
    const float *points3d1;                /* [pairs or images1][n1][3]: the world point of every database keypoint row */
    const int32_t *num0, *num1;            /* [pairs or images] live rows, or NULL = n                                */
    const int32_t *index0, *index1;        /* [pairs], LG_FLAG_INDEXED                                                */
    const int64_t *matches0;               /* [pairs][n0]: the matcher's output, read in place                        */
    const float *cameras0;                 /* [pairs or images0][4]: (fx, fy, cx, cy)                                 */
    const int32_t *group_offsets, *group_pairs;   /* [groups + 1], [pairs]: LG_ABSPOSE_GROUPED only                  */
    const float *poses_in;                 /* [groups][num_hypotheses][12], LG_ABSPOSE_GIVEN_POSES only               */
    void *workspace; int64_t workspace_bytes;
    float *rotations;                      /* [groups][9]                                                             */
    float *translations;                   /* [groups][3]                                                             */
    int32_t *num_inliers;                  /* [groups]                                                                */
    int32_t *best_hypothesis;              /* [groups], may be NULL                                                   */
    float *candidates;                     /* [groups][num_hypotheses][4][12], may be NULL                            */
    uint8_t *inliers0;                     /* [pairs][n0]                                                             */
    int32_t *pair_num_inliers;             /* [pairs]                                                                 */
    int64_t *matches0_out;                 /* [pairs][n0], may be NULL                                                */
    int32_t *status;                       /* [pairs] LG_OK / LG_ERR_INDEX / LG_ERR_CAMERA                            */
} lg_abspose_io;
int64_t lg_abspose_workspace_bytes(int64_t pairs, int32_t n0, int32_t num_hypotheses, uint32_t flags);
/* Enqueue the whole call on `hip_stream`: asynchronous, no allocation, no host synchronisation. */
int lg_abspose_estimate(const lg_abspose_io* io, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Tracks and multi-view triangulation with known poses: the connected components of the match graph of a pair list over ONE feature store, each triangulated
 * from all its views, one call for any number of pairs, reading what a matcher leaves on the device plus one pinhole camera and one pose per image.  What
 * comes back is points3d [images][n][3], the layout lg_abspose_estimate reads as points3d1, in the same convention X_cam = R X_world + t.  Stateless.  The
 * reference has no such step; this is the definition (tests/triangulate_oracle.py restates it in float64 numpy, with a union-find of its own).
 * History: added to ABI 0.6 without a version bump; the addition is backward compatible (no existing struct, flag, refusal or formula changed).
 *   nodes     node v = k n + i is row i of image k; it is live iff i < num[k] (num NULL: n; num[k] is clamped into [0, n]).
 *   edges     row i of pair p = (a, b) = (index0[p], index1[p]) with m = matches0[p][i] is an edge (a n + i, b n + m) iff 0 <= a, b < images and a != b,
 *             i < num[a], 0 <= m < n and m < num[b], and — unless LG_TRI_TRACKS_ONLY — both images pass the camera rule: the relative pose's rule on
 *             cameras[k] = (fx, fy, cx, cy), and every one of the 12 entries of poses[k] = (R | t), row-major 3 x 4, finite.  A pair with an index outside the
 *             store or with a == b contributes nothing and gets status LG_ERR_INDEX; a pair with a failing image contributes nothing and gets LG_ERR_CAMERA
 *             (LG_ERR_INDEX wins when both apply).  Nothing is read through a rejected entry.  A pair listed twice or in both directions adds no new edge.
 *   tracks    a track is a connected component of the edge graph with at least two nodes.  Its name is its lowest node; its observations are its nodes in
 *             ascending node order (by image, then by row).  Tracks are a function of the edge SET alone: the order of the pair list is part of no result,
 *             and every output is the same bits from run to run and under any permutation, duplication or reversal of the list.
 *   node_state  0 not in a track; 1 triangulated; 2 conflict: the track holds two rows of one image; 3 too long: more than max_track_length observations;
 *             4 degenerate: a pivot of the initial 3 x 3 system is not above 1e-12 times its largest diagonal entry, or a non-finite result; 5 an observation
 *             with pz <= 0; 6 an observation's reprojection error above max_reproj_error; 7 no pair of observations with an angle of at least min_angle between
 *             their rays.  The first failing test in the order 3, 2, 4, 5, 6, 7 names the state, and every node of a track carries the track's state.
 *   geometry  fp64 throughout, no fused multiply-add.  The image's R, t and camera are the float32 inputs widened; c = -R^T t, each entry
 *             -((R0j t0 + R1j t1) + R2j t2).  Per observation xh = (x - cx) / fx, yh = (y - cy) / fy are formed in float32 as in the relative pose, then
 *             widened; w = R^T (xh, yh, 1) (entry j: (R0j xh + R1j yh) + R2j), ray d = w / sqrt((w0 w0 + w1 w1) + w2 w2): the norm of the rotated
 *             vector, so that |d| = 1 also under a float32 R, which is orthonormal to 1e-7 only.
 *             Start: [sum (I - d d^T)] X = sum (c - d (d . c)), sums in observation order, by Gaussian elimination with row pivoting: per column each lower
 *             row in turn is exchanged with the pivot row if its entry is strictly larger in magnitude; the pivot must be above 1e-12 times the largest
 *             diagonal entry of the matrix as summed; back substitution x2, x1, x0.
 *   refine    LG_TRI_REFINE: five Gauss-Newton steps on the sum of squared pixel reprojection errors over all observations: p = R X + t (each row
 *             ((r0 X0 + r1 X1) + r2 X2) + t), r = (fx px / pz + cx - x, fy py / pz + cy - y), J = [[fx / pz, 0, -fx px / pz^2], [0, fy / pz, -fy py / pz^2]] R;
 *             an observation with pz <= 0 at a step is passed over in that step; (J^T J) s = -J^T r by the same elimination, X <- X + s.  A failed pivot or
 *             a non-finite step abandons the refinement and the start stays.
 *   accept    on the final X in fp64: the error of an observation is sqrt(rx rx + ry ry), compared with max_reproj_error widened; track_error is the sum of
 *             the errors in observation order divided by their number.  The angle test is on the cosine, without acos: a pair (i, j) passes iff
 *             (X - c_i) . (X - c_j) <= cos(min_angle) |X - c_i| |X - c_j|, cos(min_angle) = cos(min_angle pi / 180) formed once on the host in fp64; with
 *             min_angle = 0 the test is skipped.  Outputs are rounded to float32 once.
 *   outputs   track ids are dense in [0, T), in ascending order of the track's lowest node, over the tracks of state 1.  points3d[v] = the track's point at
 *             every node of such a track, NaN elsewhere; track_id[v] its id, -1 elsewhere; node_state[v]; xyz, track_length, track_error [T] (capacity
 *             images n / 2 entries); counts[0] = T, counts[1 + s] = the tracks of state s (counts[1] = 0); status [pairs].
 *   LG_TRI_TRACKS_ONLY  no geometry: cameras, poses, max_reproj_error and min_angle are not read, every image passes, a track that is neither too long nor
 *             conflicted has state 1 and an id, points3d, xyz and track_error may be NULL and are not written.
 * Workspace: lg_triangulate_workspace_bytes bytes (below; -1 outside the envelope), 256-byte aligned: a 256-byte record, 160 bytes per image, seven int32 per node and
 *   28 bytes per possible track (every second node); it does not depend on the number of pairs.
 * Envelope (LG_ERR_INVALID with a message before the GPU is touched): null io; undefined flag bits; negative counts; n above LG_MAX_KEYPOINTS; images x n (or
 *   images) above LG_MAX_ROWS; pairs x n >= 2^31; max_track_length outside [2, 1024]; without LG_TRI_TRACKS_ONLY max_reproj_error not > 0 and finite or
 *   min_angle outside [0, 180); a null required pointer; a workspace that is too small or not 256-byte aligned.
 * Eight launches, none of which waits on another workgroup: image records and parent[v] = v; union (one lane per row of matches0: a lock-free union-find that
 *   hooks the higher root under the lower by compare-and-swap, parent[v] <= v at every instant); flatten and count; one scan over the roots; fill; sort and
 *   triangulate (one lane per track); one scan over the tracks; scatter. */
#define LG_TRI_REFINE 524288u
#define LG_TRI_TRACKS_ONLY 1048576u
#define LG_TRI_MAX_TRACK_LENGTH 1024
typedef struct lg_triangulate_io {
    int32_t pairs, n, images;
    uint32_t flags;                        /* LG_TRI_REFINE | LG_TRI_TRACKS_ONLY                                      */
    float max_reproj_error;                /* > 0, in pixels                                                          */
    float min_angle;                       /* in [0, 180), degrees                                                    */
    int32_t max_track_length;              /* in [2, LG_TRI_MAX_TRACK_LENGTH]                                         */
    const float *kpts;                     /* [images][n][2], read in place                                           */
    const int32_t *num;                    /* [images] live rows, or NULL = n                                         */
    const int32_t *index0, *index1;        /* [pairs]: both index the one store                                       */
    const int64_t *matches0;               /* [pairs][n]: the matcher's output, read in place                         */
    const float *cameras;                  /* [images][4]: (fx, fy, cx, cy)                                           */
    const float *poses;                    /* [images][12]: (R | t) row-major 3 x 4, X_cam = R X_world + t            */
    void *workspace; int64_t workspace_bytes;
    float *points3d;                       /* [images][n][3]                                                          */
    int64_t *track_id;                     /* [images][n]                                                             */
    uint8_t *node_state;                   /* [images][n]                                                             */
    float *xyz;                            /* [images n / 2][3], the first T written                                  */
    int32_t *track_length;                 /* [images n / 2]                                                          */
    float *track_error;                    /* [images n / 2]                                                          */
    int32_t *counts;                       /* [9]: T, then the tracks of state 0 .. 7                                 */
    int32_t *status;                       /* [pairs] LG_OK / LG_ERR_INDEX / LG_ERR_CAMERA                            */
} lg_triangulate_io;
int64_t lg_triangulate_workspace_bytes(int64_t images, int32_t n, uint32_t flags);
/* Enqueue the whole call on `hip_stream`: asynchronous, no allocation, no host synchronisation. */
int lg_triangulate(const lg_triangulate_io* io, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * The robust mode of the triangulator: per component a consensus over its views, and up to max_tracks tracks out of one component.  One wrong match no
 * longer rejects its track (the observation is left out as an outlier), and two tracks that a wrong match merged come apart again.  lg_triangulate itself is
 * unchanged in every bit and refusal; this is a second entry point over the same io struct.  tests/triangulate_robust_oracle.py restates it in float64 numpy.
 * History: added to ABI 0.6 without a version bump; the addition is backward compatible (no existing struct, flag, refusal or formula changed).
 *   unchanged nodes, edges, statuses, components, their names, the ascending node order of a component's list and the too-long rule (state 3) are those of
 *             lg_triangulate; all geometry is fp64 without fused multiply-add, and "start", "refine" and "accept" above are used as they stand.
 *   rounds    a component with at most max_track_length nodes is processed in up to max_tracks rounds.  A round runs on the list `rest` of L nodes in
 *             ascending order; round 0 runs on all the component's nodes.
 *   hypotheses  the index pairs (i, j), i < j, of `rest` in lexicographic order are numbered 0 .. Q - 1, Q = L (L - 1) / 2.  With Q <= num_hypotheses
 *             hypothesis h is pair h, h in [0, Q); otherwise hypothesis h in [0, num_hypotheses) is pair floor(h Q / num_hypotheses), in 64-bit integers.  No
 *             seed and no hash: the hypotheses are a function of the component alone.  A hypothesis whose two nodes lie in one image is skipped.  Its point is
 *             the start over exactly its two observations, in that order; a failed pivot or a non-finite point skips the hypothesis.
 *   score     an integer: the number of images that own at least one node of `rest` with pz > 0 and error sqrt(rx rx + ry ry) <= max_reproj_error at the
 *             hypothesis' point.  The winner has the highest score; among equal scores the lowest h.
 *   consensus under the winner's point every image contributes its passing node of smallest error; the comparison is a strict < in ascending node order, so
 *             a tie keeps the lowest node.  The consensus list is these nodes in ascending order.
 *   failures  no valid hypothesis: the round fails with state 4; a best score below 2: state 6.
 *   fit       start, refine (with LG_TRI_REFINE) and accept run on the consensus list exactly as lg_triangulate runs them on a whole track; the round's state
 *             is their result.  State 1: the consensus nodes are a track with that point, track_length the consensus size and track_error the mean error;
 *             `rest` becomes the nodes outside the consensus and the next round runs if at least 2 nodes and a round are left.  There is no re-admission of
 *             observations after the fit.  A failed round ends the component.
 *   node_state  a consensus node of a successful round: 1, with that track's id and point.  Round 0 failed: every node of the component carries round 0's
 *             state, as in lg_triangulate.  Otherwise every node left over has state 8, outlier: track_id -1, points3d NaN.  State 2 does not occur.
 *   outputs   track ids are dense in ascending (component name, round).  counts[0] = T, counts[2] = T, counts[1 + s] for s != 1 = the components whose round
 *             0 failed with state s (too long included).  outlier_counts[0] = the nodes of state 8, outlier_counts[1] = the components with more than one
 *             track.  Every output is a function of the edge set alone, the same bits from run to run and under permutation, duplication or reversal of
 *             the pair list.  When the round-0 consensus is the whole component, its point, error and state are bit for bit those of lg_triangulate.
 * Workspace: lg_triangulate_robust_workspace_bytes bytes (-1 outside the envelope): that of lg_triangulate plus two int32 per node and 28 bytes per possible
 *   track and round.
 * Envelope (LG_ERR_INVALID with a message before the GPU is touched): that of lg_triangulate, and LG_TRI_TRACKS_ONLY or any other bit than LG_TRI_REFINE in
 *   base.flags; num_hypotheses outside [1, LG_TRI_MAX_HYPOTHESES]; max_tracks outside [1, LG_TRI_MAX_TRACKS]; a null outlier_counts.
 * Eight launches: the first five of lg_triangulate as they are; then ONE WAVE per component: the list in ascending order by rank, the observations staged in
 *   that wave's LDS slice (12 bytes per node), lanes stride over the hypotheses, an integer wave maximum of score << 16 | (0xFFFF - h) names the winner, one
 *   lane selects the consensus and fits it; one scan over the (component, round) slots; scatter.  No floating-point atomics, and no wave waits on another. */
#define LG_TRI_MAX_HYPOTHESES 4096
#define LG_TRI_MAX_TRACKS 4
typedef struct lg_triangulate_robust_io {
    lg_triangulate_io base;                /* flags: LG_TRI_REFINE only; workspace: lg_triangulate_robust_workspace_bytes */
    int32_t num_hypotheses;                /* in [1, LG_TRI_MAX_HYPOTHESES], per round                                */
    int32_t max_tracks;                    /* in [1, LG_TRI_MAX_TRACKS]: the rounds of one component                  */
    int32_t *outlier_counts;               /* [2]: nodes of state 8, components with more than one track              */
} lg_triangulate_robust_io;
int64_t lg_triangulate_robust_workspace_bytes(int64_t images, int32_t n, int32_t max_tracks);
/* Enqueue the whole call on `hip_stream`: asynchronous, no allocation, no host synchronisation. */
int lg_triangulate_robust(const lg_triangulate_robust_io* io, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Bundle adjustment: joint refinement of the free poses and of all track points by Levenberg-Marquardt on the sum of squared pixel reprojection errors, over
 * what the triangulator returns (track_id, xyz) plus one camera and one pose per image; intrinsics are fixed.  Schur complement onto the poses, dense Cholesky
 * of the reduced camera system, fp64 throughout, no fused multiply-add, one call and one host synchronisation for the whole problem.  Stateless.  The reference
 * has no such step; this is the definition (tests/bundle_oracle.py restates it in float64 numpy, with a solver of its own).
 * History: added to ABI 0.6 without a version bump; the addition is backward compatible (no existing struct, flag, refusal or formula changed).
 *   nodes     as in the triangulator: node v = k n + i, live iff i < num[k] (num NULL: n; clamped into [0, n]).
 *   candidates  node (k, i) with j = track_id[k][i] is a candidate observation of track j iff i < num[k]; 0 <= j < tracks; image k passes the camera rule (the
 *             triangulator's: the relative pose's rule on cameras[k], the 12 entries of poses[k] finite); the three entries of xyz[j] are finite; and at the
 *             INPUT state pz > 0 (pz as in "residual" below, from the widened float32 inputs).
 *   observations  a track with at least 2 and at most LG_BA_MAX_TRACK_LENGTH candidates is ADJUSTED and its candidates are the active observations; the set is
 *             fixed for the whole call.  Its observations are ordered by ascending node (by image, then by row).  Two rows of one image in one track are two
 *             observations.  Every other track is not adjusted: its point comes back as the bits that went in.
 *   node_state  0 not labelled (a dead row, or track_id outside [0, tracks)); 1 active observation; 2 bad image; 3 non-finite point; 4 behind at the start
 *             (pz <= 0); 5 a candidate of a track left with fewer than 2 candidates; 6 a candidate of a track with more than LG_BA_MAX_TRACK_LENGTH.  The first
 *             failing test in the order 0, 2, 3, 4, then 5 / 6 names the state.
 *   status    [images]: LG_ERR_CAMERA for an image that fails the camera rule, else LG_OK.  Such an image takes its observations out (state 2), its pose comes
 *             back as the bits that went in, and everything else is what the same call without its labels gives, bit for bit.
 *   state     poses are carried in fp64 through the call, starting from the float32 inputs widened; the input R is NOT re-orthonormalised, and what comes
 *             back is Rodrigues products of it.  Points likewise.  Outputs are rounded to float32 once.
 *   residual  of observation (k, i) of track j, the triangulator's: p = R X + t (each row ((r0 X0 + r1 X1) + r2 X2) + t), iz = 1 / pz,
 *             r = ((fx px) iz + cx - x, (fy py) iz + cy - y), x, y the float32 keypoint widened.  cost = sum of rx rx + ry ry.
 *   Jacobians  Jp = [[ax, 0, az], [0, by, bz]], ax = fx iz, az = -(((fx px) iz) iz), by = fy iz, bz = -(((fy py) iz) iz).  Point: B = Jp R (2 x 3, the
 *             triangulator's J).  Pose: A = Jp [-[p]x | I] (2 x 6) for the camera-frame twist (w, d), the absolute pose's parametrisation:
 *             A0 = (az py, ax pz - az px, -(ax py), ax, 0, az), A1 = (bz py - by pz, -(bz px), by px, 0, by, bz).
 *             Update: R <- Rodrigues(w) R, t <- Rodrigues(w) t + d, Rodrigues(w) = I + sin(th) [k]x + (1 - cos(th)) [k]x^2, th = |w|, k = w / th (I for th = 0).
 *   gauge     an image is FREE iff it passes the camera rule, constant_pose[k] = 0 and it has at least one active observation.  Every other image keeps its
 *             observations (they enter the points' blocks and the cost) but its 6 columns drop out: identity diagonal block, zero coupling, zero right-hand
 *             side, and its pose comes back as the bits that went in.  Nothing here fixes the gauge if no image is constant: the caller must hold at least one
 *             (the Python layer refuses otherwise); two constant images fix scale, with one the damping holds it.
 *   normal equations  per free image a: U_a = sum A^T A (6 x 6), g_a = sum A^T r, over its active rows in ascending row order.  Per adjusted track j:
 *             V_j = sum B^T B (3 x 3), g_j = sum B^T r, over its observations in order.  Per observation of a free image W = A^T B (6 x 3),
 *             W[r][m] = A0[r] B0[m] + A1[r] B1[m]; W is formed again wherever it is needed, not stored.
 *   damping   Marquardt's: every diagonal entry d of U and V becomes d + lambda clamp(d, 1e-6, 1e32).
 *   points    Vi_j = the inverse of the damped V'_j, column c = the solution of V'_j x = e_c by the triangulator's 3 x 3 elimination and pivot rule (Vi is not
 *             symmetrised); y_j = Vi_j g_j, row r: (Vi[r][0] g0 + Vi[r][1] g1) + Vi[r][2] g2.
 *   reduced system  S of size 6 images x 6 images, lower block triangle.  For free a, free b <= a: E_ab = sum over the active rows i of image a in ascending row
 *             order, and for each over the observations (b, i') of the same track in order, of Y W_(b,i')^T with Y = W_(a,i) Vi_j
 *             (Y[r][m] = (W[r][0] Vi[0][m] + W[r][1] Vi[1][m]) + W[r][2] Vi[2][m]; entry (r, c): (Y[r][0] Wb[c][0] + Y[r][1] Wb[c][1]) + Y[r][2] Wb[c][2]);
 *             S_ab = -E_ab, S_aa = U'_a - E_aa.  Right-hand side of image a: (sum over its active rows in row order of W y_j) - g_a.  Only the lower triangle
 *             of S is read.
 *   Cholesky  S = L L^T, blocked by LG_BA_CHOLESKY_BLOCK = 48 columns, the right-hand side carried as row 6 images of S (so L z = rhs comes out with the factor):
 *             entry (i, j) = S_ij minus the sum of L_ik L_jk over ALL earlier panels' k in ascending order, then the panel's own columns in ascending order.
 *             A pivot that is not > 0 (or not finite) fails the trial; the factorisation goes on with 1 in its place.  L^T s = z backwards gives the pose
 *             steps; per panel the rows below are summed in 5 interleaved partial sums (row i goes to partial (i - first row below) mod 5) added in order 0 .. 4.
 *   point step  X_j <- X_j - (y_j + Vi_j sum over the track's observations of free images, in order, of W^T s_a), W^T s summed over r ascending.
 *   trial     the cost at the trial state: per image the sum over its active rows in ascending row order, the images added in ascending order.  The trial is
 *             REJECTED if an active observation has pz <= 0, a trial pose, point or cost is not finite, a 3 x 3 pivot failed or a Cholesky pivot failed.
 *             Otherwise: converged = |cost - cost_new| <= function_tolerance cost; accepted iff cost_new < cost.  Accepted: the trial becomes the state,
 *             lambda <- max(lambda / 10, 1e-12); else lambda <- min(10 lambda, 1e12).  lambda starts at initial_damping.
 *   stopping  num_iterations is a fixed budget: every launch of every iteration is enqueued unconditionally; cost, lambda, the accept / reject decision and
 *             `converged` live in a device record the kernels read, and once converged the remaining launches return at once.  No host round trip.
 *   outputs   poses [images][12] and xyz [tracks][3] rounded to float32 once (bits unchanged for an image that is not free / a track that is not adjusted);
 *             points3d [images][n][3] = the adjusted point at every active observation's row, NaN elsewhere (what lg_abspose_estimate reads as points3d1);
 *             node_state; observation_error [images][n] = sqrt(rx rx + ry ry) at the final state, NaN where not active; status [images];
 *             summary [8] fp64: initial cost, final cost, iterations run, steps accepted, converged, active observations, final lambda, 0.
 *   Determinism: no floating-point atomics; every sum is a fixed function of position, so every output is the same bits from run to run and under any
 *             relabelling of the tracks (a permutation of the rows of xyz with track_id renamed accordingly).
 * Workspace: lg_bundle_workspace_bytes bytes (below; -1 outside the envelope), 256-byte aligned: a 256-byte record; per image 312 bytes (a 64-byte record, the
 *   pose twice, the step, the cost); S with its right-hand side row, (6 images + 1) x 6 images fp64 (18.9 MB at 256 images); 8 bytes per node (the track list:
 *   node and image); 156 bytes per track (count, offset, cursor, the point twice, Vi, y).  W is recomputed, not stored (it would be 144 bytes per observation).
 * Envelope (LG_ERR_INVALID with a message before the GPU is touched): null io; any flag bit (none is defined); n above LG_MAX_KEYPOINTS; images outside
 *   [1, LG_BA_MAX_IMAGES]; images x n above LG_MAX_ROWS; tracks outside [0, images x n / 2]; num_iterations outside [1, LG_BA_MAX_ITERATIONS]; initial_damping or
 *   function_tolerance not finite and > 0; a null required pointer; a workspace that is too small or not 256-byte aligned.
 * Launches, none of which waits on another workgroup: records; candidates (count); one scan over the tracks; fill; sort (one lane per track); the cost of the
 *   input; then per iteration: points (one lane per track: V, g, Vi, y), reduce (one workgroup per image and 6 column blocks: U, g, the block row of S, rhs),
 *   two launches per Cholesky panel (ONE workgroup factors the diagonal block, then one workgroup per 48-row tile solves its rows below it), back substitution and trial poses (ONE workgroup), trial points (one lane
 *   per track), trial cost (one workgroup per image), decide (one lane); last the scatter. */
#define LG_BA_MAX_IMAGES 256
#define LG_BA_MAX_ITERATIONS 100
#define LG_BA_MAX_TRACK_LENGTH 1024
#define LG_BA_CHOLESKY_BLOCK 48
typedef struct lg_bundle_io {
    int32_t n, images, tracks;
    uint32_t flags;                        /* none defined: must be 0                                                 */
    int32_t num_iterations;                /* in [1, LG_BA_MAX_ITERATIONS]                                            */
    double initial_damping;                /* > 0                                                                     */
    double function_tolerance;             /* > 0                                                                     */
    const float *kpts;                     /* [images][n][2], read in place                                           */
    const int32_t *num;                    /* [images] live rows, or NULL = n                                         */
    const int64_t *track_id;               /* [images][n]: the triangulator's output                                  */
    const float *xyz;                      /* [tracks][3]                                                             */
    const float *cameras;                  /* [images][4]: (fx, fy, cx, cy)                                           */
    const float *poses;                    /* [images][12]: (R | t) row-major 3 x 4, X_cam = R X_world + t            */
    const uint8_t *constant_pose;          /* [images]: non-zero = the pose is held fixed                             */
    void *workspace; int64_t workspace_bytes;
    float *poses_out;                      /* [images][12]                                                            */
    float *xyz_out;                        /* [tracks][3]                                                             */
    float *points3d;                       /* [images][n][3]                                                          */
    uint8_t *node_state;                   /* [images][n]                                                             */
    float *observation_error;              /* [images][n]                                                             */
    double *summary;                       /* [8]                                                                     */
    int32_t *status;                       /* [images] LG_OK / LG_ERR_CAMERA                                          */
} lg_bundle_io;
int64_t lg_bundle_workspace_bytes(int64_t images, int32_t n, int64_t tracks, uint32_t flags);
/* Enqueue the whole call on `hip_stream`: asynchronous, no allocation, no host synchronisation. */
int lg_bundle_adjust(const lg_bundle_io* io, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * The robust mode of the bundle adjuster: a robust loss on the pixel errors (iteratively reweighted least squares) and, in the same call, up to
 * LG_BA_MAX_FILTER_ROUNDS rounds of "drop the observations above max_reproj_error and adjust again".  lg_bundle_adjust itself is unchanged in every bit and
 * refusal; this is a second entry point whose io holds lg_bundle_io as `base`.  tests/bundle_robust_oracle.py restates it in float64 numpy.  Everything not
 * named here is lg_bundle_adjust's definition, word for word.
 * History: added to ABI 0.6 without a version bump; the addition is backward compatible (no existing struct, flag, refusal or formula changed).
 *   loss      for an observation with residual (rx, ry), s = rx rx + ry ry, c = loss_scale (pixels), c2 = c c:
 *             LG_BA_LOSS_SQUARED  rho = s, w = 1;
 *             LG_BA_LOSS_HUBER    rho = s if s <= c2, else (2 c) sqrt(s) - c2;  w = 1 if s <= c2, else c / sqrt(s);
 *             LG_BA_LOSS_CAUCHY   rho = c2 log1p(s / c2);  w = 1 / (1 + s / c2).
 *             cost = sum of rho(s), in the orders of lg_bundle_adjust (per image in ascending row order, the images in ascending order).
 *   weights   first order (iteratively reweighted least squares, no second-order correction): at the accepted state sw = sqrt(w); the two rows of A, the two
 *             rows of B and (rx, ry) are each multiplied by sw ONCE, right after they are formed; every later formula (U, V, g, W, Y, E, the right-hand sides,
 *             the point step) reads the scaled quantities and is otherwise unchanged.  W of an observation therefore carries that observation's weight.  With
 *             LG_BA_LOSS_SQUARED no multiplication is made.  Both robust losses are concave in s, so the weighted quadratic majorises the cost; the accept /
 *             reject / convergence rules are those of lg_bundle_adjust on the sum of rho.  A pz <= 0 or a non-finite s fails a trial as before (its term is 0).
 *   stages    a call runs filter_rounds + 1 stages of num_iterations iterations each.  After every stage but the last, the FILTER: an active observation
 *             whose error at the accepted state exceeds e = max_reproj_error (tested as s > e e, s unweighted) takes node_state 7, filtered.  Then the
 *             tracks' lists and counts and the images' active counts are rebuilt from the nodes still in state 1, in ascending node order: a track left
 *             with fewer than 2 observations stops being adjusted and its remaining observations take state 5; an image left without an active
 *             observation stops being free.  A track or image that stops moving returns its LAST ACCEPTED state, not the bits that went in (a track that
 *             was never adjusted and an image that was never free return their input bits, as in lg_bundle_adjust).  There is no re-admission.
 *             If the filter removed at least one observation: cost is computed again over the new set, lambda returns to initial_damping and `converged`
 *             is cleared.  If it removed none the record is left alone and the next stage goes on where the last one stopped (a converged call stays
 *             converged): a call whose filters remove nothing is, bit for bit, the call with filter_rounds = 0 and num_iterations x (filter_rounds + 1).
 *   stopping  as in lg_bundle_adjust: every launch of every stage is enqueued unconditionally, the decisions live in the device record, one host
 *             synchronisation (the caller's).
 *   outputs   those of lg_bundle_adjust; points3d and observation_error (always the UNWEIGHTED pixel error) are set at the rows active at the end, NaN elsewhere.
 *             summary [12] fp64: 0 the initial cost over the first stage's set under the loss; 1 the final cost over the final set; 2 iterations run and
 *             3 steps accepted, summed over the stages; 4 `converged` of the last stage; 5 active observations at the end; 6 final lambda; 7 zero; 8 filtered
 *             observations; 9 stages in which a filter removed something; 10, 11 zero.
 *   Determinism: as lg_bundle_adjust.  The filter is a per-node test and adds no order; the rebuilt lists are sorted again.  With LG_BA_LOSS_SQUARED and
 *             filter_rounds = 0 every output is that of lg_bundle_adjust bit for bit, and so is LG_BA_LOSS_HUBER while no s exceeds c2 (all weights are 1).
 * Workspace: lg_bundle_robust_workspace_bytes bytes (-1 outside the envelope): that of lg_bundle_adjust plus one int32 per track.
 * Envelope (LG_ERR_INVALID with a message that names the field, before the GPU is touched): that of lg_bundle_adjust (any bit in base.flags included), and
 *   loss outside 0 .. 2; loss_scale not finite or not > 0 when the loss is not squared; filter_rounds outside [0, LG_BA_MAX_FILTER_ROUNDS]; max_reproj_error
 *   not finite or not > 0 when filter_rounds > 0.
 * Launches, none of which waits on another workgroup: those of lg_bundle_adjust per stage, with the loss compiled into points, reduce, trial points and cost;
 *   between two stages the filter (one lane per node, an integer count of what it removed; the same launch clears the tracks' and images' counters), count
 *   (candidate = state 1), scan, fill, sort, the cost of the accepted state and one lane that starts the record again if something was removed. */
#define LG_BA_LOSS_SQUARED 0
#define LG_BA_LOSS_HUBER 1
#define LG_BA_LOSS_CAUCHY 2
#define LG_BA_MAX_FILTER_ROUNDS 4
typedef struct lg_bundle_robust_io {
    lg_bundle_io base;                     /* flags: must be 0; workspace: lg_bundle_robust_workspace_bytes; summary: [12] */
    int32_t loss;                          /* LG_BA_LOSS_*                                                            */
    int32_t filter_rounds;                 /* in [0, LG_BA_MAX_FILTER_ROUNDS]                                         */
    double loss_scale;                     /* c in pixels, > 0 (not read with LG_BA_LOSS_SQUARED)                     */
    double max_reproj_error;               /* e in pixels, > 0 (not read with filter_rounds = 0)                      */
} lg_bundle_robust_io;
int64_t lg_bundle_robust_workspace_bytes(int64_t images, int32_t n, int64_t tracks, uint32_t flags);
/* Enqueue the whole call on `hip_stream`: asynchronous, no allocation, no host synchronisation. */
int lg_bundle_adjust_robust(const lg_bundle_robust_io* io, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * The bundle adjuster with one focal length per image refined next to the poses and the points.  lg_bundle_adjust and lg_bundle_adjust_robust are unchanged
 * in every bit, message and refusal (their kernels' instruction streams are compared in profiles/bundle_adjust_focal.md); this is a third entry point whose
 * io holds lg_bundle_robust_io as `base`.  tests/bundle_focal_oracle.py restates it in float64 numpy.  Everything not named here is lg_bundle_adjust_robust's
 * definition (and through it lg_bundle_adjust's), word for word: candidates, observations, node states, status, the loss and its weights, the stages and the
 * filter, the point blocks, the damping, the accept / reject / convergence rules, the stopping.
 * History: added to ABI 0.6 without a version bump; the addition is backward compatible (no existing struct, flag, refusal or formula changed).
 *   unknowns  image k carries SEVEN: the pose's twist (w, d) as before (columns 0 .. 5) and d_k (column 6), the logarithm of a common scale of fx and fy.
 *             Update: fx <- fx exp(d_k), fy <- fy exp(d_k) (exp of the fp64 library), so the aspect ratio and the sign of the focal lengths stay; cx and cy
 *             are never touched.  The camera state is carried in fp64 through the call like the poses, starting from the float32 inputs widened, it lives
 *             twice (the accepted state and the trial) and every residual, Jacobian, cost and filter test reads the state it belongs to.
 *   Jacobian  column 6 of A at camera-frame point p: (ax px, by py) with ax = fx iz, by = fy iz of lg_bundle_adjust, fx and fy of the ACCEPTED state: the
 *             derivative of ((fx exp(d) px) iz, (fy exp(d) py) iz) at d = 0.  Under a robust loss both entries are multiplied by sw with the rest of the row.
 *   free columns  pose and camera are held independently.  Columns 0 .. 5 of image k are free iff the image is FREE in lg_bundle_adjust's sense (camera rule,
 *             constant_pose[k] = 0, at least one active observation); column 6 is free iff the image passes the camera rule, constant_camera[k] = 0
 *             (constant_camera NULL: no camera is held) and it has at least one active observation.  A held column is lg_bundle_adjust's dropped column:
 *             identity diagonal, zero coupling to every other column (those of its own image included), zero right-hand side, step 0.  An image with a held
 *             pose and a free camera returns its pose as the bits that went in and its focal lengths refined; with a free pose and a held camera the
 *             reverse; an image that fails the camera rule or has no active observation keeps both.  Nothing here fixes the gauge of the poses: the
 *             caller holds at least one, as before.  After a filter an image may lose its last observation: both its pose and its camera then stop moving
 *             and return their last accepted state (lg_bundle_adjust_robust's rule for poses).
 *   layout    the reduced system S has 7 images columns, INTERLEAVED per image: column 7 k + c is unknown c of image k, so block (a, b) is 7 x 7 and the
 *             right-hand side is row 7 images of S.  U_a = sum A^T A (7 x 7), g_a = sum A^T r, W = A^T B (7 x 3), Y = W Vi, E_ab, S_ab = -E_ab,
 *             S_aa = U'_a - E_aa and the right-hand side (sum of W y_j) - g_a are lg_bundle_adjust's formulas with r, c running to 6, over the same rows and
 *             observations in the same orders; every diagonal entry of U, column 6's included, is damped by Marquardt's rule; then the held columns
 *             are overwritten as above.  Cholesky, its panels of LG_BA_CHOLESKY_BLOCK columns, the failed-pivot rule and the back substitution with its five
 *             interleaved partial sums are lg_bundle_adjust's on dim = 7 images (with 7 images the 49 columns cross the first panel by one).
 *   point step  as lg_bundle_adjust with W^T s summed over r = 0 .. 6 ascending, over the track's observations of images with at least one free column
 *             (a held column's step is 0).
 *   trial     as lg_bundle_adjust_robust; additionally a trial is REJECTED if a free camera's trial fx or fy is not finite or not > 0.
 *   outputs   those of lg_bundle_adjust_robust, and cameras_out [images][4]: fx and fy of the accepted state rounded to float32 once for a camera that was
 *             free in any stage, the input's bits for every other camera; cx and cy always the input's bits.  An image with LG_ERR_CAMERA returns its input
 *             row.  summary [12]: as lg_bundle_adjust_robust, and 10 = the number of cameras that were free in any stage.
 *   Determinism: as lg_bundle_adjust (no floating-point atomics, every sum a fixed function of position, the same bits from run to run and under a relabelling
 *             of the tracks).  With every camera held the result is lg_bundle_adjust_robust's within rounding (the same sums at other positions of a wider
 *             matrix: other panels, other partial sums); bit equality is not promised.
 * Workspace: lg_bundle_focal_workspace_bytes bytes (-1 outside the envelope), 256-byte aligned: that of lg_bundle_adjust_robust with 56 bytes of step per
 *   image instead of 48 and S with its right-hand side row as (7 images + 1) x 7 images fp64 (25.7 MB at 256 images instead of 18.9), plus the camera state
 *   twice (64 bytes per image).
 * Envelope (LG_ERR_INVALID with a message that names the field, before the GPU is touched), in this order: null io; the layout (any bit in
 *   base.base.flags, n, images, images x n, tracks: lg_bundle_adjust's bounds); the robust settings (loss, loss_scale, filter_rounds, max_reproj_error:
 *   lg_bundle_adjust_robust's rules); a null cameras_out; then lg_bundle_adjust's list (num_iterations, initial_damping and function_tolerance, a null
 *   required pointer, the workspace).  A null constant_camera is not refused.
 * Launches, none of which waits on another workgroup: those of lg_bundle_adjust_robust, each in the instantiation that reads the camera state; the reduce
 *   runs one workgroup per image and 4 column blocks (4 x 49 entry threads, and in the diagonal workgroup 28 + 7 + 7 threads for U, g and the sum of W y);
 *   the back substitution (ONE workgroup) also writes the trial cameras; the scatter also writes cameras_out. */
typedef struct lg_bundle_focal_io {
    lg_bundle_robust_io base;              /* base.base.workspace: lg_bundle_focal_workspace_bytes; summary: [12]     */
    const uint8_t *constant_camera;        /* [images]: non-zero = the camera is held fixed; NULL = none is held      */
    float *cameras_out;                    /* [images][4]                                                             */
} lg_bundle_focal_io;
int64_t lg_bundle_focal_workspace_bytes(int64_t images, int32_t n, int64_t tracks, uint32_t flags);
/* Enqueue the whole call on `hip_stream`: asynchronous, no allocation, no host synchronisation. */
int lg_bundle_adjust_focal(const lg_bundle_focal_io* io, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * The bundle adjuster with an iterative solver for the reduced camera system: preconditioned conjugate gradients with the block-Jacobi preconditioner
 * (Ceres: ITERATIVE_SCHUR with SCHUR_JACOBI), matrix-free (S is never formed), fp64, for up to LG_BA_PCG_MAX_IMAGES images.  lg_bundle_adjust,
 * lg_bundle_adjust_robust and lg_bundle_adjust_focal are unchanged in every bit, message and refusal; this is a fourth entry point whose io holds
 * lg_bundle_robust_io as `base`.  tests/bundle_pcg_oracle.py restates it in float64 numpy.  Everything outside the linear solve is lg_bundle_adjust_robust's
 * definition (and through it lg_bundle_adjust's), word for word: candidates, node states, status, the loss and its weights, damping, the 3 x 3 point blocks
 * (V', Vi, y), the point step, the trial, accept / reject / convergence, the stages, the filter and the outputs.  Seven unknowns per image are not offered.
 * History: added to ABI 0.6 without a version bump; the addition is backward compatible (no existing struct, flag, refusal or formula changed).
 * Per Levenberg-Marquardt iteration, after the points (V', Vi, y per adjusted track):
 *   setup     per free image a, over its active rows in ascending row order: U_a and g_a (lg_bundle_adjust's; the upper triangle of U is summed and mirrored),
 *             U'_a = U_a with Marquardt's damping on its diagonal, the right-hand side b_a = (sum of W y_j) - g_a, and the lower triangle (c <= r) of
 *             E_aa = the sum over the rows i, and for each over the observations (a, i') of the same track in the track's order, of Y W_(a,i')^T with
 *             Y = W_(a,i) Vi_j (lg_bundle_adjust's formulas and orders; two rows of one image in one track are two observations, each W with its own weight).
 *             S_aa = U'_a - E_aa (lower triangle).  S_aa = L L^T by rows: for entry (i, j), j <= i, the products L_ik L_jk, k < j ascending, are subtracted
 *             from S_ij one at a time; L_ii is the square root of what is left, L_ij that over L_jj.  A pivot that is not > 0 (or not finite) fails the
 *             trial and the factorisation goes on with 1 in its place (the dense path's rule).
 *             M_a = S_aa^-1, column c: L w = e_c forwards, w_i = (e_i less L_ik w_k, k < i ascending, one at a time) / L_ii, then L^T m = w backwards,
 *             m_i = (w_i less L_ki m_k, k = i + 1 .. 5 ascending, one at a time) / L_ii; M[r][c] = m_r (M is not symmetrised).
 *             An image that is not free has no unknowns: its entries of every vector below are 0 and are never read as anything else.
 *   products  M v of image a: entry r is the sum of M[r][c] v_c over c ascending (the first product starts the sum); U' v likewise.
 *   operator  q = S p: per adjusted track j, u_j = Vi_j w with w = the sum over the track's observations of free images, in the track's order, of W^T p_k
 *             (entry m: the sum over r ascending of W[r][m] p_k[r], started at 0 — lg_bundle_adjust's point step with p in place of the step);
 *             u_j[r] = (Vi[r][0] w0 + Vi[r][1] w1) + Vi[r][2] w2.  Per free image a: q_a = U'_a p_a - (the sum over its active rows in ascending row order
 *             of W_(a,i) u_j, entry r: (W[r][0] u0 + W[r][1] u1) + W[r][2] u2).  W is formed again from the pose and the point, as everywhere.
 *   dot       a.b = per image d_k = the sum of a_k[e] b_k[e] over e ascending (the first product starts the sum; 0 for an image that is not free); partial m,
 *             m < 256, = the sum of d_k over the images k = m, m + 256, m + 512, .. ascending, started at 0; then for h = 128, 64, .. 1: partial m +=
 *             partial m + h for every m < h; the result is partial 0.
 *   PCG       x = 0, r = b, z = M r, p = z, rz0 = rz = r.z.  If rz0 is 0 the solve ends at once with x = 0; if it is not finite or < 0 the trial fails.
 *             Step i = 1, 2, ..: q = S p; pq = p.q; a pq that is not > 0 or not finite fails the trial.  alpha = rz / pq; x += alpha p; r -= alpha q
 *             (each entry x + alpha p, r - alpha q); z = M r; rz' = r.z; an rz' that is not finite or < 0 (a non-finite vector entry shows here) fails
 *             the trial.  The solve ends on the tolerance iff sqrt(rz') <= cg_tolerance sqrt(rz0), else on the budget iff i = max_cg_iterations; otherwise
 *             beta = rz' / rz, p = z + beta p, rz = rz'.  A trial that failed in the points, the setup or the solve is rejected by lg_bundle_adjust's rule.
 *             The pose step is x; trial poses, trial points, cost and the decision are lg_bundle_adjust's.
 *   stopping  the budget is fixed like num_iterations: every launch of every solver iteration of every Levenberg-Marquardt iteration is enqueued
 *             unconditionally; "this solve is done" is a field of the device record that only the single-workgroup step kernel writes, and once it is
 *             set, or `converged` or the trial's failure is, the solve's remaining launches return at once.
 *   outputs   those of lg_bundle_adjust_robust, summary [12] with 7 = the solver iterations run over the whole call and 11 = the Levenberg-Marquardt
 *             iterations whose solve ended on the budget.
 *   Determinism: as lg_bundle_adjust: no floating-point atomics, every sum a fixed function of position, the same bits from run to run and under a
 *             relabelling of the tracks.
 * Workspace: lg_bundle_pcg_workspace_bytes bytes (-1 outside the envelope), 256-byte aligned, every piece rounded up to 256 bytes: that of
 *   lg_bundle_adjust_robust without S, plus a 256-byte record, 784 bytes per image (r, z, p, q: 4 x 48; U' and M: 2 x 288; the image's partials of p.q and
 *   r.z: 2 x 8; x is lg_bundle_adjust's step) and 24 bytes per track (u).
 * Envelope (LG_ERR_INVALID with a message that names the field, before the GPU is touched), in this order: null io; lg_bundle_adjust's layout bounds with
 *   images in [1, LG_BA_PCG_MAX_IMAGES] (images x n <= LG_MAX_ROWS still binds); the robust settings; pad not 0; max_cg_iterations outside
 *   [1, LG_BA_PCG_MAX_CG_ITERATIONS]; cg_tolerance not in (0, 1) (NaN included); num_iterations x (filter_rounds + 1) x max_cg_iterations above
 *   LG_BA_PCG_MAX_SOLVER_ITERATIONS (the call enqueues that many solver iterations); then lg_bundle_adjust's list.
 * Launches, none of which waits on another workgroup: those of lg_bundle_adjust_robust with reduce, the Cholesky panels and the back substitution replaced by
 *   setup (one workgroup per image) and, max_cg_iterations times, tracks (one lane per track: u), images (one workgroup per image: q and its partial of
 *   p.q) and step (ONE workgroup: the dots, alpha, beta, x, r, z, p, the record, and the trial poses when the solve ends); last one lane writes summary
 *   7 and 11. */
#define LG_BA_PCG_MAX_IMAGES 4096
#define LG_BA_PCG_MAX_CG_ITERATIONS 1000
#define LG_BA_PCG_MAX_SOLVER_ITERATIONS 20000
typedef struct lg_bundle_pcg_io {
    lg_bundle_robust_io base;              /* base.base.workspace: lg_bundle_pcg_workspace_bytes; summary: [12]       */
    int32_t max_cg_iterations;             /* in [1, LG_BA_PCG_MAX_CG_ITERATIONS]                                     */
    int32_t pad;                           /* must be 0                                                               */
    double cg_tolerance;                   /* in (0, 1)                                                               */
} lg_bundle_pcg_io;
int64_t lg_bundle_pcg_workspace_bytes(int64_t images, int32_t n, int64_t tracks, uint32_t flags);
/* Enqueue the whole call on `hip_stream`: asynchronous, no allocation, no host synchronisation. */
int lg_bundle_adjust_pcg(const lg_bundle_pcg_io* io, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Global poses: one pose per image from the relative poses of a pair list (what lg_relpose_estimate returns), by rotation averaging over the view graph and
 * position averaging along the pairs' translation directions, both robust to wrong pairs; the per-image poses are what lg_triangulate and lg_bundle_adjust
 * take.  fp64 throughout, no fused multiply-add, dense Cholesky, one call and one host synchronisation.  Stateless.  The reference has no such step; this is
 * the definition (tests/posegraph_oracle.py restates it in float64 numpy).
 * History: added to ABI 0.6 without a version bump; the addition is backward compatible (no existing struct, flag, refusal or formula changed).
 *   inputs    pair p = (a, b) = pair_index[p]; rotations[p] = R_ab (row-major 3 x 3) and translations[p] = t_ab with X_b = R_ab X_a + t_ab, t_ab a direction
 *             (any length > 0); weights[p]; num_inliers[p] if given.  All float32, widened; R_ab is NOT re-orthonormalised.  Angles of the io are degrees.
 *   pair_state  0 used; 1 a or b outside [0, images) or a = b; 2 no model: an entry of R_ab not finite, an entry of R_ab^T R_ab further than 1e-3 from the
 *             identity, det R_ab <= 0, t_ab not finite or |t_ab|^2 not > 0, the weight not finite and > 0, or num_inliers[p] < min_inliers; 3 outside the
 *             origin's component; 4 rotation outlier; 5 touches an image without a position.  The first failing test in this order names the state; a pair
 *             takes part in a step iff none of the tests before that step failed (4 and 5 still enter the rotations, 5 not the positions).
 *   image_state  0 posed; 1 rotation only (in the origin's component, no position); 2 not connected to the origin.
 *   adjacency  every pair that passes 1 and 2 is listed under both of its images; an image's list is in ascending (neighbour image, pair index) order and every
 *             sum below over an image's pairs runs in that order.  A pair listed twice, in either direction, is two entries.
 *   tree      level-synchronous breadth-first search from `origin` (level 0, rotation I): an image without a level takes as parent the neighbour ON THE CURRENT
 *             LEVEL over its heaviest pair, the first such entry of its list on ties; R_i = R_ab R_a if it is the pair's b, R_ab^T R_b if it is its a.  The
 *             images reached are the origin's component.
 *   log       of M: v = (M21 - M12, M02 - M20, M10 - M01), tr = (M00 + M11) + M22, theta = atan2(|v| / 2, (tr - 1) / 2), omega = (theta / |v|) v; if
 *             |v| < 1e-6: omega = v / 2, or 0 if tr < 0.  exp is the bundle adjuster's Rodrigues.
 *   rotation averaging  num_iterations steps of reweighted Gauss-Newton.  Iteration it: per pair omega = log(R_b^T (R_ab R_a)), theta = |omega|,
 *             w' = w / (1 + (theta / s)^2), s = rotation_scale max(1, 2^(n - 5 - it)).  System: images x images, row i: diagonal = sum of w' over i's list,
 *             entry (i, j) = -(sum of w' over the entries with neighbour j), right-hand sides (three columns) = sum of +w' omega where i is the pair's b,
 *             -w' omega where it is its a.  The origin and every image outside the component: identity row and column, zero right-hand side.  Solved by the
 *             Cholesky below; R_i <- R_i exp(delta_i).  The stage ends after the update of an iteration with s = rotation_scale, every delta finite and
 *             max |delta| < 1e-10.  Then rotation_error[p] = |omega| in degrees at the final rotations (NaN for states 1 .. 3); above max_rotation_error: 4.
 *   direction  d_p = -R_b^T (t_ab / |t_ab|): from the centre of a to the centre of b, with the solved R_b.
 *   baseline  the neighbour of `origin` over its heaviest pair of state 0 (to `baseline` if that is >= 0), the first such entry on ties; c_origin = 0,
 *             c_baseline = d_p of that pair, or -d_p if the origin is its b.  No such pair: no positions (as after a failed pivot below; 0 iterations).
 *   positions  which images get one: start with the component; repeat until nothing changes (all images at once per round): drop every image other than the
 *             origin and the baseline that has state-0 pairs to fewer than two different images still there.  A state-0 pair with a dropped image: 5.
 *   position averaging  num_iterations steps of reweighted least squares on the sum of w rho |(I - d d^T)(c_b - c_a)|^2 over the state-0 pairs.  Iteration 0:
 *             rho = 1.  Later, with e = c_b - c_a of the previous iterate: rho = (1 / max(|e|^2, 1e-12)) / (1 + (phi / s)^2), phi = atan2(|e - (d . e) d|, d . e),
 *             s = direction_scale max(1, 2^(n - 6 - it)).  System: 3 images x 3 images of 3 x 3 blocks M = (w rho)(I - d d^T): diagonal block = sum of M over
 *             the image's list, block (i, j) = -(sum over the entries with neighbour j); the origin, the baseline and every image without a position:
 *             identity rows and columns; the baseline's centre moves to the right-hand side (sum of M c_baseline over the entries with that neighbour).
 *             The stage ends after an iteration with s = direction_scale, every step finite and max |c_new - c_old| < 1e-12.
 *   Cholesky  the bundle adjuster's (48 columns per panel, right-hand sides as extra rows, the same order of every sum, the same substitution), except for
 *             the pivot rule: a pivot fails unless it is finite and > 1e-10 x the diagonal entry it started from (a system that is singular in exact
 *             arithmetic leaves rounding noise of either sign there: a sign test alone would decide by chance).  It goes on with 1 in its place.  A failed
 *             pivot of ANY position iteration clears positions_ok: every image of the component is "rotation only".  (The rotation system of a connected
 *             component with finite weights is positive definite; a failed pivot there is not reported.)
 *   outputs   poses [images][12] (R | t) rounded to float32 once, t_i = -(R_i c_i) (each row (r0 c0 + r1 c1) + r2 c2): R NaN for state 2, t NaN for states
 *             1 and 2; direction_error[p] = phi in degrees at the final centres for state 0 with positions_ok, else NaN;
 *             summary [8] fp64: origin, baseline (-1: none), images posed, rotation iterations run, position iterations run, positions_ok, 0, 0.
 *   Determinism: no floating-point atomics; every sum is a fixed function of the lists' order, so every output is the same bits from run to run, and under a
 *             permutation of a pair list in which no image pair appears twice (then an image's list order does not depend on the pair indices).
 * Workspace: lg_posegraph_workspace_bytes bytes (below; -1 outside the envelope), 256-byte aligned: a 256-byte record; 116 bytes per image; 52 bytes per
 *   pair; the position system with its right-hand side row, (3 images + 1) x 3 images fp64 (4.7 MB at 256 images), every piece rounded up to 256 bytes.
 * Envelope (LG_ERR_INVALID with a message before the GPU is touched): null io; any flag bit (none is defined); images outside [2, LG_BA_MAX_IMAGES]; pairs
 *   outside [1, 2^20]; num_iterations outside [LG_PG_MIN_ITERATIONS, LG_BA_MAX_ITERATIONS]; origin outside [0, images); baseline neither -1 nor an image other
 *   than origin; a scale or max_rotation_error not finite and > 0; a null required pointer (num_inliers may be NULL); a workspace too small or not aligned.
 * Launches, none of which waits on another workgroup: clear, classify, scan, fill, sort (one lane per image), tree (ONE workgroup); per rotation iteration
 *   assemble (one workgroup per image row), two per Cholesky panel, update (ONE workgroup); select (ONE workgroup); per position iteration the same four kinds
 *   over 3 images columns; output.  8 + n (4 + 2 ceil(images / 48) + 2 ceil(3 images / 48)) in all; after a stage has ended its launches return at once. */
#define LG_PG_MIN_ITERATIONS 6
typedef struct lg_posegraph_io {
    int32_t images, pairs;
    uint32_t flags;                        /* none defined: must be 0                                                 */
    int32_t num_iterations;                /* of EACH stage, in [LG_PG_MIN_ITERATIONS, LG_BA_MAX_ITERATIONS]          */
    int32_t origin;                        /* the image whose pose is the identity                                    */
    int32_t baseline;                      /* the image at distance 1 from it, or -1: chosen on the device            */
    int32_t min_inliers;                   /* read only with num_inliers                                              */
    double rotation_scale;                 /* degrees, > 0                                                            */
    double max_rotation_error;             /* degrees, > 0                                                            */
    double direction_scale;                /* degrees, > 0                                                            */
    const int64_t *pair_index;             /* [pairs][2]: (a, b)                                                      */
    const float *rotations;                /* [pairs][9]                                                              */
    const float *translations;             /* [pairs][3]                                                              */
    const float *weights;                  /* [pairs]                                                                 */
    const int32_t *num_inliers;            /* [pairs], or NULL                                                        */
    void *workspace; int64_t workspace_bytes;
    float *poses;                          /* [images][12]                                                            */
    uint8_t *image_state;                  /* [images]                                                                */
    uint8_t *pair_state;                   /* [pairs]                                                                 */
    float *rotation_error;                 /* [pairs] degrees                                                         */
    float *direction_error;                /* [pairs] degrees                                                         */
    double *summary;                       /* [8]                                                                     */
} lg_posegraph_io;
int64_t lg_posegraph_workspace_bytes(int64_t images, int64_t pairs, uint32_t flags);
/* Enqueue the whole call on `hip_stream`: asynchronous, no allocation, no host synchronisation. */
int lg_posegraph_solve(const lg_posegraph_io* io, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Global poses with an iterative solver for both stages: preconditioned conjugate gradients with the (block-)Jacobi preconditioner, matrix-free (neither
 * system is formed: both are operators over the images' adjacency lists), fp64, for up to LG_BA_PCG_MAX_IMAGES images.  lg_posegraph_solve is unchanged in
 * every bit, message and refusal; this is a second entry point whose io holds lg_posegraph_io as `base`.  tests/posegraph_pcg_oracle.py restates it in
 * float64 numpy.  Everything outside the two linear solves is lg_posegraph_solve's definition, word for word: pair and image states, the adjacency and its
 * order, the tree, log / exp, the weights and their schedules, the baseline, the peeling, the direction, the stage-convergence tests (1e-10 / 1e-12) and the
 * outputs.
 * History: added to ABI 0.6 without a version bump; the addition is backward compatible (no existing struct, flag, refusal or formula changed).
 *   list sum  THE order of every sum over an image's list below: the entries that take part keep their positions e = 0, 1, .. in the sorted list (an entry
 *             that does not take part adds nothing); partial l, l < 64, = the sum of the terms at positions l, l + 64, l + 128, .. ascending, started at 0;
 *             then for h = 32, 16, .. 1: partial l += partial l + h for every l < h; the result is partial 0.  A vector or block is summed entry by entry.
 *   free      rotation stage: an image of the origin's component other than the origin.  Position stage: an image that gets a position other than the
 *             origin and the baseline.  An image that is not free has no unknowns: its entries of r, z, p, q, x are 0 and are never read as anything else.
 *   rotation stage, iteration it.  Per pair of state 0: omega and w' of lg_posegraph_solve, and the vector w' omega (each entry w' x omega_r).  Per free
 *             image i: D_i = the list sum of w'; b_i = the list sum of +(w' omega) where i is the pair's b, -(w' omega) where it is its a.  The unknown
 *             is the 3-vector delta_i per free image; operator q_i = D_i p_i - (the list sum of w'_p p_j over the entries (j, p)), each entry of q_i
 *             D_i p_i[r] less the sum; preconditioner z_i = (1 / D_i) r_i (the reciprocal is formed once).  x0 = 0, r = b.  R_i <- R_i exp(x_i).
 *   position stage, iteration it.  Per pair of state 0: M = (w rho)(I - d d^T) as six entries (lg_posegraph_solve's rho, schedule and block).  Per free
 *             image i: D_i = the list sum of M; b_i = the list sum of M c_baseline over the entries whose neighbour is the baseline; t_i = the list sum of
 *             M c_j over all other entries, c_j the current centre (0 for the origin).  M v: each row (m0 v0 + m1 v1) + m2 v2.  Operator q_i = D_i p_i
 *             - (the list sum of M p_j).  Preconditioner z_i = Di_i r_i (rows as above) with Di_i = D_i^-1 column by column by the 3 x 3 elimination of
 *             lg_triangulate (partial pivoting; a pivot must exceed 1e-12 x the block's largest diagonal entry).  A block that fails it, in ANY position
 *             iteration, clears positions_ok like the dense path's failed pivot, and the position stage ends there (the centres keep their last values;
 *             the iteration is counted).  Collinear cameras give blocks of rank 2 up to rounding and are caught here.
 *             Warm start: the system is solved for the centres themselves, so x0 = the current centres (0 at iteration 0) and
 *             r_i = b_i - (D_i c_i - t_i).  Started from 0 at cg_tolerance 1e-6 the poses sit up to 5e-6 from the dense definition, warm-started 2e-11.
 *   dot       a.b = per image d_k = (a0 b0 + a1 b1) + a2 b2 (0 for an image that is not free), then lg_bundle_adjust_pcg's fold of the images' d_k
 *             (256 partials, a halving tree).
 *   PCG       lg_bundle_adjust_pcg's recurrence and stopping rule: z = M r, p = z, rz0 = rz = r.z with r the (warm-started) residual.  rz0 = 0 ends the
 *             solve at once with x = x0.  Step i = 1, 2, ..: q = A p; pq = p.q; alpha = rz / pq; x += alpha p; r -= alpha q; z = M r; rz' = r.z.  The
 *             solve ends on the tolerance iff sqrt(rz') <= cg_tolerance sqrt(rz0), else on the budget iff i = the stage's budget; otherwise
 *             beta = rz' / rz, p = z + beta p, rz = rz'.  A pq that is not finite and > 0, or an rz0 / rz' that is not finite and >= 0, is a failed
 *             recurrence: in the rotation stage the solve ends with the step taken so far (which is applied), in the position stage it clears
 *             positions_ok and ends the stage like a failed block.  Either is counted in summary 6.
 *   update    when a solve ends: the rotations or centres of the free images take x, and the stage's iteration counter, largest step and convergence are
 *             lg_posegraph_solve's.
 *   stopping  both budgets are fixed like num_iterations: every launch of every solver iteration of every iteration of both stages is enqueued
 *             unconditionally; "this solve is done" is a field of the device record that only the single-workgroup step kernel writes, and once it is
 *             set, or the stage has ended, the remaining launches return at once.
 *   outputs   those of lg_posegraph_solve; summary [12]: the eight values of lg_posegraph_solve with 6 = failed recurrences, then 8 = rotation solver
 *             iterations run over the call, 9 = position solver iterations run, 10 = rotation solves that ended on the budget, 11 = position solves that
 *             ended on the budget.
 *   Documented difference: positions_ok = 0 is reported only for a missing baseline, a failed 3 x 3 block and a failed recurrence.  A view graph whose
 *             position system the dense path calls singular by its pivot floor is NOT recognised: an iterative solve has no pivot to test.  On 1 100 images
 *             with 3 300 pairs (3 per image) the dense definition fails a pivot and returns positions_ok = 0; this solver converges (up to 918 solver
 *             iterations in one solve) to centres 4.35 x the scene's extent off.  With 8 pairs per image (1 100 / 8 800, 600 / 4 800) both definitions
 *             pose every image and agree (centre error 0.25 - 0.29 % of the extent).  The caller's signals are direction_error and summary 10 / 11.
 *   Determinism: as lg_posegraph_solve: no floating-point atomics, every sum a fixed function of the lists' order and the image index.
 * Workspace: lg_posegraph_pcg_workspace_bytes bytes (-1 outside the envelope), 256-byte aligned, every piece rounded up to 256 bytes: that of
 *   lg_posegraph_solve without the dense system, plus a 256-byte record, 48 bytes per pair (w' and w' omega, or M) and 256 bytes per image (r, z, p, q, x:
 *   5 x 24; D: 48; D^-1: 72; the image's partials of p.q and r.z: 2 x 8): 512 + 372 images + 4 + 100 pairs before the rounding.
 * Envelope (LG_ERR_INVALID with a message that names the field, before the GPU is touched), in this order: null io; any flag bit; images outside
 *   [2, LG_BA_PCG_MAX_IMAGES]; pairs outside [1, 2^20]; lg_posegraph_solve's settings (num_iterations, origin, baseline, the scales); rotation_cg_iterations
 *   outside [1, LG_BA_PCG_MAX_CG_ITERATIONS]; position_cg_iterations likewise; cg_tolerance not in (0, 1) (NaN included); num_iterations x
 *   (rotation_cg_iterations + position_cg_iterations) above LG_BA_PCG_MAX_SOLVER_ITERATIONS (the call enqueues that many solver iterations); a null required
 *   pointer; the workspace.
 * Launches, none of which waits on another workgroup: clear, classify, scan, fill, sort and output are lg_posegraph_solve's; tree and select are ONE workgroup
 *   of 1 024 threads with the images strided over the lanes (the same decisions); per iteration of a stage pairs (one lane per pair), setup (one wave per
 *   image: D, D^-1, b, the warm-started r, z, p, its partial of r.z) and, budget times, operator (one wave per image: q and its partial of p.q) and step (ONE
 *   workgroup: the dots, alpha, beta, x, r, z, p, the record, and the stage's update when the solve ends); last one lane writes summary 6 and 8 .. 11.
 *   9 + 2 n (2 + rotation_cg_iterations + position_cg_iterations) in all. */
typedef struct lg_posegraph_pcg_io {
    lg_posegraph_io base;                  /* base.workspace: lg_posegraph_pcg_workspace_bytes; base.summary: [12]    */
    int32_t rotation_cg_iterations;        /* per rotation iteration, in [1, LG_BA_PCG_MAX_CG_ITERATIONS]             */
    int32_t position_cg_iterations;        /* per position iteration, in [1, LG_BA_PCG_MAX_CG_ITERATIONS]             */
    double cg_tolerance;                   /* in (0, 1)                                                               */
} lg_posegraph_pcg_io;
int64_t lg_posegraph_pcg_workspace_bytes(int64_t images, int64_t pairs, uint32_t flags);
/* Enqueue the whole call on `hip_stream`: asynchronous, no allocation, no host synchronisation. */
int lg_posegraph_solve_pcg(const lg_posegraph_pcg_io* io, void* hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Global positioning: the camera centres of the free images and the points of all tracks, solved jointly from the viewing rays of every observation, with
 * the rotations kept as they come in (from lg_posegraph_solve, say) and at least two images held to fix origin, orientation and scale.  It replaces the
 * positions that averaging the pairs' translation directions gives: a track ties many rays to one point, a pair carries one direction.  The points come with
 * it, so lg_bundle_adjust can start from (track_id_out, xyz) directly.  fp64 throughout, no fused multiply-add, dense Cholesky, one call and one host
 * synchronisation.  Stateless.  The reference has no such step; this is the definition (tests/positioning_oracle.py restates it in float64 numpy).
 * History: added to ABI 0.6 without a version bump; the addition is backward compatible (no existing struct, flag, refusal or formula changed).
 *   nodes     as in the triangulator: node v = k n + i, live iff i < num[k] (num NULL: n; clamped into [0, n]).
 *   images    image k PASSES iff cameras[k] passes the camera rule and the 9 entries of its rotation (poses[k], columns 0 .. 2) are finite; a HELD image
 *             (constant_pose[k] != 0) also needs its 3 translation entries finite.  The translation of an image that is not held is not read.  status[k] is
 *             LG_ERR_CAMERA for an image that does not pass, else LG_OK.  A held image's centre is c = -(R^T t), each entry -((R0e t0 + R1e t1) + R2e t2).
 *   gauge     at least two held images must pass and their centres must not all be equal; otherwise nothing is solved (summary[5] = 0: the Python layer
 *             raises).  They fix origin, orientation and scale.
 *   ray       of node (k, i): u = ((x - cx) / fx, (y - cy) / fy, 1) from the float32 inputs widened, w = R_k^T u, entry e: (R0e ux + R1e uy) + R2e, and
 *             v = w / |w|, |w| = sqrt((w0 w0 + w1 w1) + w2 w2): the length is taken of the ROTATED vector, as the triangulator does, because a float32 R is
 *             orthonormal to 1e-7 only and I - v v^T must be a projection (parallel rays must fail the 3 x 3 pivot).  R is NOT re-orthonormalised.
 *   candidates  node (k, i) with j = track_id[k][i] is a candidate observation of track j iff i < num[k], 0 <= j < tracks and image k passes.  Two rows of one
 *             image in one track are two observations.  A track with more than LG_BA_MAX_TRACK_LENGTH candidates is left out.  A track's observations are
 *             ordered by ascending node.
 *   who takes part  start from all candidates of the tracks with 2 .. LG_BA_MAX_TRACK_LENGTH of them and all images that pass; repeat until nothing changes:
 *             a track leaves if it has observations in fewer than two DIFFERENT images still there; an image that is not held leaves if it has observations
 *             in fewer than two different tracks still there.  (Removal is monotone: what is left does not depend on the order of the removals.)  Then the
 *             images and tracks that no chain of shared observations joins to a held image leave as "not connected".  An image that takes part and is not
 *             held is FREE.
 *   cost      the sum of rho |(I - v v^T)(X_j - c_k)|^2 over the observations taking part, solved by num_iterations steps of reweighted LINEAR least squares
 *             in all free centres and all points at once.  Iteration 0: rho = 1 (no initial centres or points are needed).  Later, with e = X_j - c_k of the
 *             previous iterate: rho = (1 / max(|e|^2, 1e-12)) / (1 + (phi / s)^2), phi = atan2(|e - (v . e) v|, v . e), s = angle_scale max(1, 2^(n - 6 - it))
 *             (the position stage's schedule and depth weight in lg_posegraph_solve, for the same reason: the cost must not shrink the scene).
 *   system    M = rho (I - v v^T) per observation, entries rho (1 - v0 v0), rho (0 - v0 v1), ...  Per track: V_j = sum of M, g_j = sum over its observations in
 *             HELD images of M c_k (rows (m0 c0 + m1 c1) + m2 c2), in list order; Vi_j column c = the solution of V_j x = e_c by the triangulator's 3 x 3
 *             elimination and pivot rule.  A failed pivot takes the track out for the rest of the call (node_state 6).  Reduced system over the free centres,
 *             3 images x 3 images of 3 x 3 blocks, lower block triangle: for free a and free b <= a, E_ab = sum over the rows i of image a in ascending order
 *             whose observation takes part, and for each over the observations (b, i') of the same track in list order, of Y M_(b,i') with Y = M_(a,i) Vi_j
 *             (Y[r][m] = (M[r][0] Vi[0][m] + M[r][1] Vi[1][m]) + M[r][2] Vi[2][m]; entry (r, c): (Y[r][0] Mb[0][c] + Y[r][1] Mb[1][c]) + Y[r][2] Mb[2][c]);
 *             S_ab = -E_ab, S_aa = U_a - E_aa with U_a = sum of M over the same rows; right-hand side of a = sum over the same rows of Y g_j.  These three
 *             sums over the rows of image a run in GROUPS of G consecutive rows, G = half the smallest power of two >= max(images, 2): a group's terms are
 *             added in ascending row order starting from zero, and the groups' sums are added to the total in ascending order (with few images a
 *             workgroup shares the rows out over its lanes; the order stays a function of position alone).  Every other image: identity rows and columns,
 *             zero right-hand side.
 *   Cholesky  lg_posegraph_solve's: the bundle adjuster's blocked factorisation with one right-hand-side row and the pivot floor 1e-10 x the diagonal entry.
 *             A failed pivot of ANY iteration clears positions_ok: no free image gets a centre (image_state 5) and no point is returned (node_state 9).
 *   points    X_j = Vi_j (g_j + sum over its observations in free images, in list order, of M c_k) with the NEW centres and this iteration's M.
 *   stopping  num_iterations is a fixed budget, every launch is enqueued unconditionally; the stage ends after an iteration with s = angle_scale, every
 *             step finite and max |c_new - c_old| < 1e-12 (that iteration's points are still formed); later launches return at once.
 *   final state  per observation taking part: angle_error = phi in degrees at the final centres and points; it is an OUTLIER (node_state 7) iff not
 *             (v . e > 0 and phi <= max_angle_error).  No solve follows.  A track left with inlier observations in fewer than two different images has no
 *             point (those nodes: 8).
 *   node_state  0 not labelled; 1 inlier observation; 2 bad image; 3 a candidate of a track with more than LG_BA_MAX_TRACK_LENGTH; 4 peeled (its track has
 *             fewer than 2 candidates, or its track or image left in the peeling); 5 not connected; 6 its track's 3 x 3 pivot failed; 7 outlier; 8 inlier of a
 *             track without a point; 9 no solution (a Cholesky pivot failed).
 *   image_state  0 posed (free, with a centre); 1 held; 2 too few tracks (peeled); 3 not connected; 4 bad image; 5 no solution.
 *   outputs   poses_out [images][12]: R the input's bits; t = -(R c) rounded to float32 once for a posed image, the input's bits for a held one, NaN for states
 *             2, 3, 5; all twelve NaN for a bad image.  xyz [tracks][3] rounded once, NaN for a track without a point.  points3d [images][n][3] the point and
 *             track_id_out [images][n] the input label at every inlier observation, NaN / -1 elsewhere (labels are not renumbered).  angle_error [images][n],
 *             NaN where not evaluated.  summary [8] fp64: images with a pose (held or posed), tracks with a point, outlier observations, iterations run,
 *             positions_ok, gauge ok, tracks whose 3 x 3 pivot failed, 0.
 *   Determinism: no floating-point atomics; every sum is a fixed function of position (a track's list in ascending node order, an image's rows ascending,
 *             images ascending), so every output is the same bits from run to run and under any relabelling of the tracks.  An image that does not pass
 *             takes its observations out and leaves everything else bit for bit.
 * Workspace: lg_positioning_workspace_bytes bytes (below; -1 outside the envelope), 256-byte aligned: a 256-byte record; 180 bytes per image; the system with
 *   its right-hand side row, (3 images + 1) x 3 images fp64 (4.7 MB at 256 images); 40 bytes per node (list entry, its image, ray, rho); 140 bytes per track.
 * Envelope (LG_ERR_INVALID with a message before the GPU is touched): null io; any flag bit (none is defined); n above LG_MAX_KEYPOINTS; images outside
 *   [2, LG_BA_MAX_IMAGES]; images x n above LG_MAX_ROWS; tracks outside [0, images x n / 2]; num_iterations outside [LG_PG_MIN_ITERATIONS,
 *   LG_BA_MAX_ITERATIONS]; angle_scale or max_angle_error not finite and > 0; a null required pointer; a workspace too small or not 256-byte aligned.
 * Launches, none of which waits on another workgroup: records; candidates and rays (count); one scan over the tracks; fill; sort (one lane per track); who
 *   takes part (ONE workgroup); per iteration points (one lane per track), reduce (one workgroup per image: its block row), two per Cholesky panel, centres
 *   (ONE workgroup), point update (one lane per track); classify (one lane per track); output.  8 + n (4 + 2 ceil(3 images / 48)) in all. */
typedef struct lg_positioning_io {
    int32_t n, images, tracks;
    uint32_t flags;                        /* none defined: must be 0                                                 */
    int32_t num_iterations;                /* in [LG_PG_MIN_ITERATIONS, LG_BA_MAX_ITERATIONS]                         */
    double angle_scale;                    /* degrees, > 0                                                            */
    double max_angle_error;                /* degrees, > 0                                                            */
    const float *kpts;                     /* [images][n][2], read in place                                           */
    const int32_t *num;                    /* [images] live rows, or NULL = n                                         */
    const int64_t *track_id;               /* [images][n]: the triangulator's labels                                  */
    const float *cameras;                  /* [images][4]: (fx, fy, cx, cy)                                           */
    const float *poses;                    /* [images][12]: (R | t) row-major 3 x 4; t is read for held images only   */
    const uint8_t *constant_pose;          /* [images]: non-zero = the image is held                                  */
    void *workspace; int64_t workspace_bytes;
    float *poses_out;                      /* [images][12]                                                            */
    float *xyz;                            /* [tracks][3]                                                             */
    float *points3d;                       /* [images][n][3]                                                          */
    int64_t *track_id_out;                 /* [images][n]                                                             */
    uint8_t *node_state;                   /* [images][n]                                                             */
    uint8_t *image_state;                  /* [images]                                                                */
    float *angle_error;                    /* [images][n] degrees                                                     */
    double *summary;                       /* [8]                                                                     */
    int32_t *status;                       /* [images] LG_OK / LG_ERR_CAMERA                                          */
} lg_positioning_io;
int64_t lg_positioning_workspace_bytes(int64_t images, int32_t n, int64_t tracks, uint32_t flags);
/* Enqueue the whole call on `hip_stream`: asynchronous, no allocation, no host synchronisation. */
int lg_positioning_solve(const lg_positioning_io* io, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTGLUE_AMD_H */
