// lightglue_amd — the algorithms both keypoint extractors run (SuperPoint: lg_sp_encoder.hip, lg_superpoint.hip; ALIKED: lg_aliked.hip),
// implemented once in lg_extract.hip: the exact-fp32 implicit-GEMM convolution, the weight repack, simple_nms, threshold + raster-order
// compaction and the top-K selection.
#pragma once
#include "lg_host_call.h"     // Bump: workspace carving
#include "lg_kernels.h"
#include "../../include/lightglue_amd.h"

namespace lg {

// ---------------------------------------------------------------- convolution
// Implicit GEMM on NHWC activations, C[pixel][cout] = sum_{tap, cin} A[pixel + tap][cin] W[tap][cout][cin] (exact fp32, v_mfma_f32_16x16x4_f32):
//   * one MFMA "chunk" = 16 input channels: lane (lr, g) supplies pixel lr / cout lr and the 4 consecutive channels 4g .. 4g + 3 -> ONE 16-byte
//     load per fragment for both operands (weights are repacked [tap][cout][cin] once, launch_fold);
//   * wave = 2 image rows x 32 pixels x 16 NT output channels (NT = 1, 2, 4 from Cout: the 16-channel layers of ALIKED do not run 48 dead
//     output columns), workgroup = 4 waves = 8 rows: the 9 taps re-read the same input lines from L1 / L2, nothing is staged through LDS;
//   * zero padding = clamped address + select; bias / activation / the 2x2 max-pool run on the accumulators (a lane holds 4 horizontally
//     consecutive pixels of one channel and both rows of the pool window).
// The split-f16 kernels of lg_sp_encoder.hip take the same arguments (w then holds their packing) and end in the same epilogue.
enum : int { ACT_NONE = 0, ACT_RELU = 1, ACT_SELU = 2 };
struct ConvArgs {
    const float* in; const void* w; const float* bias;   // in [B][H][W][Cin]; w [taps][Cout][Cin] fp32; bias [Cout] or null
    const float* in2; const float* w2;                   // optional extra K at the centre pixel (ResBlock downsample): in2 [B][H][W][Cin2], w2 [Cout][Cin2]
    float* out;                                          // [B][H][W][Cout]; pool: [B][H/2][W/2][Cout]; out_nchw: [B][Cout][H][W]
    int B, H, W, Cin, Cin2, Cout, taps;                  // taps 9 (3 x 3, zero pad 1) or 1
    int act, pool, out_nchw;
};
void launch_conv(const ConvArgs& a, hipStream_t s);      // exact fp32; Cin % 16 == 0

// Ragged batch: H, W are the CANVAS of this pyramid level and give every address and stride; image b occupies its top-left
// (sizes[2b + 1] >> size_shift) x (sizes[2b] >> size_shift) corner and gives every bound (padding select, stores, pool).  A struct of its own, taken by the RAGGED
// instances of the convolution kernels only: the uniform instances keep ConvArgs as their kernel argument and compile to the code they were (a larger
// argument block alone changes how the compiler groups their scalar loads).
struct RaggedConvArgs : ConvArgs {
    const int* sizes; int size_shift;                    // [B][2] (w, h) at full resolution; the level's repeated floor halving
};
void launch_conv(const RaggedConvArgs& a, hipStream_t s);
template <class A> inline constexpr bool is_ragged = false;
template <> inline constexpr bool is_ragged<RaggedConvArgs> = true;

// The extent (rows, columns) the bounds of image b are taken from: a.H / a.W read where they always were (uniform), or the image's, clamped to [1, canvas] —
// a bad size cannot address outside a buffer (validation proper is the caller's, who has the sizes as host integers).
struct ConvExtent { int h, w; };
template <class A> __device__ __forceinline__ ConvExtent conv_extent(const A& a, int b) {
    if constexpr (is_ragged<A>) return {min(max(a.sizes[2 * b + 1] >> a.size_shift, 1), a.H), min(max(a.sizes[2 * b] >> a.size_shift, 1), a.W)};
    else return {0, 0};      // (never read)
}
template <bool RAGGED> __device__ __forceinline__ int ext_h(const ConvArgs& a, const ConvExtent& e) { if constexpr (RAGGED) return e.h; else return a.H; }
template <bool RAGGED> __device__ __forceinline__ int ext_w(const ConvArgs& a, const ConvExtent& e) { if constexpr (RAGGED) return e.w; else return a.W; }

constexpr float SELU_ALPHA = 1.6732632423543772848170429916717f, SELU_SCALE = 1.0507009873554804934193349852946f;
__device__ __forceinline__ float selu(float x) { return SELU_SCALE * (x > 0.f ? x : SELU_ALPHA * expm1f(x)); }

// bias / activation / 2x2 max-pool / stores of one wave's 2 rows x 32 pixels x 16 NT output channels, straight from the accumulators:
// acc[mt][nt][r] = out[pixel (y0 + mt / 2, x0 + (mt & 1) * 16 + 4g + r)][cout n0 + nt * 16 + lr]
// Strides come from a.H / a.W (the canvas), bounds from the image extent `e` (RAGGED) — the same a.H / a.W otherwise.
template <int NT, bool RAGGED = false>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, f32x4 (&acc)[4][NT], int b, int n0, int x0, int y0, int lr, int g, const ConvExtent& e = ConvExtent{0, 0}) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = n0 + nt * 16 + lr;
        if (co >= a.Cout) continue;
        const float bv = a.bias ? a.bias[co] : 0.f;
        f32x4 v[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            v[mt] = acc[mt][nt] + bv;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[mt][r] = a.act == ACT_RELU ? fmaxf(v[mt][r], 0.f) : (a.act == ACT_SELU ? selu(v[mt][r]) : v[mt][r]);
        }
        if (a.pool) {        // 2x2 max-pool (SuperPoint): rows y0, y0 + 1; columns (4g, 4g + 1), (4g + 2, 4g + 3)
            const int H2 = a.H >> 1, W2 = a.W >> 1, yo = y0 >> 1;
            const int H2i = ext_h<RAGGED>(a, e) >> 1, W2i = ext_w<RAGGED>(a, e) >> 1;       // pooled bounds: the image's; pooled strides: the canvas's
            if (yo < H2i) {
#pragma unroll
                for (int xt = 0; xt < 2; ++xt) {
                    const float p0 = fmaxf(fmaxf(v[xt][0], v[xt][1]), fmaxf(v[2 + xt][0], v[2 + xt][1]));
                    const float p1 = fmaxf(fmaxf(v[xt][2], v[xt][3]), fmaxf(v[2 + xt][2], v[2 + xt][3]));
                    const int xo = (x0 + xt * 16 + 4 * g) >> 1;
                    float* o = a.out + (((long long)b * H2 + yo) * W2 + xo) * a.Cout + co;
                    if (xo < W2i) o[0] = p0;
                    if (xo + 1 < W2i) o[a.Cout] = p1;
                }
            }
        } else {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int y = y0 + (mt >> 1), x = x0 + (mt & 1) * 16 + 4 * g;
                if (y >= ext_h<RAGGED>(a, e)) continue;
                if (a.out_nchw) {    // 4 consecutive pixels of one channel: one 16-byte store when the row allows it (alignment: the canvas width)
                    float* o = a.out + (((long long)b * a.Cout + co) * a.H + y) * a.W + x;
                    if (x + 3 < ext_w<RAGGED>(a, e) && (a.W & 3) == 0) *reinterpret_cast<f32x4*>(o) = v[mt];
                    else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) if (x + r < ext_w<RAGGED>(a, e)) o[r] = v[mt][r];
                    }
                } else {
                    float* o = a.out + (((long long)b * a.H + y) * a.W + x) * a.Cout + co;
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (x + r < ext_w<RAGGED>(a, e)) o[(long long)r * a.Cout] = v[mt][r];
                }
            }
        }
    }
}

// ---------------------------------------------------------------- weight repack
// dst = s[co] * src in the layout of `mode`, s = gamma / sqrt(var + 1e-5) with BatchNorm (bn = {gamma, beta, mean, var}, eval), else 1;
// bias_dst[co] = s (cbias - mean) + beta (+ extra) when bias_dst is set.  src [Cout][Cin][kk]; PK_AGG: [n_pos][128][128] -> [128][n_pos * 128]
enum : int { PK_TAP_CO_CI = 0, PK_CO_TAP_CI = 1, PK_TAP_CI_CO = 2, PK_COPY = 3, PK_AGG = 4 };
hipError_t launch_fold(const float* src, float* dst, float* bias_dst, int Cout, int Cin, int kk, int mode, const float* const* bn, const float* cbias,
                       const float* extra, hipStream_t s);

// ---------------------------------------------------------------- keypoint detection on a dense score map
// simple_nms (superpoint.py / aliked.py: three rounds of (2r+1)^2 max-pooling with equality tests), border, threshold, raster-order compaction
// (the order of torch.where / nonzero) and the selection of the K best.  All comparisons are exact.
struct DetectArgs {
    const float* S;                    // [B][H][W] scores
    int B, H, W, radius;               // NMS radius <= 8
    unsigned char* mask_a; unsigned char* mask_b;   // [B][H][W] workspace
    float* nms;                        // [B][H][W]: S at the NMS maxima, 0 elsewhere
    // the thresholded value: border_value within `border` pixels of the top / left edges and of the far ones (image_size [B][2] (w, h),
    // truncated like .long(), else H / W), nms elsewhere
    int border; const float* image_size; float border_value;
    float threshold;                   // a per-image array th[b] replaces it where the kernels are given one
    int* row_counts;                   // [B][H] pixels above the threshold
    int max_candidates;                // candidate rows per image (hits beyond are dropped; cand_total keeps counting)
    int* cand_idx; float* cand_score; int* cand_total;   // [B][max_candidates] raster index y W + x and value, [B] hits
    int K, sort_always;                // keep the K best (K <= 0: all); ordered by score when that limited the set, or always
    int sel_cap; int* sel; unsigned* sel_key;        // [B][sel_cap] kept candidates in raster order and their keys
    // ragged batch (null: every map fills H x W): H, W are the CANVAS (addresses, strides, the raster index y W + x); the score map of image b is its top-left
    // sizes[2b + 1] x sizes[2b] corner ([B][2] (w, h) of the SCORE maps: SuperPoint passes whole 8 x 8 cells, (h_b >> 3) << 3).  Outside it a pixel is max_pool2d's
    // -inf padding: never a maximum, never in supp_mask, never above the threshold; the far borders are that corner's.
    const int* sizes;
};

// rows / columns of image b's score map: the bound of every detection kernel (clamped into the canvas; H x W when the batch is uniform)
struct DetectExtent { int h, w; };
__device__ __forceinline__ DetectExtent detect_extent(const DetectArgs& a, int b) {
    if (!a.sizes) return {a.H, a.W};
    return {min(max(a.sizes[2 * b + 1], 0), a.H), min(max(a.sizes[2 * b], 0), a.W)};
}

// the workspace of one detection, carved from one buffer; rowsum / th only with `stats` (ALIKED's mean fallback)
struct DetectLayout { long long mask_a, mask_b, nms, rows, rowsum, th, cidx, cscore, ctotal, sel, selkey, total; };
DetectLayout detect_layout(int B, int H, int W, int max_candidates, int sel_cap, bool stats);
void detect_bind(DetectArgs& a, const DetectLayout& L, void* ws);   // the workspace pointers of `a`

void launch_nms(const DetectArgs& a, hipStream_t s);                                         // S -> nms (mask_a, mask_b as scratch)
void launch_row_count(const DetectArgs& a, const float* th, double* rowsum, hipStream_t s);  // rowsum (optional): [B][H] row sums of S over the image's own columns, 0 below the image
void launch_compact(const DetectArgs& a, const float* th, hipStream_t s);
void launch_select(const DetectArgs& a, hipStream_t s);

// entries the selection kept for image b, and whether their output order is by score
__device__ __forceinline__ int selected_count(const DetectArgs& a, int b) {
    const int total = min(a.cand_total[b], a.max_candidates);
    return min(a.K > 0 ? min(total, a.K) : total, a.sel_cap);
}
__device__ __forceinline__ bool selection_sorted(const DetectArgs& a, int b) {
    return a.sort_always || (a.K > 0 && min(a.cand_total[b], a.max_candidates) > a.K);
}
// output slot of kept entry j among n: score descending, the lower raster index first among equal keys.  The block streams the key list
// through LDS together (every thread reads each key as a broadcast), so every thread of the block calls it; slots j >= n get no rank.
__device__ __forceinline__ int selected_rank(const unsigned* key, int n, int j) {
    __shared__ unsigned tile[1024];
    const unsigned k = j < n ? key[j] : 0u;
    int rank = 0;
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int m = min(1024, n - i0);
        __syncthreads();
        for (int t = threadIdx.x; t < m; t += blockDim.x) tile[t] = key[i0 + t];
        __syncthreads();
        for (int t = 0; t < m; ++t) { const unsigned q = tile[t]; rank += (q > k) || (q == k && i0 + t < j); }
    }
    return rank;
}

inline unsigned blocks(long long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

// ---------------------------------------------------------------- the io struct of an extractor stage (include/lightglue_amd.h: lg_*_io)
// The refusals all six stages share, made before a field other than `flags` and `sizes` is looked at: a null io, a flag bit outside `defined`, and
// LG_EXTRACT_RAGGED without `sizes`.
template <class IO> int check_extract_io(const IO* io, uint32_t defined, const char* stage) {
    if (!io) return set_error(LG_ERR_INVALID, std::string(stage) + ": null io");
    if (io->flags & ~defined) return set_error(LG_ERR_INVALID, std::string(stage) + ": a flag bit this stage does not define (LG_EXTRACT_*)");
    if ((io->flags & LG_EXTRACT_RAGGED) && !io->sizes) return set_error(LG_ERR_INVALID, "null pointer");
    return LG_OK;
}
// `sizes` is read only with the flag: null means a uniform batch everywhere below the entry points
template <class IO> const int32_t* extract_sizes(const IO& io) { return (io.flags & LG_EXTRACT_RAGGED) ? io.sizes : nullptr; }

}  // namespace lg
