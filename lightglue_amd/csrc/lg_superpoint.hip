// lightglue_amd — SuperPoint descriptor head: the step that PRODUCES the matcher's
// [B, N, 256] descriptor tensors from the dense descriptor map (ref superpoint.py:80-95
// sample_descriptors, :216-228 dense L2 normalisation + per-keypoint sampling + transpose).
// HBM-bound gather work, two kernels:
//   sp_dense_kernel   reads the NCHW map once (coalesced along w), optionally L2-normalises every
//                     location over its 256 channels (ref :218 F.normalize(dim=1)) and writes it
//                     location-major (NHWC) through an LDS tile — the transposition the reference
//                     leaves to grid_sample's strided reads.  Algorithmic bytes: 2 * 4 * C * h * w.
//   sp_sample_kernel  one wave per keypoint: bilinear interpolation of the 4 neighbouring locations
//                     (align_corners=True, zero padding: ref :85-91 + grid_sample), each a contiguous
//                     1 KB row of the NHWC map, then the final L2 normalisation (ref :92-94); writes
//                     [B][N][C] directly (the layout ref :228 transposes to), as fp32 or as binary16.
//                     Algorithmic bytes per keypoint: 4 * 1 KB read + 1 KB written.
#include <string>

#include "lg_extract.h"
#include "../../include/lightglue_amd.h"

namespace lg {

struct SpArgs {
    const float* desc_map;     // [B][256][h][w] dense descriptor map (NCHW, as the conv stack leaves it)
    float* nhwc;               // [B][h][w][256] workspace: (normalised) location-major copy
    const float* keypoints;    // [B][N][2] pixel (x, y)
    const int* num;            // [B] live keypoints per image or nullptr
    float* out;                // [B][N][256]
    int B, h, w, N, s, normalize_dense;
    int out_f16;               // != 0: `out` holds binary16 rows (LG_EXTRACT_DESC_F16): the fp32 result rounded once, to nearest even, on store
    const int* sizes;          // ragged batch (else null): [B][2] image (w, h); h, w above are then the CANVAS map (strides), the map of image b its top-left (h_b / s) x (w_b / s) corner
};

// rows / columns of image b's descriptor map: the grid normalisation and every bound (clamped into the canvas; h x w when the batch is uniform)
__device__ __forceinline__ void sp_map_extent(const SpArgs& a, int b, int& h, int& w) {
    h = a.h; w = a.w;
    if (a.sizes) { h = min(max(a.sizes[2 * b + 1] / a.s, 1), a.h); w = min(max(a.sizes[2 * b] / a.s, 1), a.w); }
}

constexpr int SPC = 256;   // descriptor_dim of SuperPoint (ref superpoint.py:107)
constexpr int SPT = 32;    // locations per workgroup tile (32 x 257 floats of LDS)

__global__ __launch_bounds__(256) void sp_dense_kernel(SpArgs a) {
    __shared__ float tile[SPT][SPC + 1];
    __shared__ float part[8][SPT];
    const int b = blockIdx.y, loc0 = blockIdx.x * SPT, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hw = a.h * a.w, l = lane & 31, half = lane >> 5, loc = loc0 + l;
    int hi, wi;
    sp_map_extent(a, b, hi, wi);
    auto live = [&](int p) { return p < hw && (!a.sizes || (p / a.w < hi && p % a.w < wi)); };     // the canvas outside an image is neither read nor written
    const bool in = live(loc);
    const float* src = a.desc_map + (long long)b * SPC * hw;
    float ss = 0.f;
    for (int c = wave * 2 + half; c < SPC; c += 8) {     // half-wave reads 32 consecutive locations (128 B) of one channel
        const float v = in ? src[(long long)c * hw + loc] : 0.f;
        tile[l][c] = v;
        ss += v * v;
    }
    part[wave * 2 + half][l] = ss;
    __syncthreads();
    float* dst = a.nhwc + ((long long)b * hw + loc0) * SPC;
    for (int r = wave; r < SPT; r += 4) {                // wave writes one location = 1 KB contiguous
        if (loc0 + r >= hw) break;
        if (!live(loc0 + r)) continue;
        float inv = 1.f;
        if (a.normalize_dense) {                         // F.normalize: x / max(||x||_2, 1e-12)
            float q = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) q += part[k][r];
            inv = 1.f / fmaxf(sqrtf(q), 1e-12f);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[(long long)r * SPC + lane + 64 * k] = tile[r][lane + 64 * k] * inv;
    }
}

__global__ __launch_bounds__(256) void sp_sample_kernel(SpArgs a) {
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wave;
    const int n = a.num ? min(max(a.num[b], 0), a.N) : a.N;
    if (i >= a.N) return;
    const long long o = ((long long)b * a.N + i) * SPC + lane * 4;
    auto store = [&](const f32x4& v) {
        if (a.out_f16) *reinterpret_cast<f16x4*>(reinterpret_cast<f16_t*>(a.out) + o) = f16x4{(f16_t)v[0], (f16_t)v[1], (f16_t)v[2], (f16_t)v[3]};
        else *reinterpret_cast<f32x4*>(a.out + o) = v;
    };
    if (i >= n) { store(f32x4{0.f, 0.f, 0.f, 0.f}); return; }   // padding row of a ragged batch
    const float* kp = a.keypoints + ((long long)b * a.N + i) * 2;
    const float s = (float)a.s;
    int hi, wi;
    sp_map_extent(a, b, hi, wi);
    // ref :83-90: (k - s/2 + 0.5) / (w*s - s/2 - 0.5) in [0,1], *2-1, then align_corners=True un-normalisation
    // ((g + 1) / 2 * (w - 1)), evaluated in the reference's order
    const float gx = (kp[0] - s / 2.f + 0.5f) / ((float)wi * s - s / 2.f - 0.5f) * 2.f - 1.f;
    const float gy = (kp[1] - s / 2.f + 0.5f) / ((float)hi * s - s / 2.f - 0.5f) * 2.f - 1.f;
    const float ix = (gx + 1.f) / 2.f * (float)(wi - 1), iy = (gy + 1.f) / 2.f * (float)(hi - 1);
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float tx = ix - fx, ty = iy - fy;
    const float wgt[4] = {(1.f - tx) * (1.f - ty), tx * (1.f - ty), (1.f - tx) * ty, tx * ty};   // nw ne sw se
    const float* map = a.nhwc + (long long)b * a.h * a.w * SPC + lane * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + (k & 1), y = y0 + (k >> 1);
        if (x >= 0 && x < wi && y >= 0 && y < hi) {      // padding_mode="zeros"
            const f32x4 v = *reinterpret_cast<const f32x4*>(map + ((long long)y * a.w + x) * SPC);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] += v[c] * wgt[k];
        }
    }
    const float nrm = sqrtf(wave_sum(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2] + acc[3] * acc[3]));
    const float inv = 1.f / fmaxf(nrm, 1e-12f);          // ref :92-94
    store(f32x4{acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv});
}

static hipError_t launch_sp_sample(const SpArgs& a, hipStream_t s) {
    const int hw = a.h * a.w;
    hipLaunchKernelGGL(sp_dense_kernel, dim3((hw + SPT - 1) / SPT, a.B), dim3(256), 0, s, a);
    if (a.N > 0) hipLaunchKernelGGL(sp_sample_kernel, dim3((a.N + 3) / 4, a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace lg

// ====================================================================================================================
// Keypoint extraction: non-maximum suppression of the dense score map (ref superpoint.py:52-70 simple_nms),
// border removal (:189-194: the border reads -1), thresholding and row-major compaction (:197-204, the order torch.where produces),
// optional top-k by score (:207-215, top_k_keypoints :73-77) and the (y, x) -> (x, y) float conversion (:218), on the detection
// kernels of lg_extract.hip.  All comparisons are exact, so the result is bit-identical to the reference's (ties inside top-k,
// which torch leaves unspecified, break towards the lower row-major index).
namespace lg {

constexpr int SP_TOPK_MAX = 4096;   // the largest max_keypoints lg_sp_detect accepts (include/lightglue_amd.h)

struct SpDetectArgs {
    DetectArgs d;
    int capacity;              // rows of the outputs per image
    float* keypoints; float* kp_scores; int* counts;    // [B][capacity][2] (x, y), [B][capacity], [B]
    int* totals;               // optional [B]: pixels above the threshold before top-k / capacity clipping
};

// kept entry j -> its output row: (x, y) and score; counts and totals.  Raster order, or by score after a top-k.  grid (capacity / 256, B)
__global__ __launch_bounds__(256) void sp_keypoints_kernel(SpDetectArgs a) {
    const DetectArgs& d = a.d;
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const int n = selected_count(d, b);
    const long long ob = (long long)b * d.sel_cap;
    const int rank = selection_sorted(d, b) && (int)blockIdx.x * 256 < n ? selected_rank(d.sel_key + ob, n, j) : j;   // (block-uniform)
    if (j == 0) { a.counts[b] = min(n, a.capacity); if (a.totals) a.totals[b] = d.cand_total[b]; }
    if (j >= n || rank >= a.capacity) return;
    const long long c = (long long)b * d.max_candidates + d.sel[ob + j];
    const int p = d.cand_idx[c], y = p / d.W, x = p - y * d.W;
    const long long o = (long long)b * a.capacity + rank;
    a.keypoints[2 * o] = (float)x; a.keypoints[2 * o + 1] = (float)y;
    a.kp_scores[o] = d.cand_score[c];
}

static hipError_t launch_sp_detect(const SpDetectArgs& a, hipStream_t s) {
    launch_nms(a.d, s);
    launch_row_count(a.d, nullptr, nullptr, s);
    launch_compact(a.d, nullptr, s);
    launch_select(a.d, s);
    hipLaunchKernelGGL(sp_keypoints_kernel, dim3(blocks(a.capacity), a.d.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace lg

using namespace lg;

extern "C" {

// LG_EXTRACT_DESC_F16: the element type of `out`, decided at the last kernel's store
int lg_sp_sample_descriptors(const lg_sp_sample_io* io, void* hip_stream) {
    if (int rc = check_extract_io(io, LG_EXTRACT_RAGGED | LG_EXTRACT_DESC_F16, "lg_sp_sample_descriptors")) return rc;
    const lg_sp_sample_io& i = *io;
    if (i.channels != 256) return set_error(LG_ERR_INVALID, "descriptor map must have 256 channels");
    if (i.batch < 1 || i.h < 1 || i.w < 1 || i.n < 0 || i.cell < 1) return set_error(LG_ERR_INVALID, "bad descriptor map / keypoint sizes");
    if (!i.desc_map || !i.workspace || (i.n && (!i.keypoints || !i.out))) return set_error(LG_ERR_INVALID, "null pointer");
    SpArgs a{i.desc_map, i.workspace, i.keypoints, i.num, static_cast<float*>(i.out), i.batch, i.h, i.w, i.n, i.cell, i.normalize_dense ? 1 : 0,
             (i.flags & LG_EXTRACT_DESC_F16) ? 1 : 0, extract_sizes(i)};
    HIPCHK(launch_sp_sample(a, static_cast<hipStream_t>(hip_stream)));
    return LG_OK;
}

int64_t lg_sp_detect_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t max_candidates) {
    if (batch < 1 || h < 1 || w < 1 || max_candidates < 1) return 0;
    return (int64_t)detect_layout(batch, h, w, max_candidates, max_candidates, false).total;
}

// LG_EXTRACT_RAGGED: sizes (else null: every map fills h x w) are the score maps' (w, h) inside the h x w canvas
int lg_sp_detect(const lg_sp_detect_io* io, void* hip_stream) {
    if (int rc = check_extract_io(io, LG_EXTRACT_RAGGED, "lg_sp_detect")) return rc;
    const lg_sp_detect_io& i = *io;
    if ((i.flags & LG_EXTRACT_RAGGED) && (i.h < 8 || i.w < 8)) return set_error(LG_ERR_INVALID, "score canvas height / width must be at least 8");
    if (i.batch < 1 || i.h < 1 || i.w < 1 || i.h >= 32768 || i.w >= 32768) return set_error(LG_ERR_INVALID, "bad score map size");
    if (i.nms_radius < 0 || i.nms_radius > 4) return set_error(LG_ERR_INVALID, "nms_radius must be in [0, 4]");
    if (i.max_keypoints > SP_TOPK_MAX) return set_error(LG_ERR_INVALID, "max_keypoints above 4096");
    if (i.capacity < 1 || i.max_candidates < 1 || (i.max_keypoints > 0 && i.capacity < i.max_keypoints)) return set_error(LG_ERR_INVALID, "bad capacity / max_candidates");
    if (!i.scores || !i.workspace || !i.keypoints || !i.kp_scores || !i.counts) return set_error(LG_ERR_INVALID, "null pointer");
    const DetectLayout l = detect_layout(i.batch, i.h, i.w, i.max_candidates, i.max_candidates, false);
    if (i.workspace_bytes < (int64_t)l.total) return set_error(LG_ERR_INVALID, "workspace too small (lg_sp_detect_workspace_bytes)");
    SpDetectArgs a{};
    DetectArgs& d = a.d;
    detect_bind(d, l, i.workspace);
    d.S = i.scores; d.B = i.batch; d.H = i.h; d.W = i.w; d.radius = i.nms_radius;
    d.border = i.remove_borders; d.image_size = nullptr; d.border_value = -1.f; d.threshold = i.detection_threshold;
    d.max_candidates = i.max_candidates; d.K = i.max_keypoints; d.sort_always = 0; d.sel_cap = i.max_candidates;
    d.sizes = extract_sizes(i);
    a.capacity = i.capacity; a.keypoints = i.keypoints; a.kp_scores = i.kp_scores; a.counts = i.counts; a.totals = i.totals;
    HIPCHK(launch_sp_detect(a, static_cast<hipStream_t>(hip_stream)));
    return LG_OK;
}

}  // extern "C"
