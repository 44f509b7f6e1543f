// lightglue_amd — ImagePreprocessor (ref lightglue/utils.py:12-38): the resize between a photo and the extractors, as ONE kernel.
//
// Definition (kornia.geometry.transform.resize as the reference calls it: bilinear, optional antialias):
//   1. target size from `resize` (an edge length + side, or an (h, w) pair)                                  -> lg_preprocess_plan (host)
//   2. antialias, when any axis shrinks: separable Gaussian blur, x then y, per-axis sigma = max((factor - 1) / 2, 0.001) and
//      ks = int(max(4 sigma, 3)) made odd, on the image reflect-padded by ks / 2
//   3. bilinear interpolation to the target with ATen's float coordinate rule (scale = float(in) / out; src = max(scale (dst + 0.5f) - 0.5f, 0);
//      i0 = int(src), i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1), evaluated in fp32 WITHOUT contraction so the weights are ATen's own.
//
// Kernel: one workgroup = one TW x TH tile of the OUTPUT, all channels in turn (a channels-last source is then re-read from L1 / L2).
// The bilinear step reads the blurred image at only 2 TW columns (x0 / x1 of every output column) and 2 TH rows, so per channel:
//   source footprint -> LDS (reflect indexing, uint8 -> float(v) / 255.0f, any element strides)        S  [sh][sw]
//   horizontal taps at the 2 TW needed columns of every footprint row                                   Hb [sh][2 TW]
//   vertical taps at the 2 x 2 needed (row, column) pairs of an output + the two lerps                  -> dst, coalesced along x
// The footprint grows with the downscale factor (sw ~ TW * factor + ks), so the host picks the tile shape per plan (pick_tile): the largest
// tile whose LDS stays under 40 KB (4 workgroups per CU), down to 1 x 1 — every plan inside the envelope runs.  No blur and upscaling are
// the same kernel with ks = 1 (weight 1.0: fmaf(v, 1, 0) == v).  A bandwidth kernel: the source is read once from HBM (tile halos from L2).
//
// The tile body is written once (pp_tile) and called by two kernels: the uniform one (a batch of equal images under one plan, the record as its kernel argument)
// and the ragged one (images of different sizes, dtypes and plans into the top-left corners of one canvas: a device table of records, a 1-D grid over all tiles).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "lg_kernels.h"
#include "../../include/lightglue_amd.h"

namespace lg {

constexpr int PP_TAPS = LG_PREPROCESS_MAX_TAPS;
constexpr int PP_THREADS = 256;
constexpr int PP_MLP = 8;            // source loads a thread issues back to back
constexpr int PP_LG_TW_MAX = 6, PP_LG_TH_MAX = 4;   // tiles up to 64 x 16 outputs: threads 0 .. 63 set up the columns, 64 .. 79 the rows
constexpr int PP_LDS_BUDGET = 40 * 1024;
constexpr int PP_OUT_PER_THREAD = (1 << (PP_LG_TW_MAX + PP_LG_TH_MAX)) / PP_THREADS;   // outputs of the largest tile per thread
enum { PP_MODE_SAME = 0, PP_MODE_BROADCAST = 1, PP_MODE_GRAY = 2 };   // source channels -> canvas channels: 1 -> 1 | 3 -> 3, 1 -> 3, 3 -> 1

struct PpArgs {
    const void* src; float* dst;
    long long stride_b; int stride_c, stride_y, stride_x;   // element strides (one image is addressed with 32-bit offsets)
    int u8, C, H, W, Ho, Wo;
    int ksx, ksy, align;
    float scale_x, scale_y;          // ATen's area_pixel_compute_scale
    int lg_tw, lg_th, tiles_x;       // tile = (1 << lg_tw) x (1 << lg_th) outputs
    int sw_max, sh_max, pitch;       // footprint bounds of one tile (host: pick_tile) and the row pitch of S
    float wx[PP_TAPS], wy[PP_TAPS];
    // the ragged kernel's part (one record per image in a device table)
    long long dst_off;               // the image's first plane in the canvas, in elements
    int mode;                        // PP_MODE_*
    int copy;                        // the plan keeps the size: strided copy / conversion
    int tile0;                       // tiles of the images before this one (exclusive prefix)
    int pad_;
};

// ATen's area_pixel_compute_source_index + the index / lambda rule of upsample_bilinear2d for float
__device__ __forceinline__ void src_index(float scale, int dst, int in_size, int align, int& i0, int& i1, float& l1) {
#pragma clang fp contract(off)
    float s;
    if (align) s = scale * (float)dst;
    else {
        const float d = (float)dst + 0.5f;
        const float m = scale * d;
        s = m - 0.5f;
        s = s < 0.f ? 0.f : s;
    }
    i0 = min((int)s, in_size - 1);
    i1 = min(i0 + 1, in_size - 1);
    l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

__device__ __forceinline__ int reflect(int i, int n) {     // torch's reflect padding (pad < n): -1 -> 1, n -> n - 2
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

// The gray value of an RGB pixel as the framework evaluates `0.299 * r + 0.587 * g + 0.114 * b` on float32 tensors: three rounded products, added in
// order, nothing contracted.  One call per channel pass; the partial sum stays in the thread's registers between the passes.
__device__ __forceinline__ float gray_step(float acc, float v, int ch) {
#pragma clang fp contract(off)
    const float p = v * (ch == 0 ? 0.299f : ch == 1 ? 0.587f : 0.114f);
    return ch == 0 ? p : acc + p;
}

// One output tile of one image, all channels in turn: the body of both kernels.  `a`: the image's record (block-uniform), `tile`: the tile's index within the
// image, `src`: the image's first element, `dst`: where the image's first output plane starts, with the destination's row and plane pitches in elements.  RAGGED = false is the uniform kernel:
// channels as they are, every plan through the resize passes.  RAGGED = true reads the channel mode and the copy flag from the record.
template <bool U8, bool RAGGED>
__device__ __forceinline__ void pp_tile(const PpArgs& a, const void* __restrict__ src, int tile, float* __restrict__ dst, int row_pitch, long long plane_pitch) {
    extern __shared__ float smem[];
    const int tid = threadIdx.x;
    const int mode = RAGGED ? a.mode : PP_MODE_SAME;
    const int TW = 1 << a.lg_tw, TH = 1 << a.lg_th;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int ox0 = tx << a.lg_tw, oy0 = ty << a.lg_th;
    const int tw = min(TW, a.Wo - ox0), th = min(TH, a.Ho - oy0);
    // (global address space, stated: a pointer read from the table is generic to the compiler, and its loads would be flat ones)
    const auto* src8 = (const __attribute__((address_space(1))) unsigned char*)src;
    const auto* src32 = (const __attribute__((address_space(1))) float*)src;
    constexpr int kUnroll = RAGGED ? PP_OUT_PER_THREAD : 1;     // gray[q] needs q as a constant; the uniform kernel keeps its rolled output loop (and its register count)
    float gray[PP_OUT_PER_THREAD] = {};    // mode 3 -> 1: the thread owns the same outputs in every channel pass

    // output q of this thread in channel pass ch (q is a compile-time index at every call)
    auto emit = [&](int ch, int q, int oyl, int oxl, float v) {
        const long long at = (long long)(oy0 + oyl) * row_pitch + ox0 + oxl;
        if (mode == PP_MODE_GRAY) {
            gray[q] = gray_step(gray[q], v, ch);
            if (ch == 2) dst[at] = gray[q];
        } else if (mode == PP_MODE_BROADCAST) {
            dst[at] = v; dst[plane_pitch + at] = v; dst[2 * plane_pitch + at] = v;
        } else dst[ch * plane_pitch + at] = v;
    };

    if (RAGGED && a.copy) {             // a plan that keeps the size: a strided copy / conversion, every value as it is (no weights applied)
        for (int ch = 0; ch < a.C; ++ch) {
#pragma unroll
            for (int q = 0; q < PP_OUT_PER_THREAD; ++q) {
                const int i = tid + q * PP_THREADS;
                const int oyl = i >> a.lg_tw, oxl = i & (TW - 1);
                if (oxl >= tw || oyl >= th) continue;
                const int off = ch * a.stride_c + (oy0 + oyl) * a.stride_y + (ox0 + oxl) * a.stride_x;
                emit(ch, q, oyl, oxl, U8 ? (float)src8[off] / 255.0f : src32[off]);
            }
        }
        return;
    }

    float* S = smem;
    float* Hb = S + a.sh_max * a.pitch;
    int* xi = reinterpret_cast<int*>(Hb + a.sh_max * 2 * TW);   // [2 TW]: x0 of every output column, then x1 (relative to the tile's first)
    float* lx = reinterpret_cast<float*>(xi + 2 * TW);          // [TW]
    int* yi = reinterpret_cast<int*>(lx + TW);                  // [2 TH]
    float* ly = reinterpret_cast<float*>(yi + 2 * TH);          // [TH]

    // footprint of the tile (block-uniform): blurred columns fx0 .. last x1, plus ks / 2 on both sides
    int fx0, fy0, lastx, lasty, t; float tl;
    src_index(a.scale_x, ox0, a.W, a.align, fx0, t, tl);
    src_index(a.scale_x, ox0 + tw - 1, a.W, a.align, t, lastx, tl);
    src_index(a.scale_y, oy0, a.H, a.align, fy0, t, tl);
    src_index(a.scale_y, oy0 + th - 1, a.H, a.align, t, lasty, tl);
    const int px = a.ksx >> 1, py = a.ksy >> 1;
    const int nbx = min(lastx - fx0 + 1, a.sw_max - 2 * px), nby = min(lasty - fy0 + 1, a.sh_max - 2 * py);   // (the host bound always holds; the min keeps LDS indices in range regardless)
    const int sw = nbx + 2 * px, sh = nby + 2 * py;
    const int cbase = fx0 - px, rbase = fy0 - py;

    if (tid < tw) {
        int i0, i1; float l1;
        src_index(a.scale_x, ox0 + tid, a.W, a.align, i0, i1, l1);
        xi[tid] = min(i0 - fx0, nbx - 1); xi[TW + tid] = min(i1 - fx0, nbx - 1); lx[tid] = l1;
    } else if (tid >= 64 && tid - 64 < th) {
        int i0, i1; float l1;
        src_index(a.scale_y, oy0 + tid - 64, a.H, a.align, i0, i1, l1);
        yi[tid - 64] = min(i0 - fy0, nby - 1); yi[TH + tid - 64] = min(i1 - fy0, nby - 1); ly[tid - 64] = l1;
    }

    const float inv_sw = 1.f / (float)sw;
    for (int ch = 0; ch < a.C; ++ch) {
        __syncthreads();                      // the previous channel's readers are done (first pass: publishes xi / yi)
        // PP_MLP independent loads per thread in flight before the first LDS store: with one, the kernel ran at the rate Little's law gives 24 waves
        // per CU of 4-byte requests (1.5 TB/s of float32 source, the same TIME for uint8)
        for (int i0 = tid; i0 < sh * sw; i0 += PP_MLP * PP_THREADS) {
            uint32_t raw[PP_MLP]; int at[PP_MLP];
#pragma unroll
            for (int u = 0; u < PP_MLP; ++u) {
                const int i = i0 + u * PP_THREADS;
                int r = (int)((float)i * inv_sw), c = i - r * sw;
                if (c < 0) { --r; c += sw; } else if (c >= sw) { ++r; c -= sw; }
                const int off = ch * a.stride_c + reflect(rbase + r, a.H) * a.stride_y + reflect(cbase + c, a.W) * a.stride_x;
                at[u] = i < sh * sw ? r * a.pitch + c : -1;
                raw[u] = 0u;
                if (at[u] >= 0) raw[u] = U8 ? (uint32_t)src8[off] : __builtin_bit_cast(uint32_t, src32[off]);
            }
#pragma unroll
            for (int u = 0; u < PP_MLP; ++u)
                if (at[u] >= 0) S[at[u]] = U8 ? (float)raw[u] / 255.0f : __builtin_bit_cast(float, raw[u]);
        }
        __syncthreads();
        for (int i = tid; i < (sh << (a.lg_tw + 1)); i += PP_THREADS) {
            const int r = i >> (a.lg_tw + 1), k = i & (2 * TW - 1);
            if ((k & (TW - 1)) >= tw) continue;
            const float* row = S + r * a.pitch + xi[k];
            float acc = 0.f;
            for (int j = 0; j < a.ksx; ++j) acc = fmaf(row[j], a.wx[j], acc);
            Hb[i] = acc;
        }
        __syncthreads();
#pragma unroll kUnroll
        for (int q = 0; q < PP_OUT_PER_THREAD; ++q) {
            const int i = tid + q * PP_THREADS;
            const int oyl = i >> a.lg_tw, oxl = i & (TW - 1);
            if (oxl >= tw || oyl >= th) continue;               // (also every i past the tile: oyl >= TH >= th)
            const float* c0 = Hb + (yi[oyl] << (a.lg_tw + 1)) + oxl;        // rows of y0, column of x0 (x1: + TW)
            const float* c1 = Hb + (yi[TH + oyl] << (a.lg_tw + 1)) + oxl;
            float v00 = 0.f, v01 = 0.f, v10 = 0.f, v11 = 0.f;
            for (int j = 0; j < a.ksy; ++j) {
                const float wj = a.wy[j];
                const int o = j << (a.lg_tw + 1);
                v00 = fmaf(c0[o], wj, v00); v01 = fmaf(c0[o + TW], wj, v01);
                v10 = fmaf(c1[o], wj, v10); v11 = fmaf(c1[o + TW], wj, v11);
            }
            const float l1x = lx[oxl], l0x = 1.f - l1x, l1y = ly[oyl], l0y = 1.f - l1y;
            const float top = v00 * l0x + v01 * l1x, bot = v10 * l0x + v11 * l1x;
            emit(ch, q, oyl, oxl, top * l0y + bot * l1y);
        }
    }
}

template <bool U8>
__global__ __launch_bounds__(PP_THREADS) void pp_resize_kernel(PpArgs a) {
    const int b = blockIdx.y;
    const void* src = U8 ? static_cast<const void*>(static_cast<const unsigned char*>(a.src) + (long long)b * a.stride_b)
                         : static_cast<const void*>(static_cast<const float*>(a.src) + (long long)b * a.stride_b);
    pp_tile<U8, false>(a, src, (int)blockIdx.x, a.dst + (long long)b * a.C * a.Ho * a.Wo, a.Wo, (long long)a.Ho * a.Wo);
}

// The ragged form: one launch, `batch` images of different sizes, plans, dtypes and tile shapes.  The grid holds every image's tiles back to back; a workgroup
// finds its image by bisecting the exclusive prefix of tile counts (block-uniform: the table is read with scalar loads) and writes into the image's plane of the canvas.
__global__ __launch_bounds__(PP_THREADS) void pp_resize_ragged_kernel(const PpArgs* __restrict__ table, int batch, float* __restrict__ canvas, int row_pitch,
                                                                       long long plane_pitch) {
    const int tile = (int)blockIdx.x;
    int lo = 0, hi = batch;               // the last image whose first tile is <= tile (every image has at least one tile, so the prefix is strictly increasing)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (table[mid].tile0 <= tile) lo = mid; else hi = mid;
    }
    const PpArgs& a = table[lo];
    if (a.u8) pp_tile<true, true>(a, a.src, tile - a.tile0, canvas + a.dst_off, row_pitch, plane_pitch);
    else pp_tile<false, true>(a, a.src, tile - a.tile0, canvas + a.dst_off, row_pitch, plane_pitch);
}

// ---------------------------------------------------------------- host: tile shape per plan
// Source rows / columns one tile of n outputs can touch: x1(last) - x0(first) + 1 <= (n - 1) scale + 3 (+ float slack) plus the blur halo.
static int footprint(int n, double scale, int taps, int in_size) {
    const long long span = (long long)std::floor((double)(n - 1) * scale * (1.0 + 1e-6)) + 4;
    return (int)std::min<long long>(span, in_size) + 2 * (taps / 2);
}
struct PpTile { int lg_tw, lg_th, sw, sh, pitch; size_t lds; };
static size_t tile_lds(int TW, int TH, int sw, int sh, int pitch) {
    return sizeof(float) * ((size_t)sh * pitch + (size_t)sh * 2 * TW + 3 * TW + 3 * TH);
}
static bool pick_tile(const PpArgs& a, PpTile& best) {
    double best_cost = 0.0; bool found = false;
    for (size_t budget : {(size_t)PP_LDS_BUDGET, (size_t)64 * 1024}) {
        for (int lw = PP_LG_TW_MAX; lw >= 0; --lw) for (int lh = PP_LG_TH_MAX; lh >= 0; --lh) {
            const int TW = 1 << lw, TH = 1 << lh;
            if ((lw > 0 && TW / 2 >= a.Wo) || (lh > 0 && TH / 2 >= a.Ho)) continue;     // the half-size tile covers the axis too
            const int sw = footprint(TW, a.scale_x, a.ksx, a.W), sh = footprint(TH, a.scale_y, a.ksy, a.H), pitch = sw | 1;
            const size_t lds = tile_lds(TW, TH, sw, sh, pitch);
            if (lds > budget) continue;
            const double cost = (double)sh * (pitch + 2.0 * TW * a.ksx / 4.0) / ((double)std::min(TW, a.Wo) * std::min(TH, a.Ho));   // LDS traffic per output
            if (!found || cost < best_cost) { best = PpTile{lw, lh, sw, sh, pitch, lds}; best_cost = cost; found = true; }
        }
        if (found) return true;
    }
    return false;
}

// torch's float32 statement of the kernel: x = arange(ks) - ks // 2; g = exp(-x^2 / (2 sigma^2)); g / g.sum()
static void gaussian_taps(int ks, double sigma, float* w) {
    if (ks == 1) { w[0] = 1.f; return; }
    const float denom = (float)(2.0 * sigma * sigma);
    float sum = 0.f;
    for (int i = 0; i < ks; ++i) { const float x = (float)(i - ks / 2); w[i] = std::exp(-(x * x) / denom); sum += w[i]; }
    for (int i = 0; i < ks; ++i) w[i] /= sum;
}

static int check_plan(const lg_resize_plan* p) {
    if (!p) return set_error(LG_ERR_INVALID, "null plan");
    if (p->h_in < 1 || p->w_in < 1 || p->h_out < 1 || p->w_out < 1) return set_error(LG_ERR_INVALID, "image and target sizes must be positive");
    if (p->h_in > LG_PREPROCESS_MAX_SIDE || p->w_in > LG_PREPROCESS_MAX_SIDE || p->h_out > LG_PREPROCESS_MAX_SIDE || p->w_out > LG_PREPROCESS_MAX_SIDE)
        return set_error(LG_ERR_INVALID, "image or target side above LG_PREPROCESS_MAX_SIDE (2^23)");
    const int ks[2] = {p->ks_y, p->ks_x}, len[2] = {p->h_in, p->w_in};
    const double sg[2] = {p->sigma_y, p->sigma_x};
    for (int i = 0; i < 2; ++i) {
        if (ks[i] < 1 || (ks[i] & 1) == 0) return set_error(LG_ERR_INVALID, "blur kernel sizes must be odd and positive");
        if (ks[i] > LG_PREPROCESS_MAX_TAPS)
            return set_error(LG_ERR_INVALID, "antialias kernel of " + std::to_string(ks[i]) + " taps is above LG_PREPROCESS_MAX_TAPS (33): downscale factors up to ~17 per call");
        if (ks[i] / 2 >= len[i])
            return set_error(LG_ERR_INVALID, "reflect padding of " + std::to_string(ks[i] / 2) + " needs an axis longer than that (ks / 2 < axis length), got " + std::to_string(len[i]));
        if (ks[i] > 1 && !(sg[i] > 0.0)) return set_error(LG_ERR_INVALID, "sigma must be positive where ks > 1");
    }
    return LG_OK;
}

// The envelope of one image under one plan (everything lg_preprocess_resize refuses, in its order) and the image's record: strides, scales, taps, tile shape.
// `tiles`: the image's tile count.  Host arithmetic only.
static int image_record(const lg_image_source& im, const lg_resize_plan* plan, PpArgs& a, PpTile& t, long long& tiles) {
    if (im.dtype != LG_DTYPE_F32 && im.dtype != LG_DTYPE_U8) return set_error(LG_ERR_INVALID, "unknown dtype (LG_DTYPE_F32 / LG_DTYPE_U8)");
    if (im.channels != 1 && im.channels != 3) return set_error(LG_ERR_INVALID, "channels must be 1 or 3");
    const int rc = check_plan(plan);
    if (rc != LG_OK) return rc;
    const int h = im.h, w = im.w;
    if (h != plan->h_in || w != plan->w_in) return set_error(LG_ERR_INVALID, "the plan was made for another image size");
    if (im.stride_b < 0 || im.stride_c < 0 || im.stride_y < 0 || im.stride_x < 0) return set_error(LG_ERR_INVALID, "strides must be non-negative");
    const long long reach = (long long)(im.channels - 1) * im.stride_c + (long long)(h - 1) * im.stride_y + (long long)(w - 1) * im.stride_x;
    if (im.stride_c > 2147483647LL || im.stride_y > 2147483647LL || im.stride_x > 2147483647LL || reach > 2147483647LL)
        return set_error(LG_ERR_INVALID, "one image must span fewer than 2^31 elements (32-bit element offsets)");
    if (!im.data) return set_error(LG_ERR_INVALID, "null pointer");

    a = PpArgs{};
    a.src = im.data;
    a.stride_b = im.stride_b; a.stride_c = (int)im.stride_c; a.stride_y = (int)im.stride_y; a.stride_x = (int)im.stride_x;
    a.u8 = im.dtype == LG_DTYPE_U8; a.C = im.channels; a.H = h; a.W = w; a.Ho = plan->h_out; a.Wo = plan->w_out;
    a.ksx = plan->ks_x; a.ksy = plan->ks_y; a.align = plan->align_corners ? 1 : 0;
    if (a.align) {
        a.scale_x = a.Wo > 1 ? (float)(w - 1) / (float)(a.Wo - 1) : 0.f;
        a.scale_y = a.Ho > 1 ? (float)(h - 1) / (float)(a.Ho - 1) : 0.f;
    } else {
        a.scale_x = (float)w / (float)a.Wo; a.scale_y = (float)h / (float)a.Ho;
    }
    gaussian_taps(a.ksx, plan->sigma_x, a.wx);
    gaussian_taps(a.ksy, plan->sigma_y, a.wy);
    if (!pick_tile(a, t)) return set_error(LG_ERR_INVALID, "no tile shape fits this plan");   // (1 x 1 always fits inside the envelope)
    a.lg_tw = t.lg_tw; a.lg_th = t.lg_th; a.sw_max = t.sw; a.sh_max = t.sh; a.pitch = t.pitch;
    const int TW = 1 << t.lg_tw, TH = 1 << t.lg_th;
    a.tiles_x = (a.Wo + TW - 1) / TW;
    tiles = (long long)a.tiles_x * ((a.Ho + TH - 1) / TH);
    if (tiles > 2147483647LL) return set_error(LG_ERR_INVALID, "too many output tiles");
    return LG_OK;
}

// What lg_preprocess_ragged_plan writes in front of the records: the launch geometry, read back from the HOST copy by lg_preprocess_resize_ragged
struct PpTableHead { uint32_t magic; int batch, c_out, hc, wc, lds; long long tiles; long long pad_[4]; };
constexpr uint32_t PP_TABLE_MAGIC = 0x7072a99du;
static_assert(sizeof(PpTableHead) == 64 && sizeof(PpArgs) % 8 == 0, "the records follow the head 8-byte aligned");

}  // namespace lg

using namespace lg;

extern "C" {

int lg_preprocess_plan(int32_t h, int32_t w, int32_t resize_h, int32_t resize_w, int32_t side, int32_t antialias, int32_t align_corners,
                       lg_resize_plan* plan) {
    if (!plan) return set_error(LG_ERR_INVALID, "null plan");
    if (h < 1 || w < 1) return set_error(LG_ERR_INVALID, "image size must be positive");
    if (side < LG_SIDE_LONG || side > LG_SIDE_HORZ) return set_error(LG_ERR_INVALID, "unknown side (LG_SIDE_LONG / SHORT / VERT / HORZ)");
    long long ho, wo;
    if (resize_w == LG_RESIZE_EDGE) {           // kornia's side_to_image_size, in double like the Python floats
        const int s = resize_h;
        if (s < 1) return set_error(LG_ERR_INVALID, "resize must be positive");
        const double ar = (double)w / (double)h;
        bool s_is_h;
        if (side == LG_SIDE_VERT) s_is_h = true;
        else if (side == LG_SIDE_HORZ) s_is_h = false;
        else s_is_h = (side == LG_SIDE_SHORT) ^ (ar < 1.0);
        if (s_is_h) { ho = s; wo = (long long)((double)s * ar); }
        else { ho = (long long)((double)s / ar); wo = s; }
    } else {
        if (resize_h < 1 || resize_w < 1) return set_error(LG_ERR_INVALID, "resize (h, w) must be positive");
        ho = resize_h; wo = resize_w;
    }
    if (ho < 1 || wo < 1) return set_error(LG_ERR_INVALID, "the target size has a zero side (" + std::to_string(ho) + " x " + std::to_string(wo) + ")");
    if (ho > LG_PREPROCESS_MAX_SIDE || wo > LG_PREPROCESS_MAX_SIDE || h > LG_PREPROCESS_MAX_SIDE || w > LG_PREPROCESS_MAX_SIDE)
        return set_error(LG_ERR_INVALID, "image or target side above LG_PREPROCESS_MAX_SIDE (2^23)");
    lg_resize_plan p{};
    p.h_in = h; p.w_in = w; p.h_out = (int32_t)ho; p.w_out = (int32_t)wo;
    p.ks_y = p.ks_x = 1; p.sigma_y = p.sigma_x = 0.0;
    p.align_corners = align_corners ? 1 : 0;
    p.identity = (ho == h && wo == w) ? 1 : 0;
    const double fy = (double)h / (double)ho, fx = (double)w / (double)wo;
    if (!p.identity && antialias && std::max(fy, fx) > 1.0) {
        const double f[2] = {fy, fx};
        double* sg[2] = {&p.sigma_y, &p.sigma_x};
        int32_t* ks[2] = {&p.ks_y, &p.ks_x};
        for (int i = 0; i < 2; ++i) {
            const double sigma = std::max((f[i] - 1.0) / 2.0, 0.001);
            const double k = std::max(4.0 * sigma, 3.0);
            if (k > 1e6) return set_error(LG_ERR_INVALID, "antialias kernel above LG_PREPROCESS_MAX_TAPS (33)");
            int n = (int)k;
            if ((n & 1) == 0) ++n;
            *sg[i] = sigma; *ks[i] = n;
        }
    }
    p.scale_x = (double)p.w_out / (double)w; p.scale_y = (double)p.h_out / (double)h;
    const int rc = check_plan(&p);
    if (rc != LG_OK) return rc;
    *plan = p;
    return LG_OK;
}

int lg_preprocess_resize(const void* src, int32_t dtype, int32_t batch, int32_t channels, int32_t h, int32_t w, int64_t stride_b,
                         int64_t stride_c, int64_t stride_y, int64_t stride_x, const lg_resize_plan* plan, float* dst, void* hip_stream) {
    if (dtype != LG_DTYPE_F32 && dtype != LG_DTYPE_U8) return set_error(LG_ERR_INVALID, "unknown dtype (LG_DTYPE_F32 / LG_DTYPE_U8)");
    if (batch < 1 || batch > 65535) return set_error(LG_ERR_INVALID, "batch must be in [1, 65535]");
    const lg_image_source image{src, dtype, channels, h, w, stride_b, stride_c, stride_y, stride_x};
    PpArgs a{}; PpTile t{}; long long tiles = 0;
    const int rc = image_record(image, plan, a, t, tiles);
    if (rc != LG_OK) return rc;
    if (!dst) return set_error(LG_ERR_INVALID, "null pointer");
    a.dst = dst;
    const dim3 grid((unsigned)tiles, (unsigned)batch);
    if (a.u8) hipLaunchKernelGGL(pp_resize_kernel<true>, grid, dim3(PP_THREADS), t.lds, static_cast<hipStream_t>(hip_stream), a);
    else hipLaunchKernelGGL(pp_resize_kernel<false>, grid, dim3(PP_THREADS), t.lds, static_cast<hipStream_t>(hip_stream), a);
    HIPCHK(hipGetLastError());
    return LG_OK;
}

int64_t lg_preprocess_ragged_table_bytes(int32_t batch) {
    if (batch < 1 || batch > LG_PREPROCESS_RAGGED_MAX_BATCH) return 0;
    return (int64_t)sizeof(PpTableHead) + (int64_t)batch * (int64_t)sizeof(PpArgs);
}

int lg_preprocess_ragged_plan(const lg_image_source* sources, const lg_resize_plan* plans, int32_t batch, int32_t c_out, int32_t hc, int32_t wc,
                              void* table_host, int64_t table_bytes, int64_t* total_tiles, int64_t* lds_bytes, int32_t* tile_prefix, int32_t* image_lds) {
    if (batch < 1 || batch > LG_PREPROCESS_RAGGED_MAX_BATCH) return set_error(LG_ERR_INVALID, "batch must be in [1, LG_PREPROCESS_RAGGED_MAX_BATCH] (256)");
    if (!sources || !plans || !table_host || !total_tiles || !lds_bytes) return set_error(LG_ERR_INVALID, "null pointer");
    if (c_out != 1 && c_out != 3) return set_error(LG_ERR_INVALID, "canvas channels must be 1 or 3");
    if (hc < 1 || wc < 1 || (long long)hc * wc > 2147483647LL) return set_error(LG_ERR_INVALID, "the canvas must have between 1 and 2^31 - 1 pixels per plane");
    if (table_bytes < lg_preprocess_ragged_table_bytes(batch))
        return set_error(LG_ERR_INVALID, "the table buffer holds " + std::to_string(table_bytes) + " bytes, lg_preprocess_ragged_table_bytes(batch) = " +
                                             std::to_string(lg_preprocess_ragged_table_bytes(batch)));
    PpTableHead head{};
    PpArgs* table = reinterpret_cast<PpArgs*>(static_cast<char*>(table_host) + sizeof(PpTableHead));
    long long sum = 0; size_t lds = 0;
    for (int b = 0; b < batch; ++b) {
        PpArgs a{}; PpTile t{}; long long tiles = 0;
        const int rc = image_record(sources[b], &plans[b], a, t, tiles);
        if (rc != LG_OK) return set_error(rc, "image " + std::to_string(b) + ": " + lg_last_error());
        if (a.Ho > hc || a.Wo > wc)
            return set_error(LG_ERR_INVALID, "image " + std::to_string(b) + ": the target " + std::to_string(a.Ho) + " x " + std::to_string(a.Wo) + " does not fit the canvas " +
                                                 std::to_string(hc) + " x " + std::to_string(wc));
        a.dst_off = (long long)b * c_out * hc * wc;
        a.mode = a.C == c_out ? PP_MODE_SAME : (a.C == 1 ? PP_MODE_BROADCAST : PP_MODE_GRAY);
        a.copy = plans[b].identity ? 1 : 0;      // (check_plan: identity means the same size, ks = 1)
        if (a.copy && (a.Ho != a.H || a.Wo != a.W || a.ksx != 1 || a.ksy != 1)) return set_error(LG_ERR_INVALID, "image " + std::to_string(b) + ": an identity plan that changes the image");
        a.tile0 = (int)sum;
        if (tile_prefix) tile_prefix[b] = (int32_t)sum;
        if (image_lds) image_lds[b] = (int32_t)t.lds;
        sum += tiles;
        if (sum > 2147483647LL) return set_error(LG_ERR_INVALID, "too many output tiles in one launch (2^31 or more)");
        lds = std::max(lds, t.lds);
        table[b] = a;
    }
    head.magic = PP_TABLE_MAGIC; head.batch = batch; head.c_out = c_out; head.hc = hc; head.wc = wc; head.lds = (int)lds; head.tiles = sum;
    std::memcpy(table_host, &head, sizeof(head));
    *total_tiles = sum; *lds_bytes = (int64_t)lds;
    return LG_OK;
}

int lg_preprocess_resize_ragged(const void* table_host, const void* table_dev, int32_t batch, float* canvas, int32_t zero_fill, void* hip_stream) {
    if (!table_host || !table_dev || !canvas) return set_error(LG_ERR_INVALID, "null pointer");
    PpTableHead head;
    std::memcpy(&head, table_host, sizeof(head));
    if (head.magic != PP_TABLE_MAGIC) return set_error(LG_ERR_INVALID, "table_host was not filled by lg_preprocess_ragged_plan");
    if (batch != head.batch || batch < 1 || batch > LG_PREPROCESS_RAGGED_MAX_BATCH) return set_error(LG_ERR_INVALID, "the table was planned for another batch");
    if (head.tiles < 1 || head.tiles > 2147483647LL || head.lds < 0 || head.lds > 64 * 1024 || (head.c_out != 1 && head.c_out != 3) || head.hc < 1 || head.wc < 1)
        return set_error(LG_ERR_INVALID, "table_host was not filled by lg_preprocess_ragged_plan");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const long long plane = (long long)head.hc * head.wc;
    if (zero_fill) HIPCHK(hipMemsetAsync(canvas, 0, sizeof(float) * (size_t)batch * head.c_out * plane, stream));
    const PpArgs* table = reinterpret_cast<const PpArgs*>(static_cast<const char*>(table_dev) + sizeof(PpTableHead));
    hipLaunchKernelGGL(pp_resize_ragged_kernel, dim3((unsigned)head.tiles), dim3(PP_THREADS), (size_t)head.lds, stream, table, (int)batch, canvas, head.wc, plane);
    HIPCHK(hipGetLastError());
    return LG_OK;
}

}  // extern "C"
