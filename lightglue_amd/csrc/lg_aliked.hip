// lightglue_amd — the ALIKED extractor (aliked-n16 / n16rot / n32) on the MI355X: encoder, aggregation, score head, DKD and SDDH of
// the reference's ALIKED.forward (lightglue/aliked.py:612-760), every arithmetic step in the kernels below.
//
// Arithmetic is EXACT fp32 (v_mfma_f32_16x16x4_f32 / VALU): DKD thresholds and NMS-compares the scores, so they must agree with an fp32
// convolution to round-off.  Layouts are NHWC throughout.  The stages:
//   * convolutions: the implicit GEMM SuperPoint's fp32 stack runs (launch_conv, lg_extract.hip), with an output tile width of 16 / 32 / 64
//     channels chosen from cout.  BatchNorm (eval: running statistics) is folded into weights and bias at pack time (launch_fold); the
//     ResBlock's 1 x 1 downsample (with bias) is extra K of conv2's GEMM, read at the centre pixel of the block input; SELU is the epilogue.
//   * block1.conv1 (cin = 3, K = 27) is VALU; it reads the image through clamped addresses, which is InputPadder's replicate padding to a
//     multiple of 32, and broadcasts a 1-channel image to 3 channels (kornia grayscale_to_rgb).
//   * deformable convs (blocks 3 and 4, torchvision deform_conv2d without mask): offset conv (3 x 3, bias, 18 channels) on the MFMA path,
//     offsets clamped to +-max(h, w) / 4, bilinear sampling into a [pixel][tap * cin] buffer, then the MFMA GEMM with regular_conv.weight.
//   * aggregation + score head: conv1 .. conv4 (1 x 1, SELU) write 32-channel level maps at their own resolution; one per-pixel kernel
//     builds the 128 channels of x1234 on the fly (x1 at the pixel, x2 / x3 / x4 upsampled bilinearly, align_corners=True) and applies
//     score_head.0 + SELU; three small VALU 3 x 3 convs (SELU, SELU, sigmoid) finish, the last one crops the padding.  The full-resolution
//     128-channel map is never written.
//   * DKD (aliked.py:94-262, sub_pixel): simple_nms, zeroed borders, threshold and top-k selection on SuperPoint's detection kernels
//     (lg_extract.hip); here the threshold of each image (whole-batch mean fallback), the soft-argmax over the (2r+1)^2 window and the
//     bilinear score.
//   * SDDH (aliked.py:479-609): per keypoint the normalised x1234 vectors at the 3 x 3 patch and at the n_pos sample positions are
//     recomputed from the level maps; the 3 x 3 offset conv, sf_conv and the agg_weights contraction are MFMA GEMMs over all keypoints.
#include <string>

#include "lg_extract.h"
#include "../../include/lightglue_amd.h"

namespace lg {
namespace {

// ==================================================================================================== convolutions (MFMA)
// act_selu: SELU epilogue; in2 / w2 / Cin2: extra K at the centre pixel
void conv(const float* in, const float* w, const float* bias, float* out, int B, int H, int W, int Cin, int Cout, int taps, int act_selu, hipStream_t s,
          const float* in2 = nullptr, const float* w2 = nullptr, int Cin2 = 0) {
    launch_conv(ConvArgs{in, w, bias, in2, w2, out, B, H, W, Cin, Cin2, Cout, taps, act_selu ? ACT_SELU : ACT_NONE, 0, 0}, s);
}
// the same on a ragged batch: H, W are the canvas of the level, `padded` the images' padded sizes [B][2] (Wp_b, Hp_b) at full resolution, `shift` the level's
void conv(const int* padded, int shift, const float* in, const float* w, const float* bias, float* out, int B, int H, int W, int Cin, int Cout, int taps,
          int act_selu, hipStream_t s, const float* in2 = nullptr, const float* w2 = nullptr, int Cin2 = 0) {
    RaggedConvArgs a{};
    static_cast<ConvArgs&>(a) = ConvArgs{in, w, bias, in2, w2, out, B, H, W, Cin, Cin2, Cout, taps, act_selu ? ACT_SELU : ACT_NONE, 0, 0};
    a.sizes = padded; a.size_shift = shift;
    launch_conv(a, s);
}

// a [rows][K] x [Cout][K] GEMM as a 1 x 1 convolution over a 32-pixel-wide "image" (rows % 32 == 0)
void gemm(const float* in, const float* w, const float* bias, float* out, int rows, int K, int Cout, int act, hipStream_t s) {
    conv(in, w, bias, out, 1, rows / 32, 32, K, Cout, 1, act, s);
}

// ==================================================================================================== ragged geometry
// A ragged batch (LG_EXTRACT_RAGGED): the arrays are a CANVAS, image b its top-left h_b x w_b corner with its OWN InputPadder geometry, its padded frame in the
// top-left corner of the padded canvas.  Every kernel below is a template over Uniform / Ragged, passed as its LAST argument: addresses and strides come from
// the canvas (the size arguments the uniform kernel always had), every bound from the image's Frame.  The Uniform instance reads the same arguments for both and
// keeps the kernel arguments it had (an empty struct follows them).
struct Uniform {};
struct Ragged { const int* sizes; int Hc, Wc, shift; };      // [B][2] (w, h), clamped into the canvas Hc x Wc; shift: the pyramid level of this launch
template <class R> inline constexpr bool ragged = false;
template <> inline constexpr bool ragged<Ragged> = true;

struct Frame { int h, w, Hp, Wp, pt, pl; };                  // image size, padded size, top / left padding (InputPadder(divis_by = 32): centred)
__host__ __device__ __forceinline__ Frame frame_of(int h, int w) {
    const int ph = ((h / 32 + 1) * 32 - h) % 32, pw = ((w / 32 + 1) * 32 - w) % 32;
    return Frame{h, w, h + ph, w + pw, ph / 2, pw / 2};
}
__device__ __forceinline__ Frame frame_of(const Ragged& r, int b) {
    return frame_of(min(max(r.sizes[2 * b + 1], 1), r.Hc), min(max(r.sizes[2 * b], 1), r.Wc));
}
// the padded sizes (Wp_b, Hp_b) RaggedConvArgs takes: multiples of 32, so every level's shift is exact.  thread = image
__global__ void ak_padded_sizes_kernel(Ragged r, int B, int* padded) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const Frame f = frame_of(r, b);
    padded[2 * b] = f.Wp; padded[2 * b + 1] = f.Hp;
}

// ==================================================================================================== encoder helpers (VALU)
// block1.conv1: image [B][C][H][W] (C = 1 or 3) -> padded [B][Hp][Wp][16], BN folded, SELU.  w: [9 taps][3 cin][16 cout].
// thread = (padded pixel, 4 output channels).  Ragged: H, W, Hp, Wp are the canvas and its padded canvas; the replicate clamp is against the image, the conv's
// zero padding at the image's padded frame, and nothing is stored outside that frame.
template <class R>
__global__ __launch_bounds__(256) void ak_conv_first_kernel(const float* img, int C, int H, int W, int Hp, int Wp, int pt, int pl, const float* w,
                                                            const float* bias, float* out, int B, R rg) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, total = (long long)B * Hp * Wp * 4;
    if (idx >= total) return;
    const int c4 = (int)(idx & 3);
    const long long pix = idx >> 2;
    const int xp = (int)(pix % Wp), yp = (int)((pix / Wp) % Hp), b = (int)(pix / ((long long)Wp * Hp));
    Frame fr{H, W, Hp, Wp, pt, pl};
    if constexpr (ragged<R>) {
        fr = frame_of(rg, b);
        if (yp >= fr.Hp || xp >= fr.Wp) return;
    }
    f32x4 s = *reinterpret_cast<const f32x4*>(bias + c4 * 4);
    for (int t = 0; t < 9; ++t) {
        const int yy = yp + t / 3 - 1, xx = xp + t % 3 - 1;
        if (yy < 0 || yy >= fr.Hp || xx < 0 || xx >= fr.Wp) continue;            // the conv's own zero padding of the padded image
        const int sy = min(max(yy - fr.pt, 0), fr.h - 1), sx = min(max(xx - fr.pl, 0), fr.w - 1);   // replicate padding (InputPadder)
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
            const float p = img[(((long long)b * C + (C == 1 ? 0 : ci)) * H + sy) * W + sx];
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (t * 3 + ci) * 16 + c4 * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) s[r] = __builtin_fmaf(p, wv[r], s[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = selu(s[r]);
    *reinterpret_cast<f32x4*>(out + pix * 16 + c4 * 4) = s;
}

// f x f average pooling (nn.AvgPool2d, stride f), NHWC, C % 4 == 0.  thread = (output pixel, 4 channels).  Ragged: H, W are the canvas of the input level
// (rg.shift); output pixels outside the image's pooled level are neither computed nor stored
template <class R>
__global__ __launch_bounds__(256) void ak_pool_kernel(const float* in, float* out, int B, int H, int W, int C, int f, R rg) {
    const int Ho = H / f, Wo = W / f, C4 = C >> 2;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, total = (long long)B * Ho * Wo * C4;
    if (idx >= total) return;
    const int c4 = (int)(idx % C4);
    const long long pix = idx / C4;
    const int xo = (int)(pix % Wo), yo = (int)((pix / Wo) % Ho), b = (int)(pix / ((long long)Wo * Ho));
    if constexpr (ragged<R>) {
        const Frame fr = frame_of(rg, b);
        if (yo >= (fr.Hp >> rg.shift) / f || xo >= (fr.Wp >> rg.shift) / f) return;
    }
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < f; ++i)
        for (int j = 0; j < f; ++j) s += *reinterpret_cast<const f32x4*>(in + (((long long)b * H + yo * f + i) * W + xo * f + j) * C + c4 * 4);
    const float inv = (float)(f * f);
    *reinterpret_cast<f32x4*>(out + pix * C + c4 * 4) = f32x4{s[0] / inv, s[1] / inv, s[2] / inv, s[3] / inv};
}

// torchvision deform_conv2d sampling (3 x 3, pad 1, stride 1, one offset group, no mask): in [B][h][w][cin], off [B][h][w][18]
// (tap k = 3i + j: dy = channel 2k, dx = channel 2k + 1, clamped to +-max_off) -> cols [B][h][w][9][cin].  thread = (pixel, tap, 4 channels)
// Ragged: h, w are the canvas of the level (rg.shift) and give the strides; the sample bounds and max_off = max(h_b', w_b') / 4 are the image's level extent
// (the canvas maximum would clamp the offsets differently), and a pixel outside it returns before any load.
template <class R>
__global__ __launch_bounds__(256) void ak_deform_gather_kernel(const float* in, const float* off, float* cols, int B, int h, int w, int cin, float max_off, R rg) {
    const int C4 = cin >> 2;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, total = (long long)B * h * w * 9 * C4;
    if (idx >= total) return;
    const int c4 = (int)(idx % C4);
    const long long rest = idx / C4;
    const int k = (int)(rest % 9);
    const long long pix = rest / 9;
    const int x = (int)(pix % w), y = (int)((pix / w) % h), b = (int)(pix / ((long long)w * h));
    int hb = h, wb = w;      // the image's level extent: every bound
    if constexpr (ragged<R>) {
        const Frame fr = frame_of(rg, b);
        hb = fr.Hp >> rg.shift; wb = fr.Wp >> rg.shift;
        if (y >= hb || x >= wb) return;
        max_off = (float)max(hb, wb) / 4.f;
    }
    const float dy = fminf(fmaxf(off[pix * 18 + 2 * k], -max_off), max_off), dx = fminf(fmaxf(off[pix * 18 + 2 * k + 1], -max_off), max_off);
    const float py = (float)(y - 1 + k / 3) + dy, px = (float)(x - 1 + k % 3) + dx;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!(py <= -1.f || py >= (float)hb || px <= -1.f || px >= (float)wb)) {
        const int hl = (int)floorf(py), wl = (int)floorf(px), hh = hl + 1, wh = wl + 1;
        const float lh = py - (float)hl, lw = px - (float)wl, uh = 1.f - lh, uw = 1.f - lw;
        const float* base = in + (long long)b * h * w * cin + c4 * 4;
        auto at = [&](int yy, int xx) { return *reinterpret_cast<const f32x4*>(base + ((long long)yy * w + xx) * cin); };
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 v1 = (hl >= 0 && wl >= 0) ? at(hl, wl) : z;
        const f32x4 v2 = (hl >= 0 && wh <= wb - 1) ? at(hl, wh) : z;
        const f32x4 v3 = (hh <= hb - 1 && wl >= 0) ? at(hh, wl) : z;
        const f32x4 v4 = (hh <= hb - 1 && wh <= wb - 1) ? at(hh, wh) : z;
        const float w1 = uh * uw, w2 = uh * lw, w3 = lh * uw, w4 = lh * lw;
        v = w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4;
    }
    *reinterpret_cast<f32x4*>(cols + (pix * 9 + k) * cin + c4 * 4) = v;
}

// bilinear upsampling coordinate (nn.Upsample, align_corners=True): source rows i0 / i1 and their weights for output row `dst`
struct Up { int i0, i1; float l0, l1; };
__device__ __forceinline__ Up up_coord(int dst, int in, int out) {
    if (in == out) return Up{dst, dst, 1.f, 0.f};
    const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
    const float src = scale * (float)dst;
    const int i0 = min((int)floorf(src), in - 1);
    const float l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
    return Up{i0, i0 + (i0 < in - 1 ? 1 : 0), 1.f - l1, l1};
}

// the four 32-channel level maps of x1234 (after conv1 .. conv4 + SELU); level l has (Hp >> sh[l]) x (Wp >> sh[l]) pixels, sh = 0, 1, 3, 5
struct AkLevels { const float* x[4]; int B, Hp, Wp; };
__host__ __device__ __forceinline__ int lvl_shift(int l) { return l == 0 ? 0 : (l == 1 ? 1 : (l == 2 ? 3 : 5)); }

// x1 .. x4 at padded pixel (yp, xp) of image b: level l's map has (L.Hp >> sh) x (L.Wp >> sh) pixels in memory (the canvas), the image's own part of it is
// (fr.Hp >> sh) x (fr.Wp >> sh), and the align_corners=True scales of up_coord depend on the image's level and full extents.  Uniform: fr.Hp == L.Hp, fr.Wp == L.Wp
struct LevelTaps { const float* p00; const float* p01; const float* p10; const float* p11; Up uy, ux; };
__device__ __forceinline__ LevelTaps level_taps(const AkLevels& L, const Frame& fr, int l, int b, int yp, int xp) {
    const int sh = lvl_shift(l), hc = L.Hp >> sh, wc = L.Wp >> sh;
    const Up uy = up_coord(yp, fr.Hp >> sh, fr.Hp), ux = up_coord(xp, fr.Wp >> sh, fr.Wp);
    const float* m = L.x[l] + (long long)b * hc * wc * 32;
    return LevelTaps{m + ((long long)uy.i0 * wc + ux.i0) * 32, m + ((long long)uy.i0 * wc + ux.i1) * 32, m + ((long long)uy.i1 * wc + ux.i0) * 32,
                     m + ((long long)uy.i1 * wc + ux.i1) * 32, uy, ux};
}

// score_head.0 (128 -> 8, no bias) + SELU on x1234 built per padded pixel.  w0: [8][128].  out [B][Hp][Wp][8].  thread = padded pixel (Ragged: of the padded
// canvas; pixels outside the image's padded frame return)
template <class R>
__global__ __launch_bounds__(256) void ak_score_head0_kernel(AkLevels L, const float* w0, float* out, R rg) {
    __shared__ float sw[8 * 128];
    for (int i = threadIdx.x; i < 8 * 128; i += 256) sw[i] = w0[i];
    __syncthreads();
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (long long)L.B * L.Hp * L.Wp) return;
    const int xp = (int)(pix % L.Wp), yp = (int)((pix / L.Wp) % L.Hp), b = (int)(pix / ((long long)L.Wp * L.Hp));
    Frame fr{0, 0, L.Hp, L.Wp, 0, 0};
    if constexpr (ragged<R>) {
        fr = frame_of(rg, b);
        if (yp >= fr.Hp || xp >= fr.Wp) return;
    }
    float acc[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[o] = 0.f;
    for (int l = 0; l < 4; ++l) {
        const LevelTaps T = level_taps(L, fr, l, b, yp, xp);
        const Up uy = T.uy, ux = T.ux;
        const float* p00 = T.p00; const float* p01 = T.p01; const float* p10 = T.p10; const float* p11 = T.p11;
        for (int c4 = 0; c4 < 8; ++c4) {
            f32x4 v;
            if (l == 0) v = *reinterpret_cast<const f32x4*>(p00 + c4 * 4);
            else {
                const f32x4 a00 = *reinterpret_cast<const f32x4*>(p00 + c4 * 4), a01 = *reinterpret_cast<const f32x4*>(p01 + c4 * 4);
                const f32x4 a10 = *reinterpret_cast<const f32x4*>(p10 + c4 * 4), a11 = *reinterpret_cast<const f32x4*>(p11 + c4 * 4);
                v = uy.l0 * (ux.l0 * a00 + ux.l1 * a01) + uy.l1 * (ux.l0 * a10 + ux.l1 * a11);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = l * 32 + c4 * 4 + r;
#pragma unroll
                for (int o = 0; o < 8; ++o) acc[o] = __builtin_fmaf(sw[o * 128 + c], v[r], acc[o]);
            }
        }
    }
    f32x4 r0 = {selu(acc[0]), selu(acc[1]), selu(acc[2]), selu(acc[3])}, r1 = {selu(acc[4]), selu(acc[5]), selu(acc[6]), selu(acc[7])};
    *reinterpret_cast<f32x4*>(out + pix * 8) = r0;
    *reinterpret_cast<f32x4*>(out + pix * 8 + 4) = r1;
}

// score_head.2 / .4 / .6: 3 x 3, zero pad, no bias, raw weights [COUT][CIN][3][3].  Not FINAL: SELU, [B][Hp][Wp][COUT].  FINAL (COUT = 1): sigmoid
// and the unpad crop, scores [B][H][W].  thread = output pixel.  Ragged: Hp, Wp, H, W are the canvases (strides); the zero padding is at the image's padded
// extent, nothing is stored outside its frame, and FINAL crops with the image's pt, pl and writes 0 for the score pixels outside h_b x w_b (the score canvas is
// defined everywhere)
template <int CIN, int COUT, bool FINAL, class R>
__global__ __launch_bounds__(256) void ak_small_conv_kernel(const float* in, const float* w, float* out, int B, int Hp, int Wp, int H, int W, int pt, int pl, R rg) {
    const int OH = FINAL ? H : Hp, OW = FINAL ? W : Wp;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (long long)B * OH * OW) return;
    const int xo = (int)(pix % OW), yo = (int)((pix / OW) % OH), b = (int)(pix / ((long long)OW * OH));
    Frame fr{H, W, Hp, Wp, pt, pl};
    if constexpr (ragged<R>) {
        fr = frame_of(rg, b);
        if (FINAL ? (yo >= fr.h || xo >= fr.w) : (yo >= fr.Hp || xo >= fr.Wp)) {
            if constexpr (FINAL) out[pix] = 0.f;
            return;
        }
    }
    const int yp = FINAL ? yo + fr.pt : yo, xp = FINAL ? xo + fr.pl : xo;
    float acc[COUT];
#pragma unroll
    for (int o = 0; o < COUT; ++o) acc[o] = 0.f;
    for (int t = 0; t < 9; ++t) {
        const int yy = yp + t / 3 - 1, xx = xp + t % 3 - 1;
        if (yy < 0 || yy >= fr.Hp || xx < 0 || xx >= fr.Wp) continue;
        const float* p = in + (((long long)b * Hp + yy) * Wp + xx) * CIN;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
            const float v = p[ci];
#pragma unroll
            for (int o = 0; o < COUT; ++o) acc[o] = __builtin_fmaf(w[(o * CIN + ci) * 9 + t], v, acc[o]);
        }
    }
    if constexpr (FINAL) {
        out[pix] = 1.f / (1.f + expf(-acc[0]));
    } else {
#pragma unroll
        for (int o = 0; o < COUT; ++o) out[pix * COUT + o] = selu(acc[o]);
    }
}

// ==================================================================================================== DKD
// the threshold of each image (aliked.py:183-193): top-k mode: > 0 (the positive NMS maxima are the candidates); threshold mode: scores_th,
// unless no pixel of the WHOLE batch passes it (or scores_th <= 0): the image's mean score.  Row counts of a.threshold = scores_th.  grid (B), 256 threads
// Ragged (a.sizes): a set of independent images, so "no pixel passes" is asked of image b ALONE (each equals its own batch of one), and the mean is over its
// h_b x w_b pixels: rowsum holds exact zeros below the image, at the thread positions the crop's shorter loop never visits, so the float64 sum is the crop's.
__global__ __launch_bounds__(256) void ak_decide_kernel(DetectArgs a, int topk, const double* rowsum, float* th) {
    const int b = blockIdx.x;
    __shared__ int sh[4];
    __shared__ double shd[256];
    const DetectExtent e = detect_extent(a, b);
    int any = 0;
    if (a.sizes) { for (int i = threadIdx.x; i < a.H; i += 256) any += a.row_counts[b * a.H + i]; }
    else { for (int i = threadIdx.x; i < a.B * a.H; i += 256) any += a.row_counts[i]; }
    any = block_sum(any, sh);
    double s = 0.0;
    for (int y = threadIdx.x; y < a.H; y += 256) s += rowsum[b * a.H + y];
    shd[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) shd[threadIdx.x] += shd[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) {
        const float mean = (float)(shd[0] / ((double)e.h * e.w));
        th[b] = topk > 0 ? 0.f : ((a.threshold > 0.f && any > 0) ? a.threshold : mean);
    }
}

struct AkKeypoints { float* kpts; float* kscores; float* knorm; int* counts; };   // [B][cap][2], [B][cap], [B][cap][2], [B]; cap = a.sel_cap

// per output slot: rank (selected_rank when sorted), soft-argmax refinement and the bilinear score (aliked.py:212-247).  Rows >= the image's
// count are zero-filled.  grid (cap / 256, B).  Ragged (a.sizes): the raster index stays y W + x of the canvas; the window's zero padding, the (w - 1, h - 1)
// factors and the bilinear taps are the image's
__global__ __launch_bounds__(256) void ak_refine_kernel(DetectArgs a, AkKeypoints k) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const int n = selected_count(a, b);
    const long long ob = (long long)b * a.sel_cap;
    const int rank = selection_sorted(a, b) && (int)blockIdx.x * 256 < n ? selected_rank(a.sel_key + ob, n, j) : j;   // (block-uniform)
    if (j >= a.sel_cap) return;
    if (j == 0) k.counts[b] = n;
    if (j >= n) {   // padding rows (written by their own slot j: ranks are a permutation of [0, n))
        k.kpts[2 * (ob + j)] = 0.f; k.kpts[2 * (ob + j) + 1] = 0.f; k.kscores[ob + j] = 0.f;
        k.knorm[2 * (ob + j)] = 0.f; k.knorm[2 * (ob + j) + 1] = 0.f;
        return;
    }
    const int p = a.cand_idx[(long long)b * a.max_candidates + a.sel[ob + j]];
    const int y = p / a.W, x = p - y * a.W, r = a.radius;
    const float* S = a.S + (long long)b * a.H * a.W;
    const DetectExtent e = detect_extent(a, b);
    auto sv = [&](int yy, int xx) { return (yy >= 0 && yy < e.h && xx >= 0 && xx < e.w) ? S[(long long)yy * a.W + xx] : 0.f; };   // unfold: zero padding
    float mx = -INFINITY;
    for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx) mx = fmaxf(mx, sv(y + dy, x + dx));
    float se = 0.f, sx = 0.f, sy = 0.f;
    for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx) {
            const float e = expf(__fdiv_rn(sv(y + dy, x + dx) - mx, 0.1f));
            se += e; sx = __builtin_fmaf(e, (float)dx, sx); sy = __builtin_fmaf(e, (float)dy, sy);
        }
    const float rx = __fdiv_rn(sx, se), ry = __fdiv_rn(sy, se);
    const float wm1 = (float)(e.w - 1), hm1 = (float)(e.h - 1);
    // (xy_nms + residual) / wh * 2 - 1, each step rounded like the reference's tensor ops (no contraction)
    const float kx = __fsub_rn(__fmul_rn(__fdiv_rn(__fadd_rn((float)x, rx), wm1), 2.f), 1.f);
    const float ky = __fsub_rn(__fmul_rn(__fdiv_rn(__fadd_rn((float)y, ry), hm1), 2.f), 1.f);
    // grid_sample(bilinear, align_corners=True, zeros)
    const float ix = __fmul_rn(__fdiv_rn(__fadd_rn(kx, 1.f), 2.f), wm1), iy = __fmul_rn(__fdiv_rn(__fadd_rn(ky, 1.f), 2.f), hm1);
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float ex = fx + 1.f, ey = fy + 1.f;
    const float score = sv(y0, x0) * ((ex - ix) * (ey - iy)) + sv(y0, x0 + 1) * ((ix - fx) * (ey - iy)) + sv(y0 + 1, x0) * ((ex - ix) * (iy - fy)) +
                        sv(y0 + 1, x0 + 1) * ((ix - fx) * (iy - fy));
    const long long o = ob + rank;
    k.kpts[2 * o] = __fdiv_rn(__fmul_rn(wm1, __fadd_rn(kx, 1.f)), 2.f);       // wh * (k + 1) / 2 (aliked.py:756)
    k.kpts[2 * o + 1] = __fdiv_rn(__fmul_rn(hm1, __fadd_rn(ky, 1.f)), 2.f);
    k.kscores[o] = score;
    k.knorm[2 * o] = kx; k.knorm[2 * o + 1] = ky;
}

// ==================================================================================================== SDDH
// one lane = 2 channels of x1234 at padded pixel (yp, xp) of image b's frame `fr`: lanes 0-15 x1, 16-31 x2 (upsampled), 32-47 x3, 48-63 x4; L2-normalised
// over the wave
__device__ __forceinline__ f32x2 x1234_norm(const AkLevels& L, const Frame& fr, int b, int yp, int xp, int lane) {
    const int l = lane >> 4, c = (lane & 15) * 2;
    const LevelTaps T = level_taps(L, fr, l, b, yp, xp);
    f32x2 v;
    if (l == 0) v = *reinterpret_cast<const f32x2*>(T.p00 + c);
    else {
        const Up uy = T.uy, ux = T.ux;
        const f32x2 a00 = *reinterpret_cast<const f32x2*>(T.p00 + c), a01 = *reinterpret_cast<const f32x2*>(T.p01 + c);
        const f32x2 a10 = *reinterpret_cast<const f32x2*>(T.p10 + c), a11 = *reinterpret_cast<const f32x2*>(T.p11 + c);
        v = uy.l0 * (ux.l0 * a00 + ux.l1 * a01) + uy.l1 * (ux.l0 * a10 + ux.l1 * a11);
    }
    const float nrm = sqrtf(wave_sum(v[0] * v[0] + v[1] * v[1]));
    const float d = fmaxf(nrm, 1e-12f);
    return f32x2{v[0] / d, v[1] / d};
}

struct AkDescribe {
    AkLevels L; int H, W, pt, pl, N, np;   // unpadded size, padding offsets, keypoint rows per image, n_pos
    const float* knorm;                    // [B][N][2] normalised keypoints (DKD)
    float* patch; float* off1; float* spos; float* feat; float* sf; float* draw;
    const float* w_off2; const float* b_off2;
    const int* counts; float* out;
    int out_f16;                           // != 0: `out` holds binary16 rows (LG_EXTRACT_DESC_F16): the fp32 result rounded once, to nearest even, on store
};
// Ragged: H, W and L.Hp, L.Wp are the canvases (the level maps' strides), pt / pl unused; image b's frame gives the grid denormalisation, the pad offset into
// the level maps, the upsampling coordinates and every tap bound.  A struct of its own for the ragged instances, as RaggedConvArgs is (lg_extract.h)
struct AkDescribeRagged : AkDescribe { Ragged rg; };
template <> inline constexpr bool ragged<AkDescribeRagged> = true;
template <class D> __device__ __forceinline__ Frame frame_of_row(const D& d, int b) {
    if constexpr (ragged<D>) return frame_of(d.rg, b);
    else return Frame{d.H, d.W, d.L.Hp, d.L.Wp, d.pt, d.pl};
}

__device__ __forceinline__ void kp_pixel(const AkDescribe& d, const Frame& fr, int row, float& kw, float& kh) {   // (kpts / 2 + 0.5) * wh  (aliked.py:542)
    const float* k = d.knorm + 2LL * row;
    kw = __fmul_rn(__fadd_rn(__fdiv_rn(k[0], 2.f), 0.5f), (float)(fr.w - 1));
    kh = __fmul_rn(__fadd_rn(__fdiv_rn(k[1], 2.f), 0.5f), (float)(fr.h - 1));
}

// get_patches (aliked.py:48-64) of the normalised x1234 map: patch [row][tap = 3 dy + dx][128].  grid (rows), 4 waves: wave w takes taps w, w + 4, w + 8
template <class D>
__global__ __launch_bounds__(256) void ak_patch_kernel(D d) {
    const int row = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = row / d.N;
    const Frame fr = frame_of_row(d, b);
    float kw, kh;
    kp_pixel(d, fr, row, kw, kh);
    const long long lw = (long long)kw, lh = (long long)kh;                      // .long()
    int cx = (int)(long long)((float)lw - 1.5f + 1.f), cy = (int)(long long)((float)lh - 1.5f + 1.f);
    cx = min(max(cx, 0), fr.w - 1 - 3); cy = min(max(cy, 0), fr.h - 1 - 3);
    for (int t = wv; t < 9; t += 4) {
        const f32x2 v = x1234_norm(d.L, fr, b, cy + t / 3 + fr.pt, cx + t % 3 + fr.pl, lane);
        *reinterpret_cast<f32x2*>(d.patch + ((long long)row * 9 + t) * 128 + lane * 2) = v;
    }
}

// offset_conv.2 (1 x 1, bias) on the SELU'd first conv, clamp, sample positions in map pixels (grid_sample's un-normalisation).  thread = keypoint row
template <class D>
__global__ __launch_bounds__(256) void ak_offsets_kernel(D d, int rows) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const int C2 = 2 * d.np;
    const float* o1 = d.off1 + (long long)row * C2;
    const Frame fr = frame_of_row(d, row / d.N);
    const float mo = (float)max(fr.h, fr.w) / 4.f;
    float kw, kh;
    kp_pixel(d, fr, row, kw, kh);
    const float wm1 = (float)(fr.w - 1), hm1 = (float)(fr.h - 1);
    for (int p = 0; p < d.np; ++p) {
        float ox = d.b_off2[p], oy = d.b_off2[d.np + p];
        for (int i = 0; i < C2; ++i) {
            ox = __builtin_fmaf(d.w_off2[p * C2 + i], o1[i], ox);
            oy = __builtin_fmaf(d.w_off2[(d.np + p) * C2 + i], o1[i], oy);
        }
        ox = fminf(fmaxf(ox, -mo), mo); oy = fminf(fmaxf(oy, -mo), mo);
        const float gx = __fsub_rn(__fdiv_rn(__fmul_rn(2.f, __fadd_rn(kw, ox)), wm1), 1.f);   // 2 pos / wh - 1
        const float gy = __fsub_rn(__fdiv_rn(__fmul_rn(2.f, __fadd_rn(kh, oy)), hm1), 1.f);
        d.spos[((long long)row * d.np + p) * 2] = __fmul_rn(__fdiv_rn(__fadd_rn(gx, 1.f), 2.f), wm1);
        d.spos[((long long)row * d.np + p) * 2 + 1] = __fmul_rn(__fdiv_rn(__fadd_rn(gy, 1.f), 2.f), hm1);
    }
}

// bilinear sample (align_corners=True, zeros outside the unpadded map) of the normalised x1234 at every position: feat [row * np + p][128].  wave = one sample
template <class D>
__global__ __launch_bounds__(256) void ak_sample_kernel(D d, int samples) {
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= samples) return;
    const int b = (s / d.np) / d.N;
    const Frame fr = frame_of_row(d, b);
    const float ix = d.spos[2LL * s], iy = d.spos[2LL * s + 1];
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float ex = fx + 1.f, ey = fy + 1.f;
    const float wgt[4] = {(ex - ix) * (ey - iy), (ix - fx) * (ey - iy), (ex - ix) * (iy - fy), (ix - fx) * (iy - fy)};   // nw ne sw se
    f32x2 acc = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + (k & 1), y = y0 + (k >> 1);
        if (x >= 0 && x < fr.w && y >= 0 && y < fr.h) {      // wave-uniform
            const f32x2 v = x1234_norm(d.L, fr, b, y + fr.pt, x + fr.pl, lane);
            acc += wgt[k] * v;
        }
    }
    *reinterpret_cast<f32x2*>(d.feat + (long long)s * 128 + lane * 2) = acc;
}

// F.normalize of the aggregated descriptors -> out [B][N][128] (fp32, or the same values as binary16); rows >= count are zero.  wave = one row
__global__ __launch_bounds__(256) void ak_desc_norm_kernel(AkDescribe d, int rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int b = row / d.N, i = row - b * d.N;
    f32x2 v = *reinterpret_cast<const f32x2*>(d.draw + (long long)row * 128 + lane * 2);
    const float nrm = fmaxf(sqrtf(wave_sum(v[0] * v[0] + v[1] * v[1])), 1e-12f);
    v = i < d.counts[b] ? f32x2{v[0] / nrm, v[1] / nrm} : f32x2{0.f, 0.f};
    if (d.out_f16) {
        typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<f16x2*>(reinterpret_cast<f16_t*>(d.out) + (long long)row * 128 + lane * 2) = f16x2{(f16_t)v[0], (f16_t)v[1]};
    } else {
        *reinterpret_cast<f32x2*>(d.out + (long long)row * 128 + lane * 2) = v;
    }
}

// ==================================================================================================== host-side layouts
// packed weights (float offsets)
struct PackLayout {
    long long b1c1_w, b1c1_b, b1c2_w, b1c2_b;
    long long b2c1_w, b2c1_b, b2c2_w, b2c2_b, b2ds_w;
    struct Dcn { long long off1_w, off1_b, reg1_w, reg1_b, off2_w, off2_b, reg2_w, reg2_b, ds_w; } b3, b4;
    long long cv[4], sh0, sh2, sh4, sh6, so0_w, so0_b, so2_w, so2_b, sf, agg;
    long long total;
};
PackLayout pack_layout(int np) {
    PackLayout P{};
    long long n = 0;
    auto t = [&](long long f) { const long long o = n; n += (f + 63) / 64 * 64; return o; };
    P.b1c1_w = t(9 * 3 * 16); P.b1c1_b = t(16); P.b1c2_w = t(9 * 16 * 16); P.b1c2_b = t(16);
    P.b2c1_w = t(9 * 32 * 16); P.b2c1_b = t(32); P.b2c2_w = t(9 * 32 * 32); P.b2c2_b = t(32); P.b2ds_w = t(32 * 16);
    auto dcn = [&](PackLayout::Dcn& D, int ci, int co) {
        D.off1_w = t(9 * 18 * ci); D.off1_b = t(18); D.reg1_w = t((long long)co * 9 * ci); D.reg1_b = t(co);
        D.off2_w = t(9 * 18 * co); D.off2_b = t(18); D.reg2_w = t((long long)co * 9 * co); D.reg2_b = t(co); D.ds_w = t((long long)co * ci);
    };
    dcn(P.b3, 32, 64); dcn(P.b4, 64, 128);
    const int cin[4] = {16, 32, 64, 128};
    for (int i = 0; i < 4; ++i) P.cv[i] = t(32 * cin[i]);
    P.sh0 = t(8 * 128); P.sh2 = t(4 * 8 * 9); P.sh4 = t(4 * 4 * 9); P.sh6 = t(4 * 9);
    P.so0_w = t((long long)2 * np * 9 * 128); P.so0_b = t(2 * np); P.so2_w = t(4LL * np * np); P.so2_b = t(2 * np);
    P.sf = t(128 * 128); P.agg = t((long long)np * 128 * 128);
    P.total = n;
    return P;
}

// level maps x1 .. x4 (32 channels each), one buffer
struct LevelLayout { long long x[4]; long long total; };
LevelLayout level_layout(int B, int h, int w) {
    const Frame D = frame_of(h, w);
    Bump bp; LevelLayout L{};
    for (int l = 0; l < 4; ++l) L.x[l] = bp.take((long long)B * (D.Hp >> lvl_shift(l)) * (D.Wp >> lvl_shift(l)) * 32 * 4);
    L.total = bp.used;
    return L;
}

struct EncodeLayout { long long full_a, full_b, p2, q2, r2, p3, off, cols, t3, r3, p4, t4, r4, padded; long long total; };
EncodeLayout encode_layout(int B, int h, int w) {
    const Frame D = frame_of(h, w);
    const long long f = (long long)B * D.Hp * D.Wp, f2 = f / 4, f8 = f / 64, f32 = f / 1024;
    Bump bp; EncodeLayout E{};
    E.full_a = bp.take(f * 16 * 4); E.full_b = bp.take(f * 16 * 4);   // block1 (later: score head 8 + 4 channels, and 4 channels)
    E.p2 = bp.take(f2 * 16 * 4); E.q2 = bp.take(f2 * 32 * 4); E.r2 = bp.take(f2 * 32 * 4);
    E.p3 = bp.take(f8 * 32 * 4); E.off = bp.take(f8 * 18 * 4); E.cols = bp.take(f8 * 9 * 64 * 4); E.t3 = bp.take(f8 * 64 * 4); E.r3 = bp.take(f8 * 64 * 4);
    E.p4 = bp.take(f32 * 64 * 4); E.t4 = bp.take(f32 * 128 * 4); E.r4 = bp.take(f32 * 128 * 4);
    E.padded = bp.take((long long)B * 2 * 4);                         // ragged: the padded sizes (Wp_b, Hp_b) of RaggedConvArgs
    E.total = bp.used;
    return E;
}

struct DescribeLayout { long long patch, off1, spos, feat, sf, draw; long long total; int rows_pad; };
DescribeLayout describe_layout(int rows, int np) {
    const int rp = (rows + 31) / 32 * 32;
    Bump bp; DescribeLayout L{};
    L.rows_pad = rp;
    L.patch = bp.take((long long)rp * 9 * 128 * 4); L.off1 = bp.take((long long)rp * 2 * np * 4); L.spos = bp.take((long long)rp * np * 2 * 4);
    L.feat = bp.take((long long)rp * np * 128 * 4); L.sf = bp.take((long long)rp * np * 128 * 4); L.draw = bp.take((long long)rp * 128 * 4);
    L.total = bp.used;
    return L;
}

constexpr int kTensors = 68;
constexpr long long kMaxPixels = 1LL << 25;

int fold(const float* src, float* dst, float* bias_dst, int cout, int cin, int kk, int mode, const float* const* bn, const float* cbias, const float* extra,
         hipStream_t s) {
    return launch_fold(src, dst, bias_dst, cout, cin, kk, mode, bn, cbias, extra, s) == hipSuccess ? LG_OK : set_error(LG_ERR_HIP, "ALIKED weight packing launch failed");
}

int check_model(int np) { return (np == 16 || np == 32) ? LG_OK : set_error(LG_ERR_INVALID, "unknown ALIKED model: n_pos must be 16 (aliked-n16, -n16rot) or 32 (aliked-n32)"); }
int check_size(int B, int h, int w) {
    if (B < 1 || h < 8 || w < 8) return set_error(LG_ERR_INVALID, "ALIKED: batch >= 1 and images of at least 8 x 8 pixels");
    const Frame D = frame_of(h, w);
    if ((long long)D.Hp * D.Wp >= kMaxPixels) return set_error(LG_ERR_INVALID, "ALIKED: the padded image must stay below 2^25 pixels (32-bit pixel indices)");
    return LG_OK;
}

}  // namespace
}  // namespace lg

using namespace lg;

extern "C" {

int64_t lg_aliked_packed_bytes(int32_t n_pos) { return check_model(n_pos) == LG_OK ? pack_layout(n_pos).total * 4 : 0; }

int lg_aliked_pack_weights(int32_t n_pos, const float* const* t, int32_t n_tensors, void* packed, int64_t packed_bytes, void* hip_stream) {
    if (int rc = check_model(n_pos)) return rc;
    if (!t || !packed || n_tensors != kTensors) return set_error(LG_ERR_INVALID, "lg_aliked_pack_weights: 68 state tensors (state-dict order, without num_batches_tracked)");
    for (int i = 0; i < kTensors; ++i) if (!t[i]) return set_error(LG_ERR_INVALID, "lg_aliked_pack_weights: null tensor");
    const PackLayout P = pack_layout(n_pos);
    if (packed_bytes < P.total * 4) return set_error(LG_ERR_INVALID, "lg_aliked_pack_weights: buffer smaller than lg_aliked_packed_bytes");
    float* o = static_cast<float*>(packed);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    int rc = LG_OK;
    auto F = [&](int i, long long w, long long b, int co, int ci, int kk, int mode, int bn, int cbias, int extra) {
        if (rc) return;
        rc = fold(t[i], o + w, b >= 0 ? o + b : nullptr, co, ci, kk, mode, bn >= 0 ? t + bn : nullptr, cbias >= 0 ? t[cbias] : nullptr, extra >= 0 ? t[extra] : nullptr, s);
    };
    // state-dict order: block1 0-9, block2 10-21, block3 22-37, block4 38-53, conv1-4 54-57, score_head 58-61, desc_head 62-67
    F(0, P.b1c1_w, P.b1c1_b, 16, 3, 9, PK_TAP_CI_CO, 1, -1, -1);
    F(5, P.b1c2_w, P.b1c2_b, 16, 16, 9, PK_TAP_CO_CI, 6, -1, -1);
    F(10, P.b2c1_w, P.b2c1_b, 32, 16, 9, PK_TAP_CO_CI, 11, -1, -1);
    F(15, P.b2c2_w, P.b2c2_b, 32, 32, 9, PK_TAP_CO_CI, 16, -1, 21);    // + downsample bias
    F(20, P.b2ds_w, -1, 32, 16, 1, PK_TAP_CO_CI, -1, -1, -1);
    auto dcn = [&](int i0, const PackLayout::Dcn& D, int ci, int co) {
        F(i0, D.off1_w, D.off1_b, 18, ci, 9, PK_TAP_CO_CI, -1, i0 + 1, -1);
        F(i0 + 2, D.reg1_w, D.reg1_b, co, ci, 9, PK_CO_TAP_CI, i0 + 3, -1, -1);
        F(i0 + 7, D.off2_w, D.off2_b, 18, co, 9, PK_TAP_CO_CI, -1, i0 + 8, -1);
        F(i0 + 9, D.reg2_w, D.reg2_b, co, co, 9, PK_CO_TAP_CI, i0 + 10, -1, i0 + 15);
        F(i0 + 14, D.ds_w, -1, co, ci, 1, PK_TAP_CO_CI, -1, -1, -1);
    };
    dcn(22, P.b3, 32, 64);
    dcn(38, P.b4, 64, 128);
    const int cin[4] = {16, 32, 64, 128};
    for (int i = 0; i < 4; ++i) F(54 + i, P.cv[i], -1, 32, cin[i], 1, PK_TAP_CO_CI, -1, -1, -1);
    F(58, P.sh0, -1, 8, 128, 1, PK_COPY, -1, -1, -1);
    F(59, P.sh2, -1, 4, 8, 9, PK_COPY, -1, -1, -1);
    F(60, P.sh4, -1, 4, 4, 9, PK_COPY, -1, -1, -1);
    F(61, P.sh6, -1, 1, 4, 9, PK_COPY, -1, -1, -1);
    F(62, P.so0_w, P.so0_b, 2 * n_pos, 128, 9, PK_CO_TAP_CI, -1, 63, -1);
    F(64, P.so2_w, P.so2_b, 2 * n_pos, 2 * n_pos, 1, PK_COPY, -1, 65, -1);
    F(66, P.sf, -1, 128, 128, 1, PK_TAP_CO_CI, -1, -1, -1);
    F(67, P.agg, -1, 128, n_pos * 128, 1, PK_AGG, -1, -1, -1);
    return rc;
}

int64_t lg_aliked_levels_bytes(int32_t batch, int32_t h, int32_t w) { return check_size(batch, h, w) == LG_OK ? level_layout(batch, h, w).total : 0; }
int64_t lg_aliked_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t n_pos) {
    if (check_model(n_pos) != LG_OK || check_size(batch, h, w) != LG_OK) return 0;
    return encode_layout(batch, h, w).total;
}

}  // extern "C"

// lg_aliked_encode: one sequence of launches; with LG_EXTRACT_RAGGED every launch is the Ragged instance and h, w are the canvas
template <class R>
static int aliked_encode(const lg_aliked_encode_io& io, hipStream_t s) {
    constexpr bool RG = ragged<R>;
    const int B = io.batch, h = io.h, w = io.w;
    if (int rc = check_model(io.n_pos)) return rc;
    if (int rc = check_size(B, h, w)) return rc;
    if (io.channels != 1 && io.channels != 3) return set_error(LG_ERR_INVALID, "ALIKED: images of 1 or 3 channels");
    if (!io.image || !io.packed || !io.levels || !io.workspace || !io.scores) return set_error(LG_ERR_INVALID, "null pointer");
    const EncodeLayout E = encode_layout(B, h, w);
    if (io.workspace_bytes < E.total) return set_error(LG_ERR_INVALID, "workspace too small (lg_aliked_workspace_bytes)");
    const PackLayout P = pack_layout(io.n_pos);
    const LevelLayout LL = level_layout(B, h, w);
    const Frame D = frame_of(h, w);
    const int Hp = D.Hp, Wp = D.Wp, H2 = Hp / 2, W2 = Wp / 2, H8 = Hp / 8, W8 = Wp / 8, H32 = Hp / 32, W32 = Wp / 32;
    const float* p = static_cast<const float*>(io.packed);
    char* ws = static_cast<char*>(io.workspace);
    char* lv = static_cast<char*>(io.levels);
    auto W_ = [&](long long off) { return reinterpret_cast<float*>(ws + off); };
    float* x[4];
    for (int l = 0; l < 4; ++l) x[l] = reinterpret_cast<float*>(lv + LL.x[l]);
    const long long f = (long long)B * Hp * Wp;
    // the geometry argument of every launch at pyramid shift `sh`, and the convolution on that level
    int* padded = reinterpret_cast<int*>(ws + E.padded);
    auto G = [&](int sh) { if constexpr (RG) return Ragged{io.sizes, h, w, sh}; else return Uniform{}; };
    if constexpr (RG) hipLaunchKernelGGL(ak_padded_sizes_kernel, dim3(blocks(B)), dim3(256), 0, s, G(0), B, padded);
    auto conv = [&](int sh, auto... args) { if constexpr (RG) lg::conv(padded, sh, args...); else lg::conv(args...); };
    // ---- block1 (ConvBlock) at full resolution
    hipLaunchKernelGGL(ak_conv_first_kernel<R>, dim3(blocks(f * 4)), dim3(256), 0, s, io.image, io.channels, h, w, Hp, Wp, D.pt, D.pl, p + P.b1c1_w, p + P.b1c1_b, W_(E.full_a), B, G(0));
    conv(0, W_(E.full_a), p + P.b1c2_w, p + P.b1c2_b, W_(E.full_b), B, Hp, Wp, 16, 16, 9, 1, s);
    conv(0, W_(E.full_b), p + P.cv[0], nullptr, x[0], B, Hp, Wp, 16, 32, 1, 1, s);                  // conv1 + SELU -> x1
    // ---- block2 (ResBlock) at 1/2
    hipLaunchKernelGGL(ak_pool_kernel<R>, dim3(blocks(f / 4 * 4)), dim3(256), 0, s, W_(E.full_b), W_(E.p2), B, Hp, Wp, 16, 2, G(0));
    conv(1, W_(E.p2), p + P.b2c1_w, p + P.b2c1_b, W_(E.q2), B, H2, W2, 16, 32, 9, 1, s);
    conv(1, W_(E.q2), p + P.b2c2_w, p + P.b2c2_b, W_(E.r2), B, H2, W2, 32, 32, 9, 1, s, W_(E.p2), p + P.b2ds_w, 16);
    conv(1, W_(E.r2), p + P.cv[1], nullptr, x[1], B, H2, W2, 32, 32, 1, 1, s);                      // conv2 -> x2
    // ---- blocks 3 and 4 (deformable ResBlocks) at 1/8 and 1/32
    auto dcn_block = [&](const PackLayout::Dcn& Dc, const float* in, float* t, float* out, int hh, int ww, int sh, int ci, int co) {
        const float mo = (float)max(hh, ww) / 4.f;      // (ragged: the kernel takes it from the image's level extent)
        const long long px = (long long)B * hh * ww;
        conv(sh, in, p + Dc.off1_w, p + Dc.off1_b, W_(E.off), B, hh, ww, ci, 18, 9, 0, s);
        hipLaunchKernelGGL(ak_deform_gather_kernel<R>, dim3(blocks(px * 9 * (ci / 4))), dim3(256), 0, s, in, W_(E.off), W_(E.cols), B, hh, ww, ci, mo, G(sh));
        conv(sh, W_(E.cols), p + Dc.reg1_w, p + Dc.reg1_b, t, B, hh, ww, 9 * ci, co, 1, 1, s);
        conv(sh, t, p + Dc.off2_w, p + Dc.off2_b, W_(E.off), B, hh, ww, co, 18, 9, 0, s);
        hipLaunchKernelGGL(ak_deform_gather_kernel<R>, dim3(blocks(px * 9 * (co / 4))), dim3(256), 0, s, t, W_(E.off), W_(E.cols), B, hh, ww, co, mo, G(sh));
        conv(sh, W_(E.cols), p + Dc.reg2_w, p + Dc.reg2_b, out, B, hh, ww, 9 * co, co, 1, 1, s, in, p + Dc.ds_w, ci);
    };
    hipLaunchKernelGGL(ak_pool_kernel<R>, dim3(blocks(f / 64 * 8)), dim3(256), 0, s, W_(E.r2), W_(E.p3), B, H2, W2, 32, 4, G(1));
    dcn_block(P.b3, W_(E.p3), W_(E.t3), W_(E.r3), H8, W8, 3, 32, 64);
    conv(3, W_(E.r3), p + P.cv[2], nullptr, x[2], B, H8, W8, 64, 32, 1, 1, s);                      // conv3 -> x3
    hipLaunchKernelGGL(ak_pool_kernel<R>, dim3(blocks(f / 1024 * 16)), dim3(256), 0, s, W_(E.r3), W_(E.p4), B, H8, W8, 64, 4, G(3));
    dcn_block(P.b4, W_(E.p4), W_(E.t4), W_(E.r4), H32, W32, 5, 64, 128);
    conv(5, W_(E.r4), p + P.cv[3], nullptr, x[3], B, H32, W32, 128, 32, 1, 1, s);                  // conv4 -> x4
    // ---- score head on x1234 (never materialised) -> scores [B][h][w]
    AkLevels L{{x[0], x[1], x[2], x[3]}, B, Hp, Wp};
    float* s8 = W_(E.full_a);                  // [f][8]
    float* s4a = W_(E.full_b);                 // [f][4]
    float* s4b = W_(E.full_a) + f * 8;         // [f][4]
    hipLaunchKernelGGL(ak_score_head0_kernel<R>, dim3(blocks(f)), dim3(256), 0, s, L, p + P.sh0, s8, G(0));
    hipLaunchKernelGGL((ak_small_conv_kernel<8, 4, false, R>), dim3(blocks(f)), dim3(256), 0, s, s8, p + P.sh2, s4a, B, Hp, Wp, h, w, D.pt, D.pl, G(0));
    hipLaunchKernelGGL((ak_small_conv_kernel<4, 4, false, R>), dim3(blocks(f)), dim3(256), 0, s, s4a, p + P.sh4, s4b, B, Hp, Wp, h, w, D.pt, D.pl, G(0));
    hipLaunchKernelGGL((ak_small_conv_kernel<4, 1, true, R>), dim3(blocks((long long)B * h * w)), dim3(256), 0, s, s4b, p + P.sh6, io.scores, B, Hp, Wp, h, w, D.pt, D.pl, G(0));
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? LG_OK : set_error(LG_ERR_HIP, hipGetErrorString(e));
}

// lg_aliked_describe: one path, the element type of `descriptors` decided at the last kernel's store (LG_EXTRACT_DESC_F16); DA = AkDescribeRagged with LG_EXTRACT_RAGGED
template <class DA>
static int aliked_describe(const lg_aliked_describe_io& io, hipStream_t s) {
    const int n = io.n, n_pos = io.n_pos;
    if (int rc = check_model(n_pos)) return rc;
    if (int rc = check_size(io.batch, io.h, io.w)) return rc;
    if (n < 1) return LG_OK;
    if (n > 20000) return set_error(LG_ERR_INVALID, "ALIKED: more than 20000 keypoints per image");
    if (!io.levels || !io.packed || !io.kp_norm || !io.counts || !io.workspace || !io.descriptors) return set_error(LG_ERR_INVALID, "null pointer");
    const int rows = io.batch * n;
    const DescribeLayout DL = describe_layout(rows, n_pos);
    if (io.workspace_bytes < DL.total) return set_error(LG_ERR_INVALID, "workspace too small (lg_aliked_describe_workspace_bytes)");
    const PackLayout P = pack_layout(n_pos);
    const LevelLayout LL = level_layout(io.batch, io.h, io.w);
    const Frame D = frame_of(io.h, io.w);
    const float* p = static_cast<const float*>(io.packed);
    const char* lv = static_cast<const char*>(io.levels);
    char* ws = static_cast<char*>(io.workspace);
    DA d{};
    if constexpr (ragged<DA>) d.rg = Ragged{io.sizes, io.h, io.w, 0};
    for (int l = 0; l < 4; ++l) d.L.x[l] = reinterpret_cast<const float*>(lv + LL.x[l]);
    d.L.B = io.batch; d.L.Hp = D.Hp; d.L.Wp = D.Wp;
    d.H = io.h; d.W = io.w; d.pt = D.pt; d.pl = D.pl; d.N = n; d.np = n_pos; d.knorm = io.kp_norm;
    d.patch = reinterpret_cast<float*>(ws + DL.patch); d.off1 = reinterpret_cast<float*>(ws + DL.off1); d.spos = reinterpret_cast<float*>(ws + DL.spos);
    d.feat = reinterpret_cast<float*>(ws + DL.feat); d.sf = reinterpret_cast<float*>(ws + DL.sf); d.draw = reinterpret_cast<float*>(ws + DL.draw);
    d.w_off2 = p + P.so2_w; d.b_off2 = p + P.so2_b; d.counts = io.counts; d.out = static_cast<float*>(io.descriptors);
    d.out_f16 = (io.flags & LG_EXTRACT_DESC_F16) ? 1 : 0;
    const int rp = DL.rows_pad;
    hipLaunchKernelGGL(ak_patch_kernel<DA>, dim3(rows), dim3(256), 0, s, d);
    if (rp > rows) (void)hipMemsetAsync(d.patch + (long long)rows * 9 * 128, 0, (size_t)(rp - rows) * 9 * 128 * 4, s);   // GEMM pad rows: keep them finite
    gemm(d.patch, p + P.so0_w, p + P.so0_b, d.off1, rp, 9 * 128, 2 * n_pos, 1, s);            // offset_conv.0 + SELU
    hipLaunchKernelGGL(ak_offsets_kernel<DA>, dim3(blocks(rows)), dim3(256), 0, s, d, rows);
    hipLaunchKernelGGL(ak_sample_kernel<DA>, dim3(blocks((long long)rows * n_pos, 4)), dim3(256), 0, s, d, rows * n_pos);
    if (rp > rows) (void)hipMemsetAsync(d.feat + (long long)rows * n_pos * 128, 0, (size_t)(rp - rows) * n_pos * 128 * 4, s);
    gemm(d.feat, p + P.sf, nullptr, d.sf, rp * n_pos, 128, 128, 1, s);                        // sf_conv + SELU
    gemm(d.sf, p + P.agg, nullptr, d.draw, rp, n_pos * 128, 128, 0, s);                      // einsum("ncp,pcd->nd")
    hipLaunchKernelGGL(ak_desc_norm_kernel, dim3(blocks(rows, 4)), dim3(256), 0, s, static_cast<const AkDescribe&>(d), rows);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? LG_OK : set_error(LG_ERR_HIP, hipGetErrorString(e));
}

extern "C" {

int lg_aliked_encode(const lg_aliked_encode_io* io, void* hip_stream) {
    if (int rc = check_extract_io(io, LG_EXTRACT_RAGGED, "lg_aliked_encode")) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return !(io->flags & LG_EXTRACT_RAGGED) ? aliked_encode<Uniform>(*io, s) : aliked_encode<Ragged>(*io, s);
}

int64_t lg_aliked_detect_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t capacity) {
    if (check_size(batch, h, w) != LG_OK || capacity < 1) return 0;
    return detect_layout(batch, h, w, h * w, capacity, true).total;
}

// one path; with LG_EXTRACT_RAGGED `sizes` (DetectArgs::sizes) makes every bound the image's
int lg_aliked_detect(const lg_aliked_detect_io* io, void* hip_stream) {
    if (int rc = check_extract_io(io, LG_EXTRACT_RAGGED, "lg_aliked_detect")) return rc;
    const lg_aliked_detect_io& i = *io;
    if (int rc = check_size(i.batch, i.h, i.w)) return rc;
    if (i.nms_radius < 1 || i.nms_radius > 8) return set_error(LG_ERR_INVALID, "ALIKED: nms_radius must be in [1, 8]");
    if (i.n_limit > 20000 || i.top_k > 20000) return set_error(LG_ERR_INVALID, "ALIKED: n_limit / top_k above 20000 (ALIKED.n_limit_max)");
    if (i.top_k <= 0 && i.n_limit < 1) return set_error(LG_ERR_INVALID, "ALIKED: threshold mode needs n_limit >= 1");
    const int K = i.top_k > 0 ? i.top_k : i.n_limit;
    if (i.capacity < K) return set_error(LG_ERR_INVALID, "ALIKED: capacity must be at least top_k / n_limit");
    if (!i.scores || !i.workspace || !i.keypoints || !i.kp_scores || !i.kp_norm || !i.counts) return set_error(LG_ERR_INVALID, "null pointer");
    const DetectLayout DL = detect_layout(i.batch, i.h, i.w, i.h * i.w, i.capacity, true);
    if (i.workspace_bytes < DL.total) return set_error(LG_ERR_INVALID, "workspace too small (lg_aliked_detect_workspace_bytes)");
    DetectArgs a{};
    detect_bind(a, DL, i.workspace);
    a.S = i.scores; a.B = i.batch; a.H = i.h; a.W = i.w; a.radius = i.nms_radius; a.sizes = extract_sizes(i);
    a.border = i.nms_radius; a.image_size = i.image_size; a.border_value = 0.f; a.threshold = i.scores_th;
    a.max_candidates = i.h * i.w; a.K = K; a.sort_always = i.top_k > 0; a.sel_cap = i.capacity;
    double* rowsum = reinterpret_cast<double*>(static_cast<char*>(i.workspace) + DL.rowsum);
    float* th = reinterpret_cast<float*>(static_cast<char*>(i.workspace) + DL.th);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    launch_nms(a, s);                               // simple_nms (aliked.py:69-91)
    launch_row_count(a, nullptr, rowsum, s);        // against scores_th, and the row sums for the mean
    hipLaunchKernelGGL(ak_decide_kernel, dim3(i.batch), dim3(256), 0, s, a, i.top_k, (const double*)rowsum, th);
    launch_row_count(a, th, nullptr, s);
    launch_compact(a, th, s);
    launch_select(a, s);
    hipLaunchKernelGGL(ak_refine_kernel, dim3(blocks(i.capacity), i.batch), dim3(256), 0, s, a, AkKeypoints{i.keypoints, i.kp_scores, i.kp_norm, i.counts});
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? LG_OK : set_error(LG_ERR_HIP, hipGetErrorString(e));
}

int64_t lg_aliked_describe_workspace_bytes(int32_t rows, int32_t n_pos) {
    if (check_model(n_pos) != LG_OK || rows < 1) return 0;
    return describe_layout(rows, n_pos).total;
}

int lg_aliked_describe(const lg_aliked_describe_io* io, void* hip_stream) {
    if (int rc = check_extract_io(io, LG_EXTRACT_RAGGED | LG_EXTRACT_DESC_F16, "lg_aliked_describe")) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return !(io->flags & LG_EXTRACT_RAGGED) ? aliked_describe<AkDescribe>(*io, s) : aliked_describe<AkDescribeRagged>(*io, s);
}

}  // extern "C"
