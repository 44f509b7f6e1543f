// lightglue_amd — SuperPoint conv stack on the MI355X (the producer of the matcher's inputs):
//   ref superpoint.py:127-141 (layers) and :159-184, :213-214 (forward): shared VGG-style encoder (8 x conv3x3 + ReLU, 3 x
//   maxpool 2x2), keypoint head (conv3x3 + ReLU, conv1x1 -> 65 logits, softmax, drop the dustbin, depth-to-space 8x8) and
//   descriptor head (conv3x3 + ReLU, conv1x1 -> 256 channels; L2 normalisation + sampling live in lg_superpoint.hip).
// Arithmetic is EXACT fp32 (v_mfma_f32_16x16x4_f32): the detector thresholds / NMS-compares the scores, so they must
// agree with an fp32 convolution to round-off; the f32 MFMA rate (157 TFLOP/s) is not the limiter of this stage.
//
// The fp32 convolutions run launch_conv (lg_extract.hip, shared with ALIKED); this file holds the split-f16 forms, which end in the same
// epilogue (conv_epilogue, lg_extract.h).
#include <string>

#include "lg_extract.h"
#include "../../include/lightglue_amd.h"

namespace lg {

// The 1 x 1 layers of the split-f16 form (conv_precision "f16x3", opt-in: convPb, convDb): the implicit GEMM of launch_conv on split-f16 operands —
// activations split into hi + lo f16 planes in registers (x = hi + lo, 22 bits), weights pre-split by lg_sp_pack_conv_weight_split ([2 planes][cout][cin]
// f16, the bytes of the fp32 array), three v_mfma_f32_16x16x32_f16 per product with fp32 accumulation (hi lo + lo hi + hi hi; the dropped lo lo term is
// 2^-24-class, below the fp32 convolution's own summation-order noise over K = 576 ... 1152).  One MFMA chunk = 32 input channels: lane (lr, g) supplies
// pixel lr / cout lr and the 8 consecutive channels 8g .. 8g + 7 (two 16-byte fp32 loads per activation fragment, one 16-byte load per weight plane).
// Same tiles (64 output channels per wave), epilogue and layouts as the fp32 form.  Measured on the 3 x 3 layers before they moved to the LDS-staged
// kernel below (profiles/r06sp_*): 1.2 x the fp32 form, not the 5 x of the MFMA rates — with 16 KB of operand loads per 48 MFMAs and no LDS staging the
// kernel is bound by its loads and their address / split arithmetic, whatever the matrix instruction costs.
// A = RaggedConvArgs (both split kernels, as in conv_kernel): strides from the canvas a.H / a.W, every bound from the image extent; the uniform instances are the code they were.
template <class A>
__global__ __launch_bounds__(256) void sp_conv1x1_split_kernel(A a) {
    constexpr bool RAGGED = is_ragged<A>;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, g = lane >> 4;
    const int ngroups = (a.Cout + 63) >> 6;
    const int b = blockIdx.z / ngroups, n0 = (blockIdx.z - b * ngroups) << 6;
    const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 8 + wv * 2;
    const ConvExtent e = conv_extent(a, b);
    if (y0 >= ext_h<RAGGED>(a, e)) return;
    if constexpr (RAGGED) { if (x0 >= e.w) return; }
    f32x4 acc[4][4];   // [mt = ry*2 + xt][nt]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* inb = a.in + (long long)b * a.H * a.W * a.Cin;
    const int nchunk = a.Cin >> 5;
    const long long wplane = (long long)a.Cout * a.Cin;        // f16 elements from the hi to the lo weight plane
    const int ntl = min(4, (a.Cout - n0 + 15) >> 4);          // live n-tiles of this channel group (wave-uniform)
    // pixel of every m-tile (clamped; `ok` = inside the image)
    long long poff[4]; bool ok[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int yy = y0 + (mt >> 1), xx = x0 + (mt & 1) * 16 + lr;
        ok[mt] = yy < ext_h<RAGGED>(a, e) && xx < ext_w<RAGGED>(a, e);
        const int yc = min(yy, ext_h<RAGGED>(a, e) - 1), xc = min(xx, ext_w<RAGGED>(a, e) - 1);
        poff[mt] = ((long long)yc * a.W + xc) * a.Cin + 8 * g;
    }
    long long wrow[4];   // weight row of every n-tile, in elements (clamped into the matrix; dead lanes are zeroed after the load)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) wrow[nt] = (long long)min(n0 + nt * 16 + lr, a.Cout - 1) * a.Cin + 8 * g;
    const f16_t* wh = static_cast<const f16_t*>(a.w);
    for (int c = 0; c < nchunk; ++c) {
        u32x4 ah[4], al[4], bh[4], bl[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const float* src = inb + poff[mt] + c * 32;
            f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
            if (!ok[mt]) { v0 = f32x4{0.f, 0.f, 0.f, 0.f}; v1 = v0; }
            split8<TagF16>(v0, v1, ah[mt], al[mt]);
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const bool live = nt < ntl && n0 + nt * 16 + lr < a.Cout;
            const u32x4 h = *reinterpret_cast<const u32x4*>(wh + wrow[nt] + c * 32), l = *reinterpret_cast<const u32x4*>(wh + wplane + wrow[nt] + c * 32);
            bh[nt] = live ? h : u32x4{0u, 0u, 0u, 0u};
            bl[nt] = live ? l : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                mma_chunk<TagF16>(acc[mt][nt], ah[mt], bl[nt]);
                mma_chunk<TagF16>(acc[mt][nt], al[mt], bh[nt]);
                mma_chunk<TagF16>(acc[mt][nt], ah[mt], bh[nt]);
            }
    }
    conv_epilogue<4, RAGGED>(a, acc, b, n0, x0, y0, lr, g, e);
}

// ---- 3 x 3 convolutions of the split-f16 form, LDS-staged (conv_precision "f16x3": conv1b ... convPa / convDa; cin % 32 == 0, cout % 64 == 0).
// The register-only form is bound by its operand loads (PMC: matrix pipe 17 % busy at 1.7 waves per SIMD: every tap re-fetches its pixels from L2 and splits them
// again).  Here a workgroup (4 waves = 8 rows x 32 pixels x 64 output channels, as above) stages the (8 + 2) x (32 + 2) pixel halo tile of ONE 32-channel chunk in LDS —
// fetched once, split once into hi / lo f16 planes (43.5 KB), zero padding applied at staging — and the nine taps read their activation fragments from it (slot XOR pixel
// bits 1..2: two-way, the minimum for a 16-byte read); the next chunk's pixels are requested into registers before the taps run.  Weights arrive as in the matcher's tail
// kernel: pre-packed in MFMA-fragment order ([cout group][chunk][tap][n-tile][plane][lane][8 f16], lg_sp_pack_conv_weight_split with k = 3) and read by raw buffer loads
// one (chunk, tap) step ahead — one fully coalesced 1 KB wave load per fragment, no address arithmetic.  Two barriers per chunk (6 912 matrix cycles per wave).
constexpr int C3_HW = 34, C3_HH = 10, C3_NPX = C3_HW * C3_HH, C3_PLANE = C3_NPX * 64, C3_ITEMS = C3_NPX * 4, C3_ROUNDS = (C3_ITEMS + 255) / 256;
__device__ __forceinline__ int c3_off(int q, int slot) { return q * 64 + ((slot ^ ((q >> 1) & 3)) << 4); }

template <class A>
__global__ __launch_bounds__(256, 2) void sp_conv3x3_split_kernel(A a) {     // two workgroups per CU (<= 256 VGPRs, 43.5 KB of LDS each): at one wave per SIMD the launch is 20 % slower
    __shared__ __attribute__((aligned(16))) char smA[2 * C3_PLANE];
    constexpr bool RAGGED = is_ragged<A>;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, g = lane >> 4;
    const int ngroups = a.Cout >> 6;
    const int b = blockIdx.z / ngroups, grp = blockIdx.z - b * ngroups, n0 = grp << 6;
    const int x0 = blockIdx.x * 32, yt = blockIdx.y * 8, y0 = yt + wv * 2;
    const ConvExtent e = conv_extent(a, b);
    if constexpr (RAGGED) { if (yt >= e.h || x0 >= e.w) return; }     // tile origin outside the image: workgroup-uniform, before the first barrier
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* inb = a.in + (long long)b * a.H * a.W * a.Cin;
    const int nchunk = a.Cin >> 5, nsteps = nchunk * 9;
    const __amdgpu_buffer_rsrc_t wrs = weight_rsrc(static_cast<const char*>(a.w) + (long long)grp * nsteps * 8192);
    const int lane16 = lane * 16;
    // staging: item = (halo pixel q, 16-byte slot): 8 channels; thread tid takes items tid, tid + 256, ...  The coordinates are recomputed per use (a few VALU per
    // round against 432 MFMAs per chunk) instead of kept in 18 registers: the kernel has to fit 256 VGPRs for two workgroups per CU.
    auto item_of = [&](int r, int& q, int& slot, bool& inside, int& src_off) {
        const int item = min(tid + 256 * r, C3_ITEMS - 1);
        q = item >> 2; slot = item & 3;
        const int ry = q / C3_HW, rx = q - ry * C3_HW, yy = yt + ry - 1, xx = x0 + rx - 1;
        inside = yy >= 0 && yy < ext_h<RAGGED>(a, e) && xx >= 0 && xx < ext_w<RAGGED>(a, e);
        src_off = (min(max(yy, 0), ext_h<RAGGED>(a, e) - 1) * a.W + min(max(xx, 0), ext_w<RAGGED>(a, e) - 1)) * a.Cin + 8 * slot;      // (element offset inside one image: H W cin < 2^31 in the extractor's envelope)
    };
    f32x4 raw[C3_ROUNDS][2];
    auto stage_load = [&](int c) {
#pragma unroll
        for (int r = 0; r < C3_ROUNDS; ++r) {
            int q, slot, off; bool inside;
            item_of(r, q, slot, inside, off);
            const float* src = inb + off + c * 32;
            raw[r][0] = *reinterpret_cast<const f32x4*>(src); raw[r][1] = *reinterpret_cast<const f32x4*>(src + 4);
        }
    };
    auto stage_store = [&]() {
#pragma unroll
        for (int r = 0; r < C3_ROUNDS; ++r) {
            int q, slot, off; bool inside;
            item_of(r, q, slot, inside, off);
            const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
            u32x4 hi, lo;
            split8<TagF16>(inside ? raw[r][0] : z, inside ? raw[r][1] : z, hi, lo);
            if (tid + 256 * r < C3_ITEMS) {
                const int dst = c3_off(q, slot);
                *reinterpret_cast<u32x4*>(smA + dst) = hi;
                *reinterpret_cast<u32x4*>(smA + C3_PLANE + dst) = lo;
            }
        }
    };
    u32x4 wf[2][4][2];   // [ring][n-tile][plane]
    auto load_w = [&](u32x4 (&dst)[4][2], int step) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int p = 0; p < 2; ++p) dst[nt][p] = weight_frag(wrs, lane16, step * 8192 + (nt * 2 + p) * 1024);
    };
    stage_load(0);
    load_w(wf[0], 0);
    // chunks in PAIRS (cin = 64 / 128: 2 or 4 chunks): 18 steps per iteration, so that the two-deep weight ring's slot (step & 1) is a compile-time constant everywhere
    for (int c0 = 0; c0 < nchunk; c0 += 2) {
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int c = c0 + cc;
            stage_store();
            __syncthreads();                                   // the chunk's halo tile is complete
            stage_load(min(c + 1, nchunk - 1));                // next chunk's pixels, in flight under the nine taps (the last chunk re-fetches itself: never branched around)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int sl = (cc * 9 + tap) & 1;             // ring slot of this step's weights
                const int step = c * 9 + tap;
                load_w(wf[sl ^ 1], min(step + 1, nsteps - 1));
                const int dy = tap / 3, dx = tap % 3;         // halo coordinates: + 1 - 1
                u32x4 ah[4], al[4];
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const int q = (2 * wv + (mt >> 1) + dy) * C3_HW + (mt & 1) * 16 + lr + dx;
                    const int off = c3_off(q, g);
                    ah[mt] = *reinterpret_cast<const u32x4*>(smA + off);
                    al[mt] = *reinterpret_cast<const u32x4*>(smA + C3_PLANE + off);
                }
                __builtin_amdgcn_sched_barrier(0);
                const u32x4 (&w)[4][2] = wf[sl];
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        mma_chunk<TagF16>(acc[mt][nt], ah[mt], w[nt][1]);
                        mma_chunk<TagF16>(acc[mt][nt], al[mt], w[nt][0]);
                        mma_chunk<TagF16>(acc[mt][nt], ah[mt], w[nt][0]);
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();                                   // every wave is past its last read of the tile
        }
    }
    conv_epilogue<4, RAGGED>(a, acc, b, n0, x0, y0, lr, g, e);
}

// conv1a (ref :127, :159): 1 -> 64 channels, 3x3, pad 1, ReLU, image [B][1][H][W] -> NHWC.  K = 9: plain VALU.
// thread = (pixel, 4 output channels); weights packed [9][64] (tap-major) and read as float4.
// RAGGED: sizes [B][2] (w, h); H, W are then the canvas (strides), the image's h x w bounds the taps and the stores.
template <bool RAGGED>
__global__ __launch_bounds__(256) void sp_conv1a_kernel(const float* img, const float* w9x64, const float* bias, float* out, int B, int H, int W, const int* sizes) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)B * H * W * 16;
    if (idx >= total) return;
    const int c4 = (int)(idx & 15);
    const long long pix = idx >> 4;
    const int x = (int)(pix % W), y = (int)((pix / W) % H), b = (int)(pix / ((long long)W * H));
    int hi = H, wi = W;
    if constexpr (RAGGED) { wi = min(max(sizes[2 * b], 1), W); hi = min(max(sizes[2 * b + 1], 1), H); if (y >= hi || x >= wi) return; }
    f32x4 s = *reinterpret_cast<const f32x4*>(bias + c4 * 4);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        const float p = (yy >= 0 && yy < hi && xx >= 0 && xx < wi) ? img[((long long)b * H + yy) * W + xx] : 0.f;
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w9x64 + t * 64 + c4 * 4);
        s[0] = __builtin_fmaf(p, wv[0], s[0]); s[1] = __builtin_fmaf(p, wv[1], s[1]); s[2] = __builtin_fmaf(p, wv[2], s[2]); s[3] = __builtin_fmaf(p, wv[3], s[3]);
    }
    s[0] = fmaxf(s[0], 0.f); s[1] = fmaxf(s[1], 0.f); s[2] = fmaxf(s[2], 0.f); s[3] = fmaxf(s[3], 0.f);
    *reinterpret_cast<f32x4*>(out + pix * 64 + c4 * 4) = s;
}

// keypoint scores (ref :176-184): softmax over the 65 logits of a cell, drop the dustbin, depth-to-space: channel c of cell
// (i, j) -> pixel (8i + c / 8, 8j + c % 8).  One wave per cell.  sizes (ragged batch, else null): a cell outside image b's (h_b >> 3) x (w_b >> 3) has no logits:
// it writes 0, so that the score canvas is defined everywhere.
__global__ __launch_bounds__(256) void sp_scores_kernel(const float* logits, float* scores, int B, int h, int w, const int* sizes) {
    const int lane = threadIdx.x & 63;
    const long long cell = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= (long long)B * h * w) return;
    if (sizes) {     // (wave-uniform: one cell per wave)
        const int j = (int)(cell % w), i = (int)((cell / w) % h), b = (int)(cell / ((long long)w * h));
        if (i >= min(sizes[2 * b + 1] >> 3, h) || j >= min(sizes[2 * b] >> 3, w)) {
            scores[((long long)b * h * 8 + i * 8 + (lane >> 3)) * (w * 8) + j * 8 + (lane & 7)] = 0.f;
            return;
        }
    }
    const float* p = logits + cell * 65;
    const float v = p[lane], d = p[64];
    const float m = fmaxf(wave_max(v), d);
    const float e = expf(v - m), ed = expf(d - m);
    const float sum = wave_sum(e) + ed;
    const int j = (int)(cell % w), i = (int)((cell / w) % h), b = (int)(cell / ((long long)w * h));
    scores[((long long)b * h * 8 + i * 8 + (lane >> 3)) * (w * 8) + j * 8 + (lane & 7)] = e / sum;
}

// SPLIT form, hi = f16(w), lo = f16(w - hi).  1 x 1 layers: [2 planes][Cout][Cin] f16 (sp_conv1x1_split_kernel).  3 x 3 layers: MFMA-fragment order for
// sp_conv3x3_split_kernel, [cout group of 64][32-channel chunk][tap][n-tile][plane][lane = 16 g + lr][8 f16]: lane (lr, g) of n-tile nt holds cout 64 grp + 16 nt + lr,
// channels 32 c + 8 g .. + 7 — 1 KB per fragment, 8 KB per (chunk, tap) step.
__global__ __launch_bounds__(256) void sp_pack_weight_split_kernel(const float* src, f16_t* dst, int Cout, int Cin, int kk) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, total = (long long)Cout * Cin * kk;
    if (i >= total) return;
    const int t = (int)(i % kk), ci = (int)((i / kk) % Cin), co = (int)(i / ((long long)kk * Cin));
    const float w = src[i];
    const f16_t hi = (f16_t)w, lo = (f16_t)(w - (float)hi);
    if (kk == 9) {
        const int grp = co >> 6, nt = (co & 63) >> 4, lr = co & 15, c = ci >> 5, g = (ci & 31) >> 3, e = ci & 7, nchunk = Cin >> 5;
        const long long o = ((((long long)(grp * nchunk + c) * 9 + t) * 4 + nt) * 2) * 512 + (g * 16 + lr) * 8 + e;
        dst[o] = hi;
        dst[o + 512] = lo;
    } else {
        const long long o = ((long long)t * Cout + co) * Cin + ci;
        dst[o] = hi;
        dst[total + o] = lo;
    }
}

static hipError_t launch_sp_pack_weight_split(const float* src, void* dst, int Cout, int Cin, int k, hipStream_t s) {
    const long long total = (long long)Cout * Cin * k * k;
    hipLaunchKernelGGL(sp_pack_weight_split_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, static_cast<f16_t*>(dst), Cout, Cin, k * k);
    return hipGetLastError();
}

// repack a conv weight [Cout][Cin][k][k] -> [k*k][Cout][Cin] (conv1a: [9][64])
static hipError_t launch_sp_pack_weight(const float* src, float* dst, int Cout, int Cin, int k, hipStream_t s) {
    return launch_fold(src, dst, nullptr, Cout, Cin, k * k, PK_TAP_CO_CI, nullptr, nullptr, nullptr, s);
}

// H, W: this level's canvas; sizes (ragged batch, else null) / shift: the full-resolution (w, h) of every image and the level's halving
static void conv(bool split, const float* in, float* out, const float* w, const float* bias, int B, int H, int W, int Cin, int Cout, int taps, int relu, int pool,
                 int nchw, const int* sizes, int shift, hipStream_t s) {
    const ConvArgs a{in, w, bias, nullptr, nullptr, out, B, H, W, Cin, 0, Cout, taps, relu ? ACT_RELU : ACT_NONE, pool, nchw};
    const RaggedConvArgs ra{a, sizes, shift};
    const dim3 grid((W + 31) / 32, (H + 7) / 8, B * ((Cout + 63) / 64));
    if (!split) { if (sizes) launch_conv(ra, s); else launch_conv(a, s); }     // (every layer of the stack has cout >= 64: the 64-channel tile)
    else if (taps == 9) {              // (every 3 x 3 layer of the stack has cin % 32 == 0 and cout % 64 == 0)
        if (sizes) hipLaunchKernelGGL(sp_conv3x3_split_kernel<RaggedConvArgs>, grid, dim3(256), 0, s, ra);
        else hipLaunchKernelGGL(sp_conv3x3_split_kernel<ConvArgs>, grid, dim3(256), 0, s, a);
    } else if (sizes) hipLaunchKernelGGL(sp_conv1x1_split_kernel<RaggedConvArgs>, grid, dim3(256), 0, s, ra);
    else hipLaunchKernelGGL(sp_conv1x1_split_kernel<ConvArgs>, grid, dim3(256), 0, s, a);
}

// params: packed weight / bias pointers in layer order conv1a, conv1b, conv2a, conv2b, conv3a, conv3b, conv4a, conv4b, convPa, convPb,
// convDa, convDb (24 device pointers).  ws: two ping-pong buffers of B*H*W*64 floats each.
// split != 0: every MFMA convolution on split-f16 operands (weights packed by launch_sp_pack_weight_split; conv1a — K = 9, VALU — stays fp32 with its fp32 packing)
// sizes: null, or the ragged batch's [B][2] (w, h) — H, W are then the canvas; level k of image b is its (h_b >> k) x (w_b >> k) corner of the level's canvas
static hipError_t launch_sp_encode(const float* image, int B, int H, int W, const int* sizes, const float* const* P, float* ws, float* scores, float* desc_map,
                                   int split_flag, hipStream_t s) {
    const bool split = split_flag != 0;
    const long long half = (long long)B * H * W * 64;
    float* A = ws; float* Bf = ws + half;
    const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8;
    const long long px = (long long)B * H * W * 16;
    if (sizes) hipLaunchKernelGGL(sp_conv1a_kernel<true>, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s, image, P[0], P[1], A, B, H, W, sizes);
    else hipLaunchKernelGGL(sp_conv1a_kernel<false>, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s, image, P[0], P[1], A, B, H, W, sizes);
    conv(split, A, Bf, P[2], P[3], B, H, W, 64, 64, 9, 1, 1, 0, sizes, 0, s);           // conv1b + pool  -> [H2][W2][64]
    conv(split, Bf, A, P[4], P[5], B, H2, W2, 64, 64, 9, 1, 0, 0, sizes, 1, s);         // conv2a
    conv(split, A, Bf, P[6], P[7], B, H2, W2, 64, 64, 9, 1, 1, 0, sizes, 1, s);         // conv2b + pool  -> [H4][W4][64]
    conv(split, Bf, A, P[8], P[9], B, H4, W4, 64, 128, 9, 1, 0, 0, sizes, 2, s);        // conv3a
    conv(split, A, Bf, P[10], P[11], B, H4, W4, 128, 128, 9, 1, 1, 0, sizes, 2, s);     // conv3b + pool  -> [H8][W8][128]
    conv(split, Bf, A, P[12], P[13], B, H8, W8, 128, 128, 9, 1, 0, 0, sizes, 3, s);     // conv4a
    conv(split, A, Bf, P[14], P[15], B, H8, W8, 128, 128, 9, 1, 0, 0, sizes, 3, s);     // conv4b         -> x in Bf
    float* x = Bf;
    float* t1 = A;                                                     // [H8][W8][256]
    float* t2 = A + (long long)B * H8 * W8 * 256;                      // [H8][W8][65]
    conv(split, x, t1, P[16], P[17], B, H8, W8, 128, 256, 9, 1, 0, 0, sizes, 3, s);     // convPa
    conv(split, t1, t2, P[18], P[19], B, H8, W8, 256, 65, 1, 0, 0, 0, sizes, 3, s);     // convPb (logits)
    const long long cells = (long long)B * H8 * W8;
    hipLaunchKernelGGL(sp_scores_kernel, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, s, t2, scores, B, H8, W8, sizes);
    conv(split, x, t1, P[20], P[21], B, H8, W8, 128, 256, 9, 1, 0, 0, sizes, 3, s);     // convDa
    conv(split, t1, desc_map, P[22], P[23], B, H8, W8, 256, 256, 1, 0, 0, 1, sizes, 3, s);   // convDb -> NCHW raw descriptor map
    return hipGetLastError();
}

}  // namespace lg

using namespace lg;

extern "C" {

int lg_sp_pack_conv_weight(const float* src, int32_t cout, int32_t cin, int32_t k, float* dst, void* hip_stream) {
    if (!src || !dst || cout < 1 || cin < 1 || (k != 1 && k != 3)) return set_error(LG_ERR_INVALID, "bad conv weight");
    HIPCHK(launch_sp_pack_weight(src, dst, cout, cin, k, static_cast<hipStream_t>(hip_stream)));
    return LG_OK;
}

int64_t lg_sp_encode_workspace_bytes(int32_t batch, int32_t h, int32_t w) {
    if (batch < 1 || h < 8 || w < 8) return 0;
    return (int64_t)2 * batch * h * w * 64 * 4;
}

int lg_sp_pack_conv_weight_split(const float* src, int32_t cout, int32_t cin, int32_t k, void* dst, void* hip_stream) {
    if (!src || !dst || cout < 1 || cin < 32 || cin % 32 || (k != 1 && k != 3) || (k == 3 && cout % 64)) return set_error(LG_ERR_INVALID, "bad conv weight (split form: cin a multiple of 32; 3 x 3 layers: cout a multiple of 64)");
    HIPCHK(launch_sp_pack_weight_split(src, dst, cout, cin, k, static_cast<hipStream_t>(hip_stream)));
    return LG_OK;
}

int lg_sp_encode(const lg_sp_encode_io* io, void* hip_stream) {
    if (int rc = check_extract_io(io, LG_EXTRACT_RAGGED | LG_EXTRACT_SPLIT, "lg_sp_encode")) return rc;
    const lg_sp_encode_io& a = *io;
    const bool split = a.flags & LG_EXTRACT_SPLIT;
    if (a.batch < 1 || a.h < 8 || a.w < 8) return set_error(LG_ERR_INVALID, "image (ragged batch: canvas) height / width must be at least 8");
    // sp_conv3x3_split_kernel addresses the pixels of ONE image with 32-bit element offsets (h w 64 channels at full resolution; a ragged image's strides are the canvas's)
    if (split && (int64_t)a.h * a.w * 64 >= (int64_t)1 << 31)
        return set_error(LG_ERR_INVALID, "split-f16 conv stack: h * w (ragged batch: of the canvas) must stay below 2^25 pixels (use conv_precision = fp32 for larger images)");
    if (!a.image || !a.params || !a.workspace || !a.scores || !a.desc_map) return set_error(LG_ERR_INVALID, "null pointer");
    if (a.workspace_bytes < lg_sp_encode_workspace_bytes(a.batch, a.h, a.w)) return set_error(LG_ERR_INVALID, "workspace too small (lg_sp_encode_workspace_bytes; ragged batch: of the canvas)");
    for (int i = 0; i < 24; ++i) if (!a.params[i]) return set_error(LG_ERR_INVALID, "null layer parameter");
    HIPCHK(launch_sp_encode(a.image, a.batch, a.h, a.w, extract_sizes(a), a.params, static_cast<float*>(a.workspace), a.scores, a.desc_map, split ? 1 : 0,
                            static_cast<hipStream_t>(hip_stream)));
    return LG_OK;
}

}  // extern "C"
