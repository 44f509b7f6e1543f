// lightglue_amd — the kernels SuperPoint and ALIKED share (see lg_extract.h): the exact-fp32 convolution, the weight repack, simple_nms,
// threshold + compaction and the top-K selection.
#include "lg_extract.h"

namespace lg {

// ==================================================================================================== convolution
// acc[mt][nt] += the wave's 2 rows x 32 pixels x 16 NT channels of one operand pair (in [pixel][Cin] of one image, w [taps][Cout][Cin]).
// H, W and Cout are read from `a` where they are used (kernel arguments): passed as values, the NT = 4 instance needs 141 VGPRs instead of 126.
// Addresses and strides: a.H / a.W (the canvas); the padding select and the address clamp: the image extent `e` when RAGGED (conv_extent), so nothing outside an image is read.
template <int NT, bool RAGGED>
__device__ __forceinline__ void conv_accum(f32x4 (&acc)[4][NT], const ConvArgs& a, const float* inb, const float* wf, int Cin, int taps, int n0, int x0,
                                           int y0, int lr, int g, const ConvExtent& e) {
    const int nchunk = Cin >> 4;
    const int ntl = min(NT, (a.Cout - n0 + 15) >> 4);        // live n-tiles of this channel group (wave-uniform)
    for (int tap = 0; tap < taps; ++tap) {
        const int dy = taps == 9 ? tap / 3 - 1 : 0, dx = taps == 9 ? tap % 3 - 1 : 0;
        // source pixel of every m-tile for this tap (clamped; `ok` = inside the image)
        long long poff[4]; bool ok[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int yy = y0 + (mt >> 1) + dy, xx = x0 + (mt & 1) * 16 + lr + dx;
            ok[mt] = yy >= 0 && yy < ext_h<RAGGED>(a, e) && xx >= 0 && xx < ext_w<RAGGED>(a, e);
            const int yc = min(max(yy, 0), ext_h<RAGGED>(a, e) - 1), xc = min(max(xx, 0), ext_w<RAGGED>(a, e) - 1);
            poff[mt] = ((long long)yc * a.W + xc) * Cin + 4 * g;
        }
        long long wrow[NT];   // weight row of every n-tile, in elements (clamped into the matrix; dead lanes are zeroed after the load)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wrow[nt] = ((long long)tap * a.Cout + min(n0 + nt * 16 + lr, a.Cout - 1)) * Cin + 4 * g;
        for (int c = 0; c < nchunk; ++c) {
            u32x4 af[4], bf[NT];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(inb + poff[mt] + c * 16);
                af[mt] = ok[mt] ? v : u32x4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const bool live = nt < ntl && n0 + nt * 16 + lr < a.Cout;
                const u32x4 v = *reinterpret_cast<const u32x4*>(wf + wrow[nt] + c * 16);
                bf[nt] = live ? v : u32x4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) mma_chunk<TagF32>(acc[mt][nt], af[mt], bf[nt]);
        }
    }
}

// grid (W / 32, H / 8, B * cout groups of 16 NT).  RAGGED: a tile whose origin lies outside its image has nothing to do
template <int NT, bool EXTRA, class A>
__global__ __launch_bounds__(256) void conv_kernel(A a) {
    constexpr bool RAGGED = is_ragged<A>;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, g = lane >> 4;
    const int ngroups = (a.Cout + 16 * NT - 1) / (16 * NT);
    const int b = blockIdx.z / ngroups, n0 = (blockIdx.z - b * ngroups) * 16 * NT;
    const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 8 + wv * 2;
    const ConvExtent e = conv_extent(a, b);
    if (y0 >= ext_h<RAGGED>(a, e)) return;
    if constexpr (RAGGED) { if (x0 >= e.w) return; }
    f32x4 acc[4][NT];   // [mt = ry * 2 + xt][nt]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const long long img = (long long)b * a.H * a.W;
    conv_accum<NT, RAGGED>(acc, a, a.in + img * a.Cin, static_cast<const float*>(a.w), a.Cin, a.taps, n0, x0, y0, lr, g, e);
    if constexpr (EXTRA) conv_accum<NT, RAGGED>(acc, a, a.in2 + img * a.Cin2, a.w2, a.Cin2, 1, n0, x0, y0, lr, g, e);
    conv_epilogue<NT, RAGGED>(a, acc, b, n0, x0, y0, lr, g, e);
}

template <int NT, class A> static void conv_nt(const A& a, hipStream_t s) {
    const dim3 grid((a.W + 31) / 32, (a.H + 7) / 8, a.B * ((a.Cout + 16 * NT - 1) / (16 * NT)));
    if (a.in2) hipLaunchKernelGGL((conv_kernel<NT, true, A>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((conv_kernel<NT, false, A>), grid, dim3(256), 0, s, a);
}

template <class A> static void conv_any(const A& a, hipStream_t s) {
    if (a.Cout <= 16) conv_nt<1>(a, s);
    else if (a.Cout <= 32) conv_nt<2>(a, s);
    else conv_nt<4>(a, s);
}
void launch_conv(const ConvArgs& a, hipStream_t s) { conv_any(a, s); }
void launch_conv(const RaggedConvArgs& a, hipStream_t s) { conv_any(a, s); }

// ==================================================================================================== weight repack
__global__ __launch_bounds__(256) void fold_kernel(const float* src, float* dst, float* bias_dst, int Cout, int Cin, int kk, int mode, const float* gamma,
                                                   const float* beta, const float* mean, const float* var, const float* cbias, const float* extra) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, total = (long long)Cout * Cin * kk;
    if (i >= total) return;
    int co, ci, t;
    if (mode == PK_AGG) {    // src [n_pos][128][128] = (p, c, d) -> dst [d][p * 128 + c]; Cin = n_pos * 128
        co = (int)(i % Cout); ci = (int)(i / Cout); t = 0;
    } else {
        t = (int)(i % kk); ci = (int)((i / kk) % Cin); co = (int)(i / ((long long)kk * Cin));
    }
    const float s = gamma ? gamma[co] / sqrtf(var[co] + 1e-5f) : 1.f;
    const float v = s * src[i];
    long long o;
    switch (mode) {
        case PK_TAP_CO_CI: o = ((long long)t * Cout + co) * Cin + ci; break;
        case PK_CO_TAP_CI: o = ((long long)co * kk + t) * Cin + ci; break;
        case PK_TAP_CI_CO: o = ((long long)t * Cin + ci) * Cout + co; break;
        case PK_AGG: o = (long long)co * Cin + ci; break;
        default: o = i;
    }
    dst[o] = v;
    if (bias_dst && ci == 0 && t == 0) {
        float bv = cbias ? cbias[co] : 0.f;
        if (gamma) bv = s * (bv - mean[co]) + beta[co];
        if (extra) bv += extra[co];
        bias_dst[co] = bv;
    }
}

hipError_t launch_fold(const float* src, float* dst, float* bias_dst, int Cout, int Cin, int kk, int mode, const float* const* bn, const float* cbias,
                       const float* extra, hipStream_t s) {
    const long long total = (long long)Cout * Cin * kk;
    hipLaunchKernelGGL(fold_kernel, dim3(blocks(total)), dim3(256), 0, s, src, dst, bias_dst, Cout, Cin, kk, mode, bn ? bn[0] : nullptr,
                       bn ? bn[1] : nullptr, bn ? bn[2] : nullptr, bn ? bn[3] : nullptr, cbias, extra);
    return hipGetLastError();
}

// ==================================================================================================== simple_nms
// HBM-trivial work (a 1024 x 768 map is 3 MB): one 64 x 16 pixel tile per workgroup with a halo of 2 NR in LDS, separable max / or passes.
// NR = 4: 38 400 bytes of LDS; NR = 8: 69 120.
constexpr int NTX = 64, NTY = 16;

// for every (ly, lx) of the local region [y0, y1) x [x0, x1): body(ly, lx); threads stride over the region
template <class F> __device__ __forceinline__ void for_region(int y0, int y1, int x0, int x1, F body) {
    const int w = x1 - x0, n = (y1 - y0) * w;
    for (int i = threadIdx.x; i < n; i += blockDim.x) body(y0 + i / w, x0 + i % w);
}

// mode 0: mask_out = (S == maxpool(S))
// mode 1: one suppression round mask_in -> mask_out
// mode 2: the same round, but writes nms = mask ? S : 0 instead of the mask
template <int NR>
__global__ __launch_bounds__(256) void nms_kernel(DetectArgs a, int mode, const unsigned char* mask_in, unsigned char* mask_out) {
    constexpr int NLW = NTX + 4 * NR, NLH = NTY + 4 * NR;   // tile + halo of 2r on every side
    __shared__ float sS[NLH][NLW], sSS[NLH][NLW], sH[NLH][NLW];
    __shared__ unsigned char sM[NLH][NLW], sHM[NLH][NLW], sSupp[NLH][NLW];
    const int b = blockIdx.z, ty0 = blockIdx.y * NTY, tx0 = blockIdx.x * NTX, r = a.radius, O = 2 * NR;   // O: local origin offset
    const long long img = (long long)b * a.H * a.W;
    // the bound is image b's score extent, the strides are the canvas's.  A pixel outside the extent is padding (-inf, mask 0), NOT a zero score: 0 == maxpool(0) would make it
    // a maximum, and the first suppression round would then remove real maxima within r of the far border
    const DetectExtent e = detect_extent(a, b);
    if (ty0 >= e.h || tx0 >= e.w) return;       // tile outside the image (workgroup-uniform, before the first barrier): nothing to write, and nobody reads there
    auto inside = [&](int ly, int lx) { const int y = ty0 + ly - O, x = tx0 + lx - O; return y >= 0 && y < e.h && x >= 0 && x < e.w; };
    // ---- load S (and the mask) for tile +- 2r; outside the image: -inf / 0 (max_pool2d pads with -inf)
    for_region(O - 2 * r, O + NTY + 2 * r, O - 2 * r, O + NTX + 2 * r, [&](int ly, int lx) {
        const bool in = inside(ly, lx);
        const long long idx = img + (long long)(ty0 + ly - O) * a.W + (tx0 + lx - O);
        sS[ly][lx] = in ? a.S[idx] : -INFINITY;
        sM[ly][lx] = (mode != 0 && in) ? mask_in[idx] : 0;
    });
    __syncthreads();
    if (mode == 0) {
        for_region(O - r, O + NTY + r, O, O + NTX, [&](int ly, int lx) {
            float m = -INFINITY;
            for (int d = -r; d <= r; ++d) m = fmaxf(m, sS[ly][lx + d]);
            sH[ly][lx] = m;
        });
        __syncthreads();
        for_region(O, O + NTY, O, O + NTX, [&](int ly, int lx) {
            if (!inside(ly, lx)) return;
            float m = -INFINITY;
            for (int d = -r; d <= r; ++d) m = fmaxf(m, sH[ly + d][lx]);
            mask_out[img + (long long)(ty0 + ly - O) * a.W + (tx0 + lx - O)] = sS[ly][lx] == m;
        });
        return;
    }
    // ---- supp = maxpool(mask) > 0 on tile +- r (separable or)
    for_region(O - 2 * r, O + NTY + 2 * r, O - r, O + NTX + r, [&](int ly, int lx) {
        unsigned char v = 0;
        for (int d = -r; d <= r; ++d) v |= sM[ly][lx + d];
        sHM[ly][lx] = v;
    });
    __syncthreads();
    for_region(O - r, O + NTY + r, O - r, O + NTX + r, [&](int ly, int lx) {
        unsigned char v = 0;
        for (int d = -r; d <= r; ++d) v |= sHM[ly + d][lx];
        sSupp[ly][lx] = v;
        sSS[ly][lx] = !inside(ly, lx) ? -INFINITY : (v ? 0.f : sS[ly][lx]);   // supp_scores
    });
    __syncthreads();
    // ---- new_max_mask = supp_scores == maxpool(supp_scores) on the tile
    for_region(O - r, O + NTY + r, O, O + NTX, [&](int ly, int lx) {
        float m = -INFINITY;
        for (int d = -r; d <= r; ++d) m = fmaxf(m, sSS[ly][lx + d]);
        sH[ly][lx] = m;
    });
    __syncthreads();
    for_region(O, O + NTY, O, O + NTX, [&](int ly, int lx) {
        if (!inside(ly, lx)) return;
        float m = -INFINITY;
        for (int d = -r; d <= r; ++d) m = fmaxf(m, sH[ly + d][lx]);
        const bool keep = sM[ly][lx] || ((sSS[ly][lx] == m) && !sSupp[ly][lx]);
        const long long idx = img + (long long)(ty0 + ly - O) * a.W + (tx0 + lx - O);
        if (mode == 1) mask_out[idx] = keep;
        else a.nms[idx] = keep ? sS[ly][lx] : 0.f;
    });
}

template <int NR> static void nms_nr(const DetectArgs& a, hipStream_t s) {
    const dim3 grid((a.W + NTX - 1) / NTX, (a.H + NTY - 1) / NTY, a.B);
    hipLaunchKernelGGL(nms_kernel<NR>, grid, dim3(256), 0, s, a, 0, (const unsigned char*)nullptr, a.mask_a);
    hipLaunchKernelGGL(nms_kernel<NR>, grid, dim3(256), 0, s, a, 1, (const unsigned char*)a.mask_a, a.mask_b);   // first suppression round
    hipLaunchKernelGGL(nms_kernel<NR>, grid, dim3(256), 0, s, a, 2, (const unsigned char*)a.mask_b, (unsigned char*)nullptr);   // second + nms
}

void launch_nms(const DetectArgs& a, hipStream_t s) {
    if (a.radius <= 4) nms_nr<4>(a, s);
    else nms_nr<8>(a, s);
}

// ==================================================================================================== threshold + compaction
// far edges: image_size (truncated like .long()) where given, else the image's score extent; outside that extent: -inf, which no threshold lets pass (also with border == 0)
__device__ __forceinline__ float detect_value(const DetectArgs& a, const DetectExtent& e, int b, int y, int x) {
    int hl = e.h, wl = e.w;
    if (a.image_size) { wl = (int)a.image_size[2 * b]; hl = (int)a.image_size[2 * b + 1]; }   // .long(): truncation
    if (y >= e.h || x >= e.w) return -INFINITY;
    const bool border = a.border > 0 && (y < a.border || x < a.border || y >= hl - a.border || x >= wl - a.border);
    return border ? a.border_value : a.nms[((long long)b * a.H + y) * a.W + x];
}

// per image row: the pixels above the threshold (th[b] when th is set, else a.threshold) and, when rowsum is set, the row sum of S.  grid (H, B)
// The sum is over the image's own columns and rows: a pixel outside its extent adds an exact 0 at the thread and tree position it has, so the float64
// sum of a ragged row is bit for bit the one of the crop (a shorter strided loop and the same tree), and a row below the image sums to 0.
__global__ __launch_bounds__(256) void row_count_kernel(DetectArgs a, const float* th, double* rowsum) {
    const int y = blockIdx.x, b = blockIdx.y;
    const long long row = ((long long)b * a.H + y) * a.W;
    const float t = th ? th[b] : a.threshold;
    const DetectExtent e = detect_extent(a, b);
    const int wsum = y < e.h ? e.w : 0;
    int cnt = 0; double sum = 0.0;
    for (int x = threadIdx.x; x < a.W; x += 256) {
        cnt += detect_value(a, e, b, y, x) > t;
        if (rowsum && x < wsum) sum += (double)a.S[row + x];
    }
    __shared__ int sh[4];
    cnt = block_sum(cnt, sh);
    if (threadIdx.x == 0) a.row_counts[b * a.H + y] = cnt;
    if (rowsum) {
        __shared__ double shd[256];
        shd[threadIdx.x] = sum;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) shd[threadIdx.x] += shd[threadIdx.x + o]; __syncthreads(); }
        if (threadIdx.x == 0) rowsum[b * a.H + y] = shd[0];
    }
}

// raster-order compaction (the order of torch.where / nonzero): grid (H, B)
__global__ __launch_bounds__(256) void compact_kernel(DetectArgs a, const float* th) {
    const int y = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float t = th ? th[b] : a.threshold;
    const DetectExtent e = detect_extent(a, b);
    __shared__ int sh[4];
    int pre = 0;
    for (int yy = tid; yy < y; yy += 256) pre += a.row_counts[b * a.H + yy];
    int running = block_sum(pre, sh);
    const long long cb = (long long)b * a.max_candidates;
    for (int x0 = 0; x0 < a.W; x0 += 256) {
        const int x = x0 + tid;
        const float v = x < a.W ? detect_value(a, e, b, y, x) : 0.f;
        const bool hit = x < a.W && v > t;
        const unsigned long long bal = __ballot(hit);
        __syncthreads();
        if (lane == 0) sh[wave] = __popcll(bal);
        __syncthreads();
        int off = running;
        for (int w = 0; w < wave; ++w) off += sh[w];
        off += __popcll(bal & ((1ull << lane) - 1ull));
        if (hit && off < a.max_candidates) { a.cand_idx[cb + off] = y * a.W + x; a.cand_score[cb + off] = v; }
        running += sh[0] + sh[1] + sh[2] + sh[3];
    }
    if (y == a.H - 1 && tid == 0) a.cand_total[b] = running;
}

void launch_row_count(const DetectArgs& a, const float* th, double* rowsum, hipStream_t s) {
    hipLaunchKernelGGL(row_count_kernel, dim3(a.H, a.B), dim3(256), 0, s, a, th, rowsum);
}
void launch_compact(const DetectArgs& a, const float* th, hipStream_t s) { hipLaunchKernelGGL(compact_kernel, dim3(a.H, a.B), dim3(256), 0, s, a, th); }

// ==================================================================================================== selection
// order-preserving key of a float: larger float <-> larger unsigned
__device__ __forceinline__ unsigned score_key(float v) { const unsigned u = __float_as_uint(v); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

// radix select, 8 bits per pass from the top: `prefix` = key of the K-th largest of the n scores, `need` = how many keys equal to it are
// among the K largest.  1024 threads
__device__ __forceinline__ void radix_select(const float* score, int n, unsigned K, unsigned& prefix, unsigned& need) {
    __shared__ unsigned hist[256];
    __shared__ unsigned prefix_sh, need_sh;
    const int tid = threadIdx.x;
    prefix = 0; need = K;    // among keys matching `prefix` on the bits fixed so far, we still need `need`
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const unsigned fixed_mask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int i = tid; i < n; i += 1024) {
            const unsigned k = score_key(score[i]);
            if ((k & fixed_mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned acc = 0; int d = 255;
            for (; d > 0; --d) { if (acc + hist[d] >= need) break; acc += hist[d]; }
            prefix_sh = prefix | ((unsigned)d << shift); need_sh = need - acc;
        }
        __syncthreads();
        prefix = prefix_sh; need = need_sh;
        __syncthreads();
    }
}

// per image: the candidates that survive the limit, in raster order (sel), with their keys.  grid (B), 1024 threads
__global__ __launch_bounds__(1024) void select_kernel(DetectArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int total = min(a.cand_total[b], a.max_candidates);
    const float* csc = a.cand_score + (long long)b * a.max_candidates;
    int* sel = a.sel + (long long)b * a.sel_cap;
    unsigned* skey = a.sel_key + (long long)b * a.sel_cap;
    const bool limit = a.K > 0 && total > a.K;
    __shared__ int wsum[16];
    unsigned prefix = 0, need = 0xFFFFFFFFu;
    if (limit) radix_select(csc, total, (unsigned)a.K, prefix, need);
    // keep key > prefix, and the first `need` keys == prefix in raster order (everything when not limited)
    int taken = 0, eq_taken = 0;
    for (int i0 = 0; i0 < total; i0 += 1024) {
        const int i = i0 + tid;
        const unsigned k = i < total ? score_key(csc[i]) : 0u;
        const bool eq = limit && i < total && k == prefix;
        const unsigned long long beq = __ballot(eq);
        __syncthreads();
        if (lane == 0) wsum[wave] = __popcll(beq);
        __syncthreads();
        int eoff = eq_taken;
        for (int w = 0; w < wave; ++w) eoff += wsum[w];
        eoff += __popcll(beq & ((1ull << lane) - 1ull));
        int eall = 0;
        for (int w = 0; w < 16; ++w) eall += wsum[w];
        const bool keep = i < total && (!limit || k > prefix || (eq && eoff < (int)need));
        const unsigned long long bk = __ballot(keep);
        __syncthreads();
        if (lane == 0) wsum[wave] = __popcll(bk);
        __syncthreads();
        int off = taken;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        off += __popcll(bk & ((1ull << lane) - 1ull));
        if (keep && off < a.sel_cap) { sel[off] = i; skey[off] = k; }
        int all = 0;
        for (int w = 0; w < 16; ++w) all += wsum[w];
        taken += all; eq_taken += eall;
    }
}

void launch_select(const DetectArgs& a, hipStream_t s) { hipLaunchKernelGGL(select_kernel, dim3(a.B), dim3(1024), 0, s, a); }

// ==================================================================================================== workspace
DetectLayout detect_layout(int B, int H, int W, int max_candidates, int sel_cap, bool stats) {
    const long long px = (long long)B * H * W;
    Bump bp; DetectLayout L{};
    L.mask_a = bp.take(px); L.mask_b = bp.take(px); L.nms = bp.take(px * 4); L.rows = bp.take((long long)B * H * 4);
    L.rowsum = stats ? bp.take((long long)B * H * 8) : -1; L.th = stats ? bp.take(B * 4) : -1;
    L.cidx = bp.take((long long)B * max_candidates * 4); L.cscore = bp.take((long long)B * max_candidates * 4); L.ctotal = bp.take(B * 4);
    L.sel = bp.take((long long)B * sel_cap * 4); L.selkey = bp.take((long long)B * sel_cap * 4);
    L.total = bp.used;
    return L;
}

void detect_bind(DetectArgs& a, const DetectLayout& L, void* ws) {
    char* w = static_cast<char*>(ws);
    a.mask_a = reinterpret_cast<unsigned char*>(w + L.mask_a); a.mask_b = reinterpret_cast<unsigned char*>(w + L.mask_b);
    a.nms = reinterpret_cast<float*>(w + L.nms); a.row_counts = reinterpret_cast<int*>(w + L.rows);
    a.cand_idx = reinterpret_cast<int*>(w + L.cidx); a.cand_score = reinterpret_cast<float*>(w + L.cscore); a.cand_total = reinterpret_cast<int*>(w + L.ctotal);
    a.sel = reinterpret_cast<int*>(w + L.sel); a.sel_key = reinterpret_cast<unsigned*>(w + L.selkey);
}

}  // namespace lg
