// lightglue_amd — attention input projections as one kernel per block:
//   SelfBlock  (ref lightglue.py:165-169): qkv = Wqkv x + b, split per head, rotary on q and k
//   CrossBlock (ref :204-209):             qk = to_qk x + b, v = to_v x + b   (same weights for both images)
// Output layouts feed lg_attention.hip directly: q, k [head][row][64], v TRANSPOSED [head][64][row].
//
// Same structure as the fused tail (lg_tail.hip): workgroup = 64 keypoint rows x ALL output columns, 8 waves
// split the columns; the 64 x 256 activation tile is read from HBM exactly once, converted to the operand
// precision and kept in LDS (64 KB as split f16); weight fragments come pre-packed in MFMA order straight
// from L2 (one coalesced 1 KB wave load each).  Wave w owns the n-tiles {w + 8j}: the columns are produced in
// two passes of NTP n-tiles per wave (keeps accumulators + weight ring under the register budget); the outputs
// leave straight from the accumulators (lg_proj_body.h: transposed MFMA form for q/k, plain form for v^T).
#include "lg_proj_body.h"
#include "lg_side.h"

namespace lg {

// the workgroup's tile; false when it has no live row (`len` = live rows of its segment) or its pair has stopped
__device__ __forceinline__ bool proj_tile(const RowSpace& rs, TileLoc& t, int& len) {
    t = locate_tile(rs, blockIdx.x, PBM);
    len = rs.len[t.seg];
    if (t.r0 >= len) return false;
    if (rs.active && !rs.active[t.pair]) return false;
    return true;
}
__device__ __forceinline__ bool proj_tile(const RowSpace& rs, TileLoc& t) { int len; return proj_tile(rs, t, len); }

// A thread's share of the 64 x 256 activation tile: 16-byte chunk slot tid & 7 of row tid >> 3 in every 128-byte stage row.
// load / load_f16: HBM -> registers (`src` = the row's first element of the slot; fp32 or binary16 rows).  store: registers -> operand precision -> LDS (once); copy_out: the fp32 values are
// first stored at xdst (the residual row of a keypoint that is new at this kernel).  No barrier (proj_compute / final_compute synchronise).
template <int PREC> struct TileRegs {
    static constexpr int NV = PJ<PREC>::Tag::EPC / 4, KE = PJL<PREC>::KE, STAGES = PJL<PREC>::STAGES;
    f32x4 v[STAGES][NV];
    __device__ __forceinline__ void load(const float* src) {
#pragma unroll
        for (int st = 0; st < STAGES; ++st)
#pragma unroll
            for (int j = 0; j < NV; ++j) v[st][j] = *reinterpret_cast<const f32x4*>(src + st * KE + 4 * j);
    }
    // the same elements of a row stored as binary16: one 16-byte load of 8 halves per stage (8 bytes of 4 with fp32 operands), widened exactly into the same registers
    __device__ __forceinline__ void load_f16(const f16_t* src) {
#pragma unroll
        for (int st = 0; st < STAGES; ++st) {
            if constexpr (NV == 2) {
                const f16x8 h = *reinterpret_cast<const f16x8*>(src + st * KE);
                v[st][0] = widen4_f16(h.lo); v[st][1] = widen4_f16(h.hi);
            } else {
                static_assert(NV == 1, "4 or 8 elements per chunk");
                v[st][0] = widen4_f16(*reinterpret_cast<const f16x4*>(src + st * KE));
            }
        }
    }
    __device__ __forceinline__ void store(char* smA, int srow, int sslot, bool copy_out, float* xdst) const {
        const int off = pj_tile_off(srow, sslot);
#pragma unroll
        for (int st = 0; st < STAGES; ++st) {
            if (copy_out) {
#pragma unroll
                for (int j = 0; j < NV; ++j) *reinterpret_cast<f32x4*>(xdst + st * KE + 4 * j) = v[st][j];
            }
            char* tile = smA + st * PJL<PREC>::TILE;
            if constexpr (PREC == PREC_F32) {
                *reinterpret_cast<f32x4*>(tile + off) = v[st][0];
            } else if constexpr (PJ<PREC>::APART == 2) {
                u32x4 hi, lo;
                split8<typename PJ<PREC>::Tag>(v[st][0], v[st][1], hi, lo);
                *reinterpret_cast<u32x4*>(tile + off) = hi;
                *reinterpret_cast<u32x4*>(tile + PJL<PREC>::A_PLANE + off) = lo;
            } else {   // single plane (PREC_QKV_F16W2: one f16 plane)
                *reinterpret_cast<u32x4*>(tile + off) = pack8<typename PJ<PREC>::Tag>(v[st][0], v[st][1]);
            }
        }
    }
};
// activation tile of rows that already lie in the residual stream X: HBM -> registers -> operand precision -> LDS
template <int PREC>
__device__ __forceinline__ void proj_load_tile(const float* X, const TileLoc& t, char* smA) {
    const int srow = threadIdx.x >> 3, sslot = threadIdx.x & 7;
    TileRegs<PREC> h;
    h.load(X + (long long)(t.grow0 + srow) * 256 + sslot * PJ<PREC>::Tag::EPC);
    h.store(smA, srow, sslot, false, nullptr);   // nothing to copy out: the rows are in X
}

template <int PREC, class TA, int NTP, int NPASS>
__global__ __launch_bounds__(PTHREADS) void proj_kernel(ProjArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* smA = smem;                                              // [NPART][STAGES][64][128 B]

    TileLoc t;
    if (!proj_tile(a.rs, t)) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (a.dbg && lane == 0) dbg_slot(a.dbg, w, 0) = clock64();   // profiling tap, slot 0
    RopeRows<4> rr;
    if constexpr (NTP == 3) proj_rope_load<4>(a, t, rr);   // before the x tile: both are cold, in flight together
    proj_load_tile<PREC>(a.X, t, smA);
    proj_compute<PREC, TA, NTP, NPASS>(a, t, smA, 0, NTP == 3 ? &rr : nullptr);
}

// ---- SelfBlock projections of keypoint rows that are NEW at this kernel: one kernel body (proj_rows_kernel) over two row sources.  A source says where
// thread (srow, sslot) of the tile finds local row rc — its residual row and its 4 rotary frequencies 4 sslot .. 4 sslot + 3 — and where the fp32 copies
// of both go; the kernel stages them, stores them and projects.
struct RowDest { float* X; float* cosb; float* sinb; };   // [R][256], [R][32], [R][32]

// The first SelfBlock projection with the per-keypoint preparation fused in (lg_kernels.h launch_proj_first): rows come from the forward's inputs, through
// the device functions prep_kernel calls (lg_side.h) and into proj_kernel's arithmetic, so the outputs are bit-identical to the two-launch form.
struct FirstRows {
    typedef PrepArgs Args;
    const PrepArgs& pa;
    const PrepSide& sd;                                     // the tile's side: uniform per workgroup
    int seg; long long simg, in_row;
    __device__ __forceinline__ FirstRows(const PrepArgs& pa_, const TileLoc& t, int rc) : pa(pa_), sd(pa_.side[t.seg & 1]), seg(t.seg) {
        simg = source_image(pa.px, t.pair, seg & 1);        // the image whose rows this tile reads: the pair itself unless the inputs are indexed
        in_row = simg * sd.n + rc;
    }
    // descriptor rows (the x tile), fp32 or binary16 (a SIFT store never comes here: ForwardPlan::fuse_prep)
    template <int PREC> __device__ __forceinline__ void load_x(TileRegs<PREC>& h, int col) const {
        if (sd.kind == DESC_F16) h.load_f16(static_cast<const f16_t*>(sd.desc) + in_row * 256 + col);
        else h.load(static_cast<const float*>(sd.desc) + in_row * 256 + col);
    }
    // rotary rows: thread -> keypoint srow, frequencies 4 sslot .. 4 sslot + 3
    __device__ __forceinline__ void rotary(int sslot, f32x4& c4, f32x4& s4) const {
        float kn[4];
        normalised_keypoint(pa, sd, seg, simg, in_row, kn);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const float p = fourier_phase(pa, kn, sslot * 4 + f);
            c4[f] = cosf(p); s4[f] = sinf(p);
        }
    }
    __device__ __forceinline__ RowDest dest() const { return {pa.X, pa.cosb, pa.sinb}; }
    __device__ __forceinline__ void row_stored(long long grow, int r, int sslot) const { if (sslot == 0) pa.ind[grow] = r; }   // the index set
};
// The SelfBlock projection behind a pruning step, with the compaction folded in (lg_kernels.h GatherArgs): the workgroup fetches the residual rows and the
// rotary rows of its 64 NEW keypoint rows from wherever they lived (src map), stores them at their new place in the other buffer set and projects them.
// The same fp32 values reach the same tile positions as after an in-place compaction, so q / k / v are bit-identical to that path.
struct GatherRows {
    typedef GatherArgs Args;
    const GatherArgs& ga;
    long long in_row;
    __device__ __forceinline__ GatherRows(const GatherArgs& ga_, const TileLoc& t, int rc) : ga(ga_) {
        const long long base = t.grow0 - t.r0;                             // first row of the segment
        const int sr = ga.len_old[t.seg] >= 0 ? ga.src[base + rc] : rc;
        in_row = base + sr;
    }
    template <int PREC> __device__ __forceinline__ void load_x(TileRegs<PREC>& h, int col) const { h.load(ga.Xold + in_row * 256 + col); }
    __device__ __forceinline__ void rotary(int sslot, f32x4& c4, f32x4& s4) const {
        c4 = *reinterpret_cast<const f32x4*>(ga.cos_old + in_row * 32 + sslot * 4);
        s4 = *reinterpret_cast<const f32x4*>(ga.sin_old + in_row * 32 + sslot * 4);
    }
    __device__ __forceinline__ RowDest dest() const { return {ga.Xnew, ga.cos_new, ga.sin_new}; }
    __device__ __forceinline__ void row_stored(long long, int, int) const {}
};

template <int PREC, class TA, class Rows>
__global__ __launch_bounds__(PTHREADS) void proj_rows_kernel(ProjArgs a, typename Rows::Args sa) {
    constexpr int EPC = PJ<PREC>::Tag::EPC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* smA = smem;
    float* ldsC = reinterpret_cast<float*>(smem + PJL<PREC>::A_BYTES);   // [64][32] cos, then [64][32] sin
    float* ldsS = ldsC + PBM * 32;

    TileLoc t;
    int len;
    if (!proj_tile(a.rs, t, len)) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, g = lane >> 4;
    const int srow = tid >> 3, sslot = tid & 7;
    const int r = t.r0 + srow, rc = r < len ? r : len - 1;             // rows past the segment's count: a finite copy of its last row (never stored)
    const Rows rows(sa, t, rc);
    const RowDest dst = rows.dest();
    // ---- the x tile requested first: cold, in flight under the rotary rows' arithmetic
    TileRegs<PREC> h;
    rows.load_x(h, sslot * EPC);
    {
        f32x4 c4, s4;
        rows.rotary(sslot, c4, s4);
        *reinterpret_cast<f32x4*>(ldsC + srow * 32 + sslot * 4) = c4;
        *reinterpret_cast<f32x4*>(ldsS + srow * 32 + sslot * 4) = s4;
        if (r < len) {
            const long long grow = t.grow0 + srow;
            *reinterpret_cast<f32x4*>(dst.cosb + grow * 32 + sslot * 4) = c4;
            *reinterpret_cast<f32x4*>(dst.sinb + grow * 32 + sslot * 4) = s4;
            rows.row_stored(grow, r, sslot);
        }
    }
    // ---- x tile -> fp32 residual stream + operand planes in LDS
    h.store(smA, srow, sslot, r < len, dst.X + (long long)(t.grow0 + srow) * 256 + sslot * EPC);
    __syncthreads();   // the tile's rotary rows are in LDS
    RopeRows<4> rr;
    {
        const int f0 = ((32 * w) & 63) / 2 + 4 * g;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int row = pj_row<4>(mt, lr);
            rr.c[mt] = *reinterpret_cast<const f32x4*>(ldsC + row * 32 + f0);
            rr.s[mt] = *reinterpret_cast<const f32x4*>(ldsS + row * 32 + f0);
        }
    }
    proj_compute<PREC, TA, 3, 2>(a, t, smA, 0, &rr);
}
template <class Rows> static hipError_t launch_proj_rows(int prec, int attn_prec, const ProjArgs& a, const typename Rows::Args& sa, hipStream_t s) {
    return dispatch_qkv_prec(prec, attn_prec, a.plane, [&](auto P, auto ta) {
        constexpr int PREC = decltype(P)::value;
        const int R = a.rs.B * (a.rs.cap0 + a.rs.cap1);
        return launch_with_lds(proj_rows_kernel<PREC, decltype(ta), Rows>, dim3(R / PBM), dim3(PTHREADS), PJL<PREC>::A_BYTES + 2 * PBM * 32 * 4, s, a, sa);
    });
}
hipError_t launch_proj_first(int prec, int attn_prec, const ProjArgs& a, const PrepArgs& pa, hipStream_t s) {
    if (!(a.Nout == 768 && a.n_qk_groups == 2 && a.cosb && a.sinb) || pa.input_dim != 256) return hipErrorInvalidValue;
    return launch_proj_rows<FirstRows>(prec, attn_prec, a, pa, s);
}
hipError_t launch_proj_gather(int prec, int attn_prec, const ProjArgs& a, const GatherArgs& g, hipStream_t s) {
    if (!(a.Nout == 768 && a.n_qk_groups == 2) || !g.Xold || !g.Xnew || !g.src || !g.len_old) return hipErrorInvalidValue;
    return launch_proj_rows<GatherRows>(prec, attn_prec, a, g, s);
}

// final projection of the log assignment as its own launch (adaptive depth: the weights of the layer each pair stopped at)
template <int PREC>
__global__ __launch_bounds__(PTHREADS) void final_proj_kernel(FinalArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    TileLoc t;
    if (!proj_tile(a.rs, t)) return;
    proj_load_tile<PREC>((a.xsel && a.xsel[t.pair]) ? a.X2 : a.X, t, smem);   // gather path: a pair's rows live in the buffer set they were in when it stopped
    final_compute<PREC>(a, t, smem);
}
template <int PREC> static hipError_t launch_final_t(const FinalArgs& a, hipStream_t s) {
    return launch_with_lds(final_proj_kernel<PREC>, dim3(a.R / PBM), dim3(PTHREADS), PJL<PREC>::A_BYTES, s, a);
}
hipError_t launch_final_proj(int prec, const FinalArgs& a, hipStream_t s) {
    switch (prec) {
        case PREC_F32: return launch_final_t<PREC_F32>(a, s);
        case PREC_BF16: return launch_final_t<PREC_BF16>(a, s);
        case PREC_F16: return launch_final_t<PREC_F16>(a, s);
        case PREC_F16X3: return launch_final_t<PREC_F16X3>(a, s);
    }
    return hipErrorInvalidValue;
}

template <int PREC, class TA, int NTP, int NPASS> static hipError_t launch_proj_t(const ProjArgs& a, hipStream_t s) {
    const int R = a.rs.B * (a.rs.cap0 + a.rs.cap1);
    return launch_with_lds(proj_kernel<PREC, TA, NTP, NPASS>, dim3(R / PBM), dim3(PTHREADS), PJL<PREC>::A_BYTES, s, a);
}
hipError_t launch_proj(int prec, int attn_prec, const ProjArgs& a, hipStream_t s) {
    return dispatch_qkv_prec(prec, attn_prec, a.plane, [&](auto P, auto ta) {
        constexpr int PREC = decltype(P)::value;
        typedef decltype(ta) TA;
        if (a.Nout == 768 && a.n_qk_groups == 2 && a.cosb && a.sinb) return launch_proj_t<PREC, TA, 3, 2>(a, s);
        if (a.Nout == 512 && a.n_qk_groups == 1) return launch_proj_t<PREC, TA, 2, 2>(a, s);
        return hipErrorInvalidValue;
    });
}

}  // namespace lg
