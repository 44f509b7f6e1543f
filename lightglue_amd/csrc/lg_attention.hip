// lightglue_amd — flash-style attention for the matcher (ref lightglue.py:113-137 Attention,
// used by SelfBlock :170 and both directions of CrossBlock :211-214 / :216-223).
//   head_dim 64, 4 heads, non-causal, q_len != kv_len (cross), ragged per-segment lengths.
//
// Workgroup = 4 waves = 128 query rows of one (segment, head); K and V^T tiles of 64 keys are
// staged through LDS (register hop, next tile's loads in flight during the MFMAs) and shared by
// the 4 waves.  Each wave owns 32 query rows (two 16-row MFMA tiles).
//
// "Swapped" formulation (guide T12 idea, 16x16 tiles): S^T = K Q^T and O^T = V^T P^T, so that a
// query row lives in ONE lane column (lane & 15): the online-softmax max/sum run over a lane's own
// registers plus two cross-lane steps (lane groups g = 0..3), the rescale factor is a per-lane
// scalar, and P^T leaves the S^T accumulators already in B-operand order for the PV MFMA:
//   f32:    S^T acc[kt][qt][r] <-> key key_of<4>(kt, g, r) (natural order);  PV chunk kt: B element i <-> key 16*kt + 4*g + i
//   16-bit: the K rows feeding S^T tile kt are PERMUTED (a free choice: which K row a lane reads) so that the 8
//           probabilities a lane group packs for PV chunk tp are 8 CONSECUTIVE keys:
//           S^T acc[kt][qt][r] <-> key key_of<8>(kt, g, r),   PV chunk tp: B element j <-> key 32*tp + 8*g + j
// V is produced TRANSPOSED by the projection ([head][d][row]) so the matching A operand is ONE contiguous 16-byte
// LDS read per fragment in both cases (the natural order needed two 8-byte reads + register shuffles).
// The S matrix never touches HBM.  q and k arrive pre-multiplied by sqrt(log2(e) / sqrt(64)) (lg_proj_body.h QK_PRESCALE, the
// reference's CPU path splits its scale the same way, lightglue.py:215), so S is already the base-2 logit: softmax runs in fp32
// with bare exp2, and in the LDS-DMA kernels the score accumulators START at -m_run so that exp2 applies to the MFMA result.
// Three kernels over one set of steps: attn_kernel stages its tiles through registers (every precision), attn_dma_kernel and attn_split_kernel move them by LDS-DMA and
// keep the scores re-based on the running maximum.  The shared steps are written and explained once, ahead of the kernels; a kernel's comment says what is specific to it.
#include "lg_kernels.h"

namespace lg {

constexpr int ABK = 64, ATHREADS = 256;   // query rows per workgroup = 64 * QT (QT 16-row query tiles per wave, 4 waves)

// ---- profiling taps.  -DLG_ATTN_TIMING (tools/attn_timing.py): per-phase s_memtime sums, wave-uniform, stamped by ATT_TICK(pc, slot) on the kernel's PhaseClock.  -DLG_ATTN_WALL
// (tools/attn_wall.py): workgroup life span on the 100 MHz wall clock + shader cycles + where it ran.  Both write AttnArgs::dbg[blocks][NW waves][8]; a production build has none of it.
#ifdef LG_ATTN_TIMING
struct PhaseClock { long long tacc[7] = {0, 0, 0, 0, 0, 0, 0}, tprev = clock64(); };
#define ATT_TICK(pc, slot) do { const long long _n = clock64(); (pc).tacc[slot] += _n - (pc).tprev; (pc).tprev = _n; } while (0)
#else
struct PhaseClock {};
#define ATT_TICK(pc, slot) do { } while (0)
#endif
#ifdef LG_ATTN_WALL
struct WallClock { long long wall0 = wall_clock64(), cyc0 = clock64(); };
#else
struct WallClock {};
#endif
template <int NW> __device__ __forceinline__ long long* dbg_words(const AttnArgs& a) {   // lane 0 of a wave: the wave's 8 words; else nullptr
    return a.dbg && (threadIdx.x & 63) == 0 ? a.dbg + ((long long)blockIdx.x * NW + (threadIdx.x >> 6)) * 8 : nullptr;
}
template <int NW> __device__ __forceinline__ void dump_timing(const AttnArgs& a, const PhaseClock& pc, int ntiles) {
#ifdef LG_ATTN_TIMING
    if (long long* d = dbg_words<NW>(a)) {
        for (int i = 0; i < 6; ++i) d[i] = pc.tacc[i];
        d[6] = ntiles; d[7] = 1;
    }
#endif
}
template <int NW> __device__ __forceinline__ void dump_wall(const AttnArgs& a, const WallClock& wc, int ntiles) {
#ifdef LG_ATTN_WALL
    if (long long* d = dbg_words<NW>(a)) {
        d[0] = wc.wall0; d[1] = wall_clock64(); d[2] = clock64() - wc.cyc0; d[3] = __builtin_amdgcn_s_getreg((31 << 11) | 4); d[4] = __builtin_amdgcn_s_getreg((31 << 11) | 20); d[6] = ntiles; d[7] = 1;
    }
#endif
}

// ---- workgroup set-up: which (head, query tile of ABM rows) a workgroup owns and which keys it attends to.  XCD-aware order: the query tiles of one (segment, head)
// share its K/V (<= 1 MB at n = 4096), so keep them consecutive on one XCD's L2; v = (row tile, head) with head fastest-but-one.  Tiles of up to 128 rows tile the row space;
// 256-row tiles are laid out per segment (capacities are multiples of 128, not of 256).  attention_tiles is the host's side: a launch has 4 heads x attention_tiles workgroups.
static int attention_tiles(const RowSpace& rs, int rows) {
    return rows <= 128 ? rs.B * (rs.cap0 + rs.cap1) / rows : rs.B * ((rs.cap0 + rows - 1) / rows + (rs.cap1 + rows - 1) / rows);
}
struct AttnWg { int head; TileLoc t; int qlen, kvseg, kvlen; long long kvbase; };
// false: nothing to do (no live query row in the tile, or the pair has stopped) — the kernel returns at once, w is not filled in past qlen
template <int ABM> __device__ __forceinline__ bool attn_workgroup(const AttnArgs& a, AttnWg& w) {
    const int ntile = gridDim.x >> 2;
    const int v = xcd_remap(blockIdx.x, gridDim.x);
    w.head = v / ntile;
    TileLoc& t = w.t;
    if constexpr (ABM <= 128) {
        t = locate_tile(a.rs, v - w.head * ntile, ABM);
    } else {
        const int t0 = (a.rs.cap0 + ABM - 1) / ABM, t1 = (a.rs.cap1 + ABM - 1) / ABM, idx = v - w.head * ntile;
        t.pair = idx / (t0 + t1);
        const int rem = idx - t.pair * (t0 + t1);
        t.image = rem >= t0 ? 1 : 0;
        t.r0 = (rem - t.image * t0) * ABM;
        t.seg = 2 * t.pair + t.image;
        t.grow0 = seg_row_base(a.rs, t.seg) + t.r0;
    }
    w.qlen = a.rs.len[t.seg];
    if (t.r0 >= w.qlen) return false;
    if (a.rs.active && !a.rs.active[t.pair]) return false;
    w.kvseg = a.cross ? (t.seg ^ 1) : t.seg;
    w.kvlen = a.rs.len[w.kvseg];
    w.kvbase = seg_row_base(a.rs, w.kvseg);
    return true;
}
// ref :114-115: empty key set -> zeros
template <int ABM, int NT> __device__ __forceinline__ void zero_ctx_tile(float* ctx, const AttnWg& w, int tid) {
    for (int i = tid; i < ABM * 16; i += NT) {
        const int row = i >> 4, c4 = i & 15;
        if (w.t.r0 + row < w.qlen) *reinterpret_cast<f32x4*>(ctx + (w.t.grow0 + row) * 256LL + w.head * 64 + c4 * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
// ---- key (row of the 64-key tile) behind element r of S^T accumulator kt in lane group g: THE definition of the key order (file header).
// Lane form: the K row that lane lr reads for S^T tile kt is key_of(kt, lr >> 2, lr & 3).
template <int EPC> __device__ __forceinline__ constexpr int key_of(int kt, int g, int r) {
    return EPC == 8 ? 32 * (kt >> 1) + 8 * g + 4 * (kt & 1) + r : 16 * kt + 4 * g + r;
}
// scores of keys past the live length -> -inf (wave-uniform test: only the last tile can hold dead keys).  The ints travel by reference on purpose:
// by value hipcc if-converts the 16 tests differently and attn_kernel<., 4> comes out 3 VGPRs up.
template <int EPC, int QT> __device__ __forceinline__ void mask_dead_keys(f32x4 (&s)[4][QT], const int& g, const int& kv0, const int& kvlen) {
    if (kv0 + ABK > kvlen) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kv0 + key_of<EPC>(kt, g, 0) + r >= kvlen) s[kt][qt][r] = -INFINITY;
    }
}
// maximum over the 64 keys of query column (qt, lane & 15): 16 scores per lane as a depth-3 tree of v_max3, then the 4 lane groups of the column
// (no LDS round trip).  Finite: every tile holds >= 1 live key (q, k carry the score scale).
template <int QT> __device__ __forceinline__ float row_max16(const f32x4 (&s)[4][QT], int qt) {
    const float t0 = vmax3(s[0][qt][0], s[0][qt][1], s[0][qt][2]), t1 = vmax3(s[0][qt][3], s[1][qt][0], s[1][qt][1]);
    const float t2 = vmax3(s[1][qt][2], s[1][qt][3], s[2][qt][0]), t3 = vmax3(s[2][qt][1], s[2][qt][2], s[2][qt][3]);
    const float t4 = vmax3(s[3][qt][0], s[3][qt][1], s[3][qt][2]);
    const float mx = vmax2(vmax3(t0, t1, t2), vmax3(t3, t4, s[3][qt][3]));
    return xor32_max(xor16_max(mx));
}
// s -> exp2(s - m_run) (SUB_M) or exp2(s) (scores that arrive re-based); l_run += their sum.  SCALAR v_sub_f32 / v_add_f32 and the bare v_exp_f32 (arguments <= 8, flush-to-zero
// tail is fine).  Packed f32 ops (v_pk_add_f32) are cheaper on their own but barely co-issue with another wave's MFMAs on the SIMD (tools/ubench/mfma_valu_overlap.hip: 24 %
// overlap vs 79 % for scalar ops), and these kernels live on that overlap.  Two partial sums keep the add chain short.
template <bool SUB_M, int QT> __device__ __forceinline__ void exp_sum(f32x4 (&s)[4][QT], const float (&m_run)[QT], float (&l_run)[QT]) {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const float nm = m_run[qt];
        auto ex = [&](float x) { if constexpr (SUB_M) return __builtin_amdgcn_exp2f(x - nm); else return __builtin_amdgcn_exp2f(x); };
        float rs0 = 0.f, rs1 = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const float p0 = ex(s[kt][qt][0]), p1 = ex(s[kt][qt][1]);
            const float p2 = ex(s[kt][qt][2]), p3 = ex(s[kt][qt][3]);
            s[kt][qt][0] = p0; s[kt][qt][1] = p1; s[kt][qt][2] = p2; s[kt][qt][3] = p3;
            rs0 += p0 + p2; rs1 += p1 + p3;
        }
        l_run[qt] += rs0 + rs1;
    }
}
// ---- re-based online softmax of the LDS-DMA kernels, first half (exp_sum<false> is the second).  The score accumulators start at -m_run, so s holds
// d = score - m_run.  Dead keys -> -inf; row maximum of d; re-base when it exceeds 8 (deferred rescale, see attn_kernel: p <= 2^8 otherwise) and
// always on the first tile (m_run = 0 there is arbitrary; the re-base may go DOWN, so alpha is not used for it: l = o = 0).
template <int QT> __device__ __forceinline__ void start_rebased(f32x4 (&o)[4][QT], float (&m_run)[QT], float (&l_run)[QT]) {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        m_run[qt] = 0.f; l_run[qt] = 0.f;          // finite: the accumulators start at -m_run; the first tile always re-bases
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
template <int QT> __device__ __forceinline__ void softmax_rebase(f32x4 (&s)[4][QT], f32x4 (&o)[4][QT], float (&m_run)[QT], float (&l_run)[QT],
                                                                 bool first, int g, int kv0, int kvlen) {
    mask_dead_keys<8>(s, g, kv0, kvlen);
    float dmax[QT];
    bool grew = first;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        dmax[qt] = row_max16(s, qt);
        grew = grew || (dmax[qt] > 8.f);
    }
    if (__any(grew)) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            // per ROW: a row re-bases only on its own growth (shift 0 -> alpha = 1, s - 0: bit-exact no-ops), so a row's
            // arithmetic does not depend on which rows share its wave — workgroup shapes and batch composition cannot show
            const float shift = first ? dmax[qt] : (dmax[qt] > 8.f ? dmax[qt] : 0.f);
            const float alpha = first ? 0.f : __builtin_amdgcn_exp2f(-shift);
            l_run[qt] *= alpha;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt][qt] *= alpha;
            m_run[qt] += shift;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) s[kt][qt] -= shift;
        }
    }
}
// ---- normalise and store ctx[row][head*64 + d]; a wave owns the 16 * QT query rows from wave * 16 * QT on
template <int QT> __device__ __forceinline__ void store_ctx(float* ctx, const TileLoc& t, int head, int qlen, int wave, int lr, int g,
                                                            const f32x4 (&o)[4][QT], const float (&l_run)[QT]) {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        float l = l_run[qt];
        l = xor32_sum(xor16_sum(l));
        const float inv = 1.f / l;
        const int qrow = t.r0 + wave * (16 * QT) + qt * 16 + lr;
        if (qrow < qlen) {
            float* dst = ctx + (t.grow0 + wave * (16 * QT) + qt * 16 + lr) * 256LL + head * 64 + g * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4*>(dst + dt * 16) = o[dt][qt] * inv;
        }
    }
}
template <class Tag> __device__ __forceinline__ u32x4 mask_tail(u32x4 v, int nvalid) {  // keep the first nvalid elements of the chunk
    constexpr int EPC = Tag::EPC;
    if (nvalid >= EPC) return v;
    if (nvalid <= 0) return u32x4{0u, 0u, 0u, 0u};
    if constexpr (EPC == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) if (i >= nvalid) v[i] = 0u;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (2 * i >= nvalid) v[i] = 0u;
            else if (2 * i + 1 >= nvalid) v[i] &= 0xFFFFu;
        }
    }
    return v;
}
// K tile swizzle.  16-bit: a 16-lane ds_read_b128 group reads rows {8j + 4h + i : j, i = 0..3} (permuted key order), so
// the slot XOR is built from row bits 1, 3, 4 (8 values x 2 row parities = all 64 banks); f32 keeps lds_off<256>.
__device__ __forceinline__ int k_swz128(int row) { return ((row >> 1) & 1) | (((row >> 3) & 3) << 1); }
template <int ROWB> __device__ __forceinline__ int k_off(int row, int slot16) {
    if constexpr (ROWB == 128) return row * 128 + ((slot16 ^ k_swz128(row)) << 4);
    else return lds_off<ROWB>(row, slot16);
}
// ---- LDS-DMA source offsets (elements) of a wave's PPW pieces of a 64-row, 128-bytes-per-row tile: piece p = PPW * wave + i covers tile rows 8p .. 8p + 7 and lands at
// tile + 1024 p.  The DMA writes lane l's 16 bytes at piece base + 16 l, so the bank swizzle is applied on the SOURCE side: lane l fetches the logical slot that belongs at
// physical slot l & 7 of row l >> 3.  That is the inverse of k_off<128> (K) and of lds_off<128> (V^T); an XOR being its own inverse, both directions take their term from
// k_swz128 / lds_swz128 and MUST keep doing so: a swizzle changes there or nowhere.  koff: offset into the segment's K rows; vrow: the piece's V^T row pointer (+ kv0 per tile).
template <int PPW, class T> __device__ __forceinline__ void dma_lanes(int wave, int lane, const T* Vt, int head, long long R, long long kvbase,
                                                                      int (&koff)[PPW], const T* (&vrow)[PPW]) {
    const int prow = lane >> 3, pslot = lane & 7;
    int voff[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int row = (PPW * wave + i) * 8 + prow;
        koff[i] = row * 64 + ((pslot ^ k_swz128(row)) << 3);
        voff[i] = (pslot ^ lds_swz128(row)) << 3;
    }
#pragma unroll
    for (int i = 0; i < PPW; ++i) vrow[i] = Vt + ((long long)head * 64 + (PPW * wave + i) * 8 + prow) * R + kvbase + voff[i];
}
// ---- LDS fragment offsets of the DMA kernels, per k-chunk c one base for the K tiles and one for the V^T tiles (at vt in the buffer): the swizzle terms depend on the lane only
// (K: row bits 1, 3, 4; V^T: row bits 1..3), so tile (kt, dt) steps are immediate offsets and a k-chunk step (slot bit 2, inside the XOR) needs a second base register
__device__ __forceinline__ void frag_bases(int lr, int g, int vt, int (&kfo)[2], int (&vfo)[2]) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        kfo[c] = k_off<128>(key_of<8>(0, lr >> 2, lr & 3), c * 4 + g);
        vfo[c] = vt + lds_off<128>(lr, 4 * c + g);
    }
}
// ---- wave priority by progress (LDS-DMA kernels, set every fourth tile).  The SIMD arbiter issues oldest-wave-first, so of the 4 waves sharing a SIMD the first one ran at
// nearly solo speed and the last one at a third of it: workgroup lives spread 20 ... 57 us, the second round started ragged and the kernel ended with a 25 us ramp-down at <= 75 %
// occupancy (tools/attn_wall.py).  Priority by PROGRESS (the wave that is furthest behind issues first) makes the co-resident waves finish together: two sharp rounds, -3.5 %.
__device__ __forceinline__ void set_priority_by_progress(int tile, int ntiles) {
    if ((tile & 3) == 0) {
        const int q = (tile * 4) / ntiles;
        if (q == 0) __builtin_amdgcn_s_setprio(3); else if (q == 1) __builtin_amdgcn_s_setprio(2); else if (q == 2) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
    }
}
// ---- publish a DMA'd tile: "my pieces of this tile have landed" (and, first time round, my Q fragments) + barrier = the tile is complete AND every wave is done with the
// previous one, whose buffer may take the next.  The BUILTIN wait (wait_vmcnt0), not inline asm: hipcc's waitcnt pass must see it — it knows nothing of the asm DMAs, but it
// does track the Q fragment loads, and with an asm wait it still believed them in flight at their first use in the (peeled) first tile: its own vmcnt(0) there also waited for the
// NEXT tile's DMAs issued in between (in-order counter), i.e. one exposed DMA round trip per workgroup (ISA check: tools/check_isa.py).  The drain behind a tile loop stays inline asm.
__device__ __forceinline__ void publish_tile() {
    wait_vmcnt0();
    asm volatile("" ::: "memory");
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------
// Register-staged kernel: every precision, 16 / 32 / 64 rows per wave.  One LDS buffer, two barriers per tile (DESIGN.md has the double-buffered variants that lost); the classic
// online softmax (running maximum from -inf, scores exponentiated against it).
template <class Tag, int QT>
__global__ __launch_bounds__(ATHREADS) void attn_kernel(AttnArgs a) {
    constexpr int ABM = 64 * QT;
    typedef typename Tag::elem T;
    constexpr int EPC = Tag::EPC;
    constexpr int ROWB = 64 * (int)sizeof(T);     // bytes per LDS tile row (128 or 256)
    constexpr int SLOTS = ROWB / 16;              // 16-byte slots per row
    constexpr int NC = 64 / (4 * EPC);            // chunks along a 64-long contraction (2 or 4)
    constexpr int NCT = 64 * SLOTS / ATHREADS;    // staged chunks per thread per tile (2 or 4)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* bK = smem;                  // one K tile and one V^T tile
    char* bV = smem + 64 * ROWB;

    AttnWg w;
    if (!attn_workgroup<ABM>(a, w)) return;
    const int head = w.head, kvlen = w.kvlen;
    const long long kvbase = w.kvbase;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
    const long long R = a.R;
    const T* Q = static_cast<const T*>(a.q);
    const T* Kp = static_cast<const T*>(a.cross ? a.q : a.k);
    const T* Vt = static_cast<const T*>(a.vt);

    if (kvlen == 0) { zero_ctx_tile<ABM, ATHREADS>(a.ctx, w, tid); return; }

    // Q fragments (B operand of S^T = K Q^T): lane supplies query column lr, k-slots of group g
    u32x4 qf[QT][NC];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const long long grow = min((long long)w.t.grow0 + wave * (16 * QT) + qt * 16 + lr, R - 1);   // a 256-row tile may overhang the last segment
#pragma unroll
        for (int c = 0; c < NC; ++c)
            qf[qt][c] = *reinterpret_cast<const u32x4*>(Q + ((long long)head * R + grow) * 64 + c * 4 * EPC + g * EPC);
    }

    f32x4 o[4][QT];
    float m_run[QT], l_run[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        m_run[qt] = -INFINITY; l_run[qt] = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    u32x4 rk[NCT], rv[NCT];
    auto load_tile = [&](int kv0) {
#pragma unroll
        for (int i = 0; i < NCT; ++i) {
            const int c = tid + ATHREADS * i, row = c / SLOTS, slot = c % SLOTS;
            rk[i] = *reinterpret_cast<const u32x4*>(Kp + ((long long)head * R + kvbase + kv0 + row) * 64 + slot * EPC);
            rv[i] = *reinterpret_cast<const u32x4*>(Vt + ((long long)head * 64 + row) * R + kvbase + kv0 + slot * EPC);
        }
    };
    auto store_tile = [&](int kv0) {
        if (kv0 + ABK <= kvlen) {   // wave-uniform fast path: every key of the tile is live
#pragma unroll
            for (int i = 0; i < NCT; ++i) {
                const int c = tid + ATHREADS * i, row = c / SLOTS, slot = c % SLOTS;
                *reinterpret_cast<u32x4*>(bK + k_off<ROWB>(row, slot)) = rk[i];
                *reinterpret_cast<u32x4*>(bV + lds_off<ROWB>(row, slot)) = rv[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < NCT; ++i) {
                const int c = tid + ATHREADS * i, row = c / SLOTS, slot = c % SLOTS;
                // rows/keys past the live length may hold anything (uninitialised workspace): zero them so
                // that 0-probabilities never multiply a NaN
                const u32x4 kz = (kv0 + row < kvlen) ? rk[i] : u32x4{0u, 0u, 0u, 0u};
                *reinterpret_cast<u32x4*>(bK + k_off<ROWB>(row, slot)) = kz;
                *reinterpret_cast<u32x4*>(bV + lds_off<ROWB>(row, slot)) = mask_tail<Tag>(rv[i], kvlen - (kv0 + slot * EPC));
            }
        }
    };

    const int ntiles = (kvlen + ABK - 1) / ABK;
    PhaseClock pc;
    // ---- S^T = K Q^T  (4 key tiles x QT query tiles)
    auto qk = [&](f32x4 (&s)[4][QT]) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) s[kt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                const u32x4 kf = *reinterpret_cast<const u32x4*>(bK + k_off<ROWB>(key_of<EPC>(kt, lr >> 2, lr & 3), c * 4 + g));
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) mma_chunk<Tag>(s[kt][qt], kf, qf[qt][c]);
            }
        }
    };
    // ---- online softmax (fp32) of one tile's scores, per query column: decide and rescale here, exponentiate in exp_sum<true>
    auto smax_rescale = [&](f32x4 (&s)[4][QT], int kv0) {
        mask_dead_keys<EPC>(s, g, kv0, kvlen);
        float m_new[QT];
        bool grew = false;
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            m_new[qt] = vmax2(m_run[qt], row_max16(s, qt));
            grew = grew || (m_new[qt] > m_run[qt] + 8.f);
        }
        // Deferred rescale (guide T13): keep the stale running maximum while no row's maximum grew by more than 2^8
        // (base-2 units) — probabilities then reach at most 2^8 instead of 1, which costs nothing in the fp32 l / O
        // accumulators and nothing relative in the f16 / bf16 P operand.  Order is the textbook one: decide, rescale o
        // and l, THEN exponentiate this tile against the (possibly updated) maximum.  The first tile always takes the
        // branch (m_run = -inf); on most later tiles the O accumulators are not touched by the VALU at all.
        if (__any(grew)) {
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                // per ROW (see softmax_rebase): rows that did not grow keep their maximum, alpha = exp2(0) = 1 exactly
                const float m_upd = m_new[qt] > m_run[qt] + 8.f ? m_new[qt] : m_run[qt];
                const float alpha = __builtin_amdgcn_exp2f(m_run[qt] - m_upd);
                l_run[qt] *= alpha;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) o[dt][qt] *= alpha;
                m_run[qt] = m_upd;
            }
        }
    };
    // ---- O^T += V^T P^T
    auto pv = [&](f32x4 (&s)[4][QT]) {
        if constexpr (EPC == 8) {
#pragma unroll
            for (int tp = 0; tp < 2; ++tp) {
                u32x4 pp[QT];
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) pp[qt] = pack8<Tag>(s[2 * tp][qt], s[2 * tp + 1][qt]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const u32x4 vf = *reinterpret_cast<const u32x4*>(bV + lds_off<ROWB>(dt * 16 + lr, 4 * tp + g));   // keys 32tp + 8g .. +7
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) mma_chunk<Tag>(o[dt][qt], vf, pp[qt]);
                }
            }
        } else {
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const u32x4 vf = *reinterpret_cast<const u32x4*>(bV + lds_off<ROWB>(dt * 16 + lr, 4 * kt + g));
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) mma_chunk<Tag>(o[dt][qt], vf, __builtin_bit_cast(u32x4, s[kt][qt]));
                }
            }
        }
    };

    load_tile(0);
    f32x4 s[4][QT];
    for (int tile = 0; tile < ntiles; ++tile) {
        const int kv0 = tile * ABK;
        __syncthreads();
        ATT_TICK(pc, 0);
        store_tile(kv0);
        __syncthreads();
        ATT_TICK(pc, 1);
        load_tile(tile + 1 < ntiles ? kv0 + ABK : kv0);   // clamped, not branched (keeps hipcc's vmcnt counting exact)
        __builtin_amdgcn_sched_barrier(0);                // and pinned ahead of the MFMAs
        qk(s);
        ATT_TICK(pc, 2);
        smax_rescale(s, kv0);
        exp_sum<true>(s, m_run, l_run);
        ATT_TICK(pc, 4);
        pv(s);
        ATT_TICK(pc, 5);
    }
    dump_timing<4>(a, pc, ntiles);
    store_ctx(a.ctx, w.t, head, w.qlen, wave, lr, g, o, l_run);
}

// ---------------------------------------------------------------------------------------------------------------
// LDS-DMA variant of the 16-bit, 32-rows-per-wave kernel (the default operating point).  Same mathematics, same
// operand layouts, same instruction order inside a tile, so its output is bit-identical to attn_kernel<Tag, 2>.
// What changes is how a K / V^T tile reaches LDS and how often the workgroup synchronises:
//   * `global_load_lds_dwordx4`: each wave moves 2 + 2 pieces of 1 KB (8 rows x 128 B) per tile straight from L2 into
//     LDS (dma_lanes);
//   * two tile buffers (32 KB per workgroup, 4 workgroups per CU) and ONE barrier per tile (publish_tile): the buffer of
//     tile t - 1 takes tile t + 1 while tile t is being multiplied;
//   * no staging registers -> 128 VGPRs -> 4 waves per SIMD (was 3): at N = M = 1024, B = 32 the 2048 workgroups of a
//     launch are exactly 2 full rounds of the chip instead of 2.67;
//   * LDS fragment addresses as two per-lane bases + immediates (the swizzle depends on the lane only);
//   * wave priority by progress (set_priority_by_progress).
// A partial last tile is fixed up in LDS (V^T columns past the live length are zeroed: 0 x stale-NaN must not happen;
// K rows past it need nothing, their scores are overwritten with -inf).
template <class Tag>
__global__ __launch_bounds__(ATHREADS, 4) void attn_dma_kernel(AttnArgs a) {
    constexpr int QT = 2, ABM = 128, ROWB = 128, TILEB = 64 * ROWB, BUFB = 2 * TILEB;
    typedef typename Tag::elem T;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    AttnWg w;
    if (!attn_workgroup<ABM>(a, w)) return;
    const int head = w.head, kvlen = w.kvlen;
    const long long kvbase = w.kvbase;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, g = lane >> 4;
    const long long R = a.R;
    const T* Q = static_cast<const T*>(a.q);
    const T* Kp = static_cast<const T*>(a.cross ? a.q : a.k);
    const T* Vt = static_cast<const T*>(a.vt);

    if (kvlen == 0) { zero_ctx_tile<ABM, ATHREADS>(a.ctx, w, tid); return; }

    int koff[2];
    const T* vrow[2];
    dma_lanes<2>(wave, lane, Vt, head, R, kvbase, koff, vrow);
    const T* kseg = Kp + ((long long)head * R + kvbase) * 64;
    auto dma_tile = [&](int buf, int kv0) {
        char* bK = smem + buf * BUFB; char* bV = bK + TILEB;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            lds_dma16(kseg + (long long)kv0 * 64 + koff[i], bK + (2 * wave + i) * 1024);
            lds_dma16(vrow[i] + kv0, bV + (2 * wave + i) * 1024);
        }
    };
    dma_tile(0, 0);

    int kfo[2], vfo[2];
    frag_bases(lr, g, TILEB, kfo, vfo);
    u32x4 qf[QT][2];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const long long grow = (long long)w.t.grow0 + wave * 32 + qt * 16 + lr;
#pragma unroll
        for (int c = 0; c < 2; ++c) qf[qt][c] = *reinterpret_cast<const u32x4*>(Q + ((long long)head * R + grow) * 64 + c * 32 + g * 8);
    }
    f32x4 o[4][QT];
    float m_run[QT], l_run[QT];
    start_rebased(o, m_run, l_run);

    const int ntiles = (kvlen + ABK - 1) / ABK;
    PhaseClock pc;
    WallClock wc;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int kv0 = tile * ABK;
        const char* bK = smem + (tile & 1) * BUFB; const char* bV = bK + TILEB;
        set_priority_by_progress(tile, ntiles);
        publish_tile();
        ATT_TICK(pc, 0);
        if (kv0 + ABK > kvlen) {                            // workgroup-uniform: zero the dead key columns of V^T
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int c = tid + ATHREADS * i, row = c >> 3, slot = c & 7;
                u32x4* p = reinterpret_cast<u32x4*>(const_cast<char*>(bV) + lds_off<ROWB>(row, slot));
                *p = mask_tail<Tag>(*p, kvlen - (kv0 + slot * 8));
            }
            __syncthreads();
        }
        dma_tile((tile + 1) & 1, tile + 1 < ntiles ? kv0 + ABK : kv0);   // not branched (see attn_split_kernel); the last tile re-fetches itself into the idle buffer
        __builtin_amdgcn_sched_barrier(0);
        ATT_TICK(pc, 1);

        f32x4 s[4][QT];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) s[kt][qt] = f32x4{-m_run[qt], -m_run[qt], -m_run[qt], -m_run[qt]};   // scores arrive as s - m_run (the first MFMA of a chain reads this tuple as its C operand)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                const u32x4 kf = *reinterpret_cast<const u32x4*>(bK + kfo[c] + key_of<8>(kt, 0, 0) * ROWB);   // key row key_of<8>(kt, lr >> 2, lr & 3)
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) mma_chunk<Tag>(s[kt][qt], kf, qf[qt][c]);
            }
        }
        ATT_TICK(pc, 2);
        softmax_rebase(s, o, m_run, l_run, tile == 0, g, kv0, kvlen);
        ATT_TICK(pc, 3);
        exp_sum<false>(s, m_run, l_run);
        ATT_TICK(pc, 4);
#pragma unroll
        for (int tp = 0; tp < 2; ++tp) {
            u32x4 pp[QT];
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) pp[qt] = pack8<Tag>(s[2 * tp][qt], s[2 * tp + 1][qt]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const u32x4 vf = *reinterpret_cast<const u32x4*>(bK + vfo[tp] + dt * 16 * ROWB);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) mma_chunk<Tag>(o[dt][qt], vf, pp[qt]);
            }
        }
        ATT_TICK(pc, 5);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the last (redundant) tile fetch must have landed before this wave's LDS can be released
    dump_timing<4>(a, pc, ntiles);
    dump_wall<4>(a, wc, ntiles);
    store_ctx(a.ctx, w.t, head, w.qlen, wave, lr, g, o, l_run);
}

// one of a group's three products: acc[first + j][qt] += a[j] x b[qt][c] for the group's two tiles j
template <int QT> __device__ __forceinline__ void mma_pair(f32x4 (&acc)[4][QT], int first, const u32x4 (&a)[2], const u32x4 (&b)[QT][2], int c) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) mma_chunk<TagF16>(acc[first + j][qt], a[j], b[qt][c]);
}
// ---------------------------------------------------------------------------------------------------------------
// SPLIT-f16 attention (attention precision PREC_F16X3, the default): q, k, v arrive as hi + lo f16 planes (lg_proj_body.h,
// 22 operand bits) and the probabilities are split the same way, so both contractions run as three MFMAs per product
//      S^T = Kh Ql^T + Kl Qh^T + Kh Qh^T          O^T = Vh^T Pl^T + Vl^T Ph^T + Vh^T Ph^T
// with fp32 accumulation.  Why: with one f16 plane a base-2 logit of magnitude 30 carries an absolute error of ~1e-2, i.e. 1 % on
// the softmax weights — invisible while attention is diffuse (random-weight fixtures), 2e-2 in the matching scores once the logit
// spread reaches 25 (recipe-D fixtures, DESIGN.md §1: QK^T alone 1.4e-2, P V alone 5e-3; split: 5e-5 / < 5e-4).  There is no cheaper
// operand format with >= 17 bits on gfx950 (no xf32; fp32 MFMA runs at 1/16 of the f16 rate).
// Structure = attn_dma_kernel: LDS-DMA tiles, two buffers, one barrier per tile, wave priority by progress, scores accumulated
// from -m_run.  A buffer holds four 8 KB tiles (K hi, K lo, V^T hi, V^T lo): 64 KB per workgroup, two workgroups per CU.
// QT = 16-row query tiles per wave, NW = waves per workgroup.  Shapes (round-3 A/B at cfg #2, one box each): 8 waves x 16 rows
// (108 VGPRs, four waves per SIMD; the product shape, and 4 x 16 rows = 64-row workgroups for under-filled grids) is 2-3 % faster
// than 4 waves x 32 rows (172 VGPRs, two waves per SIMD).  Lost: a cross-tile software pipeline (S(t+1) MFMAs interleaved with the
// softmax VALU of tile t inside each wave via sched_group_barrier: bit-identical, +7 % time).  SQ counters of the kernel: matrix
// pipe 54 % busy, waves 42 % issue-stalled, 25 % parked; timing ablations: no DMA -9 %, no exponentials -4 % — LAB_NOTES.md.
// Round 6: a PING-PONG form (the two waves a workgroup has on a SIMD half a tile apart — one multiplies while the other runs its softmax —, two barriers per
// tile, K(t + 1) requested behind the first and V(t + 1) behind the second; bit-identical; tools/experiments/attn_pingpong.patch) took MORE cycles per workgroup
// (64.9k vs 63.5k) and +2 ... +6 % time; priorities by phase or none at all: noise.  The kernel is not bound by when its waves do what: inside a forward the chip
// sits at its 1.35 kW power limit and runs this kernel at 1.64 GHz of 2.4 (profiles/r06b_attn_wall_clock.log) — what moves it is energy per tile.
template <int QT, int NW>
__global__ __launch_bounds__(NW * 64, NW / 2) void attn_split_kernel(AttnArgs a) {
    typedef TagF16 Tag;
    typedef f16_t T;
    constexpr int NT = NW * 64, PPW = 8 / NW;      // threads; DMA pieces per wave per (plane, tile)
    constexpr int ABM = 16 * QT * NW, ROWB = 128, TILEB = 64 * ROWB, BUFB = 4 * TILEB;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    AttnWg w;
    if (!attn_workgroup<ABM>(a, w)) return;
    const int head = w.head, kvlen = w.kvlen;
    const long long kvbase = w.kvbase;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, g = lane >> 4;
    const long long R = a.R, PL = a.plane;
    const T* Q = static_cast<const T*>(a.q);
    const T* Kp = static_cast<const T*>(a.cross ? a.q : a.k);
    const T* Vt = static_cast<const T*>(a.vt);

    if (kvlen == 0) { zero_ctx_tile<ABM, NT>(a.ctx, w, tid); return; }

    int koff[PPW];
    const T* vrow[PPW];
    dma_lanes<PPW>(wave, lane, Vt, head, R, kvbase, koff, vrow);   // the same piece of each of the four tiles
    const T* kseg = Kp + ((long long)head * R + kvbase) * 64;
    auto dma_tile = [&](int buf, int kv0) {
        char* bK = smem + buf * BUFB;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const T* ks = kseg + (long long)kv0 * 64 + koff[i];
            const T* vs = vrow[i] + kv0;
            char* dst = bK + (PPW * wave + i) * 1024;
            lds_dma16(ks, dst); lds_dma16(ks + PL, dst + TILEB);
            lds_dma16(vs, dst + 2 * TILEB); lds_dma16(vs + PL, dst + 3 * TILEB);
        }
    };
    dma_tile(0, 0);

    int kfo[2], vfo[2];
    frag_bases(lr, g, 2 * TILEB, kfo, vfo);
    u32x4 qh[QT][2], ql[QT][2];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const long long grow = (long long)w.t.grow0 + wave * (16 * QT) + qt * 16 + lr;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const T* src = Q + ((long long)head * R + grow) * 64 + c * 32 + g * 8;
            qh[qt][c] = *reinterpret_cast<const u32x4*>(src);
            ql[qt][c] = *reinterpret_cast<const u32x4*>(src + PL);
        }
    }
    f32x4 o[4][QT];
    float m_run[QT], l_run[QT];
    start_rebased(o, m_run, l_run);

    const int ntiles = (kvlen + ABK - 1) / ABK;
    PhaseClock pc;
    WallClock wc;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int kv0 = tile * ABK;
        const char* bK = smem + (tile & 1) * BUFB;
        set_priority_by_progress(tile, ntiles);
        publish_tile();
        ATT_TICK(pc, 0);
        if (kv0 + ABK > kvlen) {                            // workgroup-uniform: zero the dead key columns of both V^T planes
#pragma unroll
            for (int i = 0; i < 1024 / NT; ++i) {         // 512 16-byte chunks per plane
                const int c = (tid + NT * i) & 511, plane = (tid + NT * i) >> 9, row = c >> 3, slot = c & 7;
                u32x4* p = reinterpret_cast<u32x4*>(const_cast<char*>(bK) + (2 + plane) * TILEB + lds_off<ROWB>(row, slot));
                *p = mask_tail<Tag>(*p, kvlen - (kv0 + slot * 8));
            }
            __syncthreads();
        }
        // Fragment reads are software-pipelined one group ahead of the MFMAs (two register sets; sched_barrier pins the order —
        // hipcc otherwise sinks every ds_read next to its use and each group of 12 MFMAs starts with an exposed LDS round trip,
        // 16 of them per tile, with only two waves per SIMD to cover).  Group = (k-chunk, pair of key tiles) for S^T and
        // (P chunk, pair of d tiles) for O^T; the first V^T group is fetched during the last K group, so that its latency
        // hides under the softmax.
        u32x4 fh[2][2], fl[2][2];
        auto load_k = [&](int grp, u32x4 (&h)[2], u32x4 (&l)[2]) {
            const int c = grp >> 1, kp = grp & 1;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const char* src = bK + kfo[c] + key_of<8>(2 * kp + j, 0, 0) * ROWB;   // key row key_of<8>(kt, lr >> 2, lr & 3), kt = 2 kp + j
                h[j] = *reinterpret_cast<const u32x4*>(src);
                l[j] = *reinterpret_cast<const u32x4*>(src + TILEB);
            }
        };
        auto load_v = [&](int grp, u32x4 (&h)[2], u32x4 (&l)[2]) {
            const int tp = grp >> 1, dp = grp & 1;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const char* src = bK + vfo[tp] + (2 * dp + j) * 16 * ROWB;
                h[j] = *reinterpret_cast<const u32x4*>(src);
                l[j] = *reinterpret_cast<const u32x4*>(src + TILEB);
            }
        };
        load_k(0, fh[0], fl[0]);
        // NOT branched around: hipcc merges its s_waitcnt bookkeeping conservatively at a join, and every fragment wait of the tile
        // became lgkmcnt(0) — i.e. the prefetched group was waited for as well (measured in the ISA).  The last tile re-fetches
        // itself into the idle buffer instead; the wave drains vmcnt before it leaves the loop (no DMA may land after the exit).
        dma_tile((tile + 1) & 1, tile + 1 < ntiles ? kv0 + ABK : kv0);
        __builtin_amdgcn_sched_barrier(0);
        ATT_TICK(pc, 1);

        // ---- S^T - m_run: per k-chunk and pair of key tiles, three products over 2 x QT independent accumulators
        f32x4 s[4][QT];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) s[kt][qt] = f32x4{-m_run[qt], -m_run[qt], -m_run[qt], -m_run[qt]};
#pragma unroll
        for (int grp = 0; grp < 4; ++grp) {
            const int c = grp >> 1, kp = grp & 1;
            if (grp < 3) load_k(grp + 1, fh[(grp + 1) & 1], fl[(grp + 1) & 1]);
            else load_v(0, fh[0], fl[0]);
            __builtin_amdgcn_sched_barrier(0);
            const u32x4 (&kh)[2] = fh[grp & 1];
            const u32x4 (&kl)[2] = fl[grp & 1];
            mma_pair(s, 2 * kp, kh, ql, c);
            mma_pair(s, 2 * kp, kl, qh, c);
            mma_pair(s, 2 * kp, kh, qh, c);
            __builtin_amdgcn_sched_barrier(0);
        }
        ATT_TICK(pc, 2);
        softmax_rebase(s, o, m_run, l_run, tile == 0, g, kv0, kvlen);
        ATT_TICK(pc, 3);
        exp_sum<false>(s, m_run, l_run);
        ATT_TICK(pc, 4);
        // ---- O^T += V^T P^T with P = Ph + Pl (both f16; the residual p - Ph is exact in fp32): three products per (d tile, query tile)
        u32x4 ph[QT][2], pl[QT][2];
#pragma unroll
        for (int tp = 0; tp < 2; ++tp)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) split8_f16<true>(s[2 * tp][qt], s[2 * tp + 1][qt], ph[qt][tp], pl[qt][tp]);
#pragma unroll
        for (int grp = 0; grp < 4; ++grp) {
            const int tp = grp >> 1, dp = grp & 1;
            if (grp < 3) load_v(grp + 1, fh[(grp + 1) & 1], fl[(grp + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            const u32x4 (&vh)[2] = fh[grp & 1];
            const u32x4 (&vl)[2] = fl[grp & 1];
            mma_pair(o, 2 * dp, vh, pl, tp);
            mma_pair(o, 2 * dp, vl, ph, tp);
            mma_pair(o, 2 * dp, vh, ph, tp);
            __builtin_amdgcn_sched_barrier(0);
        }
        ATT_TICK(pc, 5);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the last (redundant) tile fetch must have landed before this wave's LDS can be released
    dump_timing<NW>(a, pc, ntiles);
    dump_wall<NW>(a, wc, ntiles);
    store_ctx(a.ctx, w.t, head, w.qlen, wave, lr, g, o, l_run);
}

template <int QT, int NW> static hipError_t launch_attn_split(const AttnArgs& a, hipStream_t s) {
    if (a.plane <= 0) return hipErrorInvalidValue;
    return launch_with_lds(attn_split_kernel<QT, NW>, dim3(attention_tiles(a.rs, 16 * QT * NW) * 4), dim3(NW * 64), 2 * 4 * 64 * 128, s, a);
}

template <class Tag> static hipError_t launch_attn_dma(const AttnArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((attn_dma_kernel<Tag>), dim3(attention_tiles(a.rs, 128) * 4), dim3(ATHREADS), 2 * 2 * 64 * 128, s, a);
    return hipGetLastError();
}

template <class Tag, int QT> static hipError_t launch_attn_t(const AttnArgs& a, hipStream_t s) {
    constexpr int smem = 2 * 64 * 64 * (int)sizeof(typename Tag::elem);
    hipLaunchKernelGGL((attn_kernel<Tag, QT>), dim3(attention_tiles(a.rs, 64 * QT) * 4), dim3(ATHREADS), smem, s, a);
    return hipGetLastError();
}

// 16-bit operands.  a.rows_per_wave: 32 (two 16-row query tiles per wave, three waves per SIMD; with a.dma the LDS-DMA kernel), 64 (four tiles,
// two waves per SIMD, K/V fragments reused twice as often) or 16
template <class Tag> static hipError_t launch_attn_16bit(const AttnArgs& a, hipStream_t s) {
    const int rpw = a.rows_per_wave;
    if (a.dma && rpw == 32) return launch_attn_dma<Tag>(a, s);
    return rpw == 64 ? launch_attn_t<Tag, 4>(a, s) : rpw == 16 ? launch_attn_t<Tag, 1>(a, s) : launch_attn_t<Tag, 2>(a, s);
}

hipError_t launch_attention(int attn_prec, const AttnArgs& a, hipStream_t s) {
    switch (attn_prec) {
        case PREC_F32: return launch_attn_t<TagF32, 2>(a, s);
        case PREC_BF16: return launch_attn_16bit<TagBF16>(a, s);
        case PREC_F16: return launch_attn_16bit<TagF16>(a, s);
        case PREC_F16X3: return a.rows_per_wave == 16 ? launch_attn_split<1, 4>(a, s) : launch_attn_split<1, 8>(a, s);   // 64-row workgroups for under-filled grids, else 128-row ones (8 waves x 16 rows)
    }
    return hipErrorInvalidValue;
}

}  // namespace lg
