// lightglue_amd — what one forward of the matcher engine consists of, decided before anything is enqueued: the engine options (ForwardOptions) and the
// launch plan of a call (ForwardPlan, plan_forward).  lg_engine.hip runs the plan in three stages and decides nothing itself.  Host-only C++17: no HIP
// header and no device type, so tests/cpp/forward_plan_check.cpp checks the whole decision table with any host compiler.
#pragma once
#include <cstdint>

#include "../../include/lightglue_amd.h"

namespace lg {

// What lg_engine_set_option and lg_engine_debug_stop_after write (lg_engine::opt)
struct ForwardOptions {
    int fused_tail = 1, fused_next = 1, fused_prep = 1;   // fused_prep: the per-keypoint preparation inside the first projection launch (input_dim == 256, no SIFT-store flag)
    // gather path of the adaptive width (round 6, default on): the SelfBlock projection behind a pruning step reads rows from one set of residual / rotary
    // buffers and writes the compacted rows to the other (lg_proj.hip proj_rows_kernel<GatherRows>)
    bool adapt_gather = true;
    // split-f16 precision: the final projection stores f16 hi / lo planes and the similarity matrix is sim_planes_kernel (lg_sim.hip); 0 = fp32 rows + the generic sim_kernel (bit-identical)
    bool sim_planes = true;
    int sim_chunk = 0;      // image-1 rows per sim_planes workgroup, 0 = by grid fill (option "sim_chunk": tests / A-B; bit-identical)
    bool attn_dma = true;   // option "attn_dma": LDS-DMA attention kernel (16-bit operands, 32 rows per wave)
    int attn_rows = 32;     // query rows per attention wave (32 | 64), option "attn_rows" / env LG_ATTN_ROWS
    bool attn_auto_rows = true;   // small grids: 16 query rows per attention wave (twice the workgroups); off once "attn_rows" is set
    int tail_row_tiles = 0;   // option "tail_row_tiles": 16-row tiles per fused-tail workgroup; 0 = by grid fill (4 | 2 | 1)
    // 1: tail kernel, 2: self projection, 3: self attention (LG_ATTN_TIMING builds), 4: assign sweeps, 5 / 6: layer 0's CrossBlock / SelfBlock tail WITH its fused
    // next projection (stamps of the projection in TAILDBG2)
    int tail_timing = 0;
    int debug_stop = -1;    // lg_engine_debug_stop_after: the forward returns once this step is done (steps: BlockPlan::first_step), -1 = run to the end
};

inline bool pruning_on(const lg_config& cfg, uint32_t io_flags) { return cfg.width_confidence > 0 && !(io_flags & LG_FLAG_NO_PRUNING); }
// LG_FLAG_INDEXED: the index fields sit behind the round-5 extension, so they are read only when both flags are set (check_forward_io refuses one without the other)
inline bool indexed(uint32_t io_flags) { return (io_flags & LG_FLAG_EXT) && (io_flags & LG_FLAG_INDEXED); }

// ---- the storage format of one side's descriptors, decoded once from the call's flags (check_forward_io validates it, forward_ctx hands it to the kernels as PrepSide)
enum : int { DESC_F32 = 0, DESC_F16 = 1, DESC_U8 = 2 };   // how a descriptor row is stored (lg_rootsift's src_kind); lg_side.h loads each
struct SideFormat {
    int kind;         // DESC_*: LG_FLAG_DESC{side}_U8 / _F16, else fp32
    bool rootsift;    // LG_FLAG_ROOTSIFT{side}: every widened row is replaced by its RootSIFT where it enters
    bool valid;       // false: a storage flag of the side without LG_FLAG_EXT, or _U8 and _F16 together (a store has one format)
};
// The flags of side 0 / 1 lie one bit apart.  They sit behind the round-5 extension: without LG_FLAG_EXT every one of them is off.
static_assert(LG_FLAG_DESC1_F16 == LG_FLAG_DESC0_F16 << 1 && LG_FLAG_DESC1_U8 == LG_FLAG_DESC0_U8 << 1 && LG_FLAG_ROOTSIFT1 == LG_FLAG_ROOTSIFT0 << 1, "side 1's flag = side 0's << 1");
inline SideFormat side_format(uint32_t io_flags, int side) {
    const bool f16 = io_flags & (LG_FLAG_DESC0_F16 << side), u8 = io_flags & (LG_FLAG_DESC0_U8 << side), root = io_flags & (LG_FLAG_ROOTSIFT0 << side);
    if (!(io_flags & LG_FLAG_EXT)) return {DESC_F32, false, !(f16 || u8 || root)};
    return {u8 ? DESC_U8 : f16 ? DESC_F16 : DESC_F32, root, !(u8 && f16)};
}

enum class ProjBy {     // how a block's q/k/v come about
    PrevTail,           // the previous block's tail kernel has already produced them (fused_next)
    Own,                // the block's own projection launch (lg_proj.hip)
    OwnFirst,           // ... with the per-keypoint preparation fused in (fused_prep; layer 0's SelfBlock)
    OwnGather           // ... moving every pruning pair's rows to the other buffer set on their way in (adapt_gather; a SelfBlock behind a pruning step)
};
enum class TailNext { None, NextProj, FinalProj };   // what a fused tail kernel runs on the x tile it has just produced
enum class AdaptMode { None, StopOnly, PruneInPlace, PruneGather };   // the adaptive step behind a layer (lg_adaptive.hip)
inline bool prunes(AdaptMode m) { return m == AdaptMode::PruneInPlace || m == AdaptMode::PruneGather; }

struct BlockPlan {
    ProjBy proj_by;
    TailNext tail_next;     // None on the per-op path
    // 256 -> 1 heads on the rows a CrossBlock tail produces (all false for a SelfBlock): token confidence of the layer (ref :548) for the stop decision;
    // matchability of the layer (ref :298-299): its sigmoid for the pruning mask (ref :553) and its log-sigmoids as the assignment's matchability terms
    // (ref :268-276) wherever a pair may END at this layer — the last one, or any one with early stopping
    bool want_tok, prune_here, want_ls, want_lsneg;
    // debug steps (lg_engine_debug_stop_after, tests/gpu_util.py): step 0 is the preparation; a block takes six — first_step its projection, + 1 attention,
    // + 2 .. + 5 out_proj, ffn.0, LayerNorm + GELU, ffn.3 + residual, which a fused tail completes all at once
    int first_step;
    // the set of residual / rotary buffers the block works in (0 = X / COS / SIN, 1 = X2 / COS2 / SIN2); an OwnGather projection reads the other one
    int buf_set;
};

// Every whole-call decision of a forward, and — block() / after_layer() — what each block and each layer boundary does.  All of it O(1) arithmetic.
struct ForwardPlan {
    int n_layers, debug_stop;
    bool fused_tail;
    bool do_stop, do_prune;
    bool prune_possible;    // below the threshold the pruning branch is never taken (ref :551 / :559; lengths only shrink)
    bool check_finite;
    bool fuse_prep;         // prep (+ descriptor copy) inside the first projection launch (lg_proj.hip proj_rows_kernel<FirstRows>) instead of its own
    bool fuse_next;         // a tail kernel also runs the NEXT block's projection on the x tile it has just produced
    bool use_gather;        // the product configuration only (the per-op / debug-stop paths keep the in-place compaction kernel, which the tests compare it with)
    bool sim_planes;
    bool split_qkv;         // split attention: q / k / v^T are an f16 hi plane, then an f16 lo plane
    bool all_rows_live;     // every row of the row space is a keypoint of its pair (indexed: a pair whose index is out of range has no live row)
    bool wants_log_assignment;

    bool stops_at(int step) const { return debug_stop >= 0 && step >= debug_stop; }
    int last_step() const { return 12 * n_layers; }

    // the adaptive step behind `layer` (ref :544-566); none behind the last one
    AdaptMode after_layer(int layer) const {
        if (layer < 0 || layer + 1 >= n_layers) return AdaptMode::None;
        if (prune_possible) return use_gather ? AdaptMode::PruneGather : AdaptMode::PruneInPlace;
        return do_stop ? AdaptMode::StopOnly : AdaptMode::None;
    }

    // Across a layer boundary the fusion is valid whenever no row can MOVE in between: early stop alone only deactivates a pair (its speculative
    // projection is never read), pruning re-orders rows — but it cannot happen while every segment is at or below the pruning threshold.
    // Fixed depth: every live pair ends at the last layer, so the LAST tail runs the final projection of the log assignment instead.
    TailNext tail_next(int layer, int blk) const {
        if (!fuse_next) return TailNext::None;
        const bool last = layer + 1 == n_layers;
        if (blk == 0 || (!last && !prune_possible)) return TailNext::NextProj;
        return last && !do_stop ? TailNext::FinalProj : TailNext::None;
    }

    // blk 0 = SelfBlock (ref :159-172), 1 = CrossBlock (ref :201-230)
    BlockPlan block(int layer, int blk) const {
        BlockPlan b{};
        const bool first = layer == 0 && blk == 0, last = layer + 1 == n_layers;
        if (!first && tail_next(layer - (blk ^ 1), blk ^ 1) == TailNext::NextProj) b.proj_by = ProjBy::PrevTail;
        else if (first && fuse_prep) b.proj_by = ProjBy::OwnFirst;
        else if (blk == 0 && after_layer(layer - 1) == AdaptMode::PruneGather) b.proj_by = ProjBy::OwnGather;
        else b.proj_by = ProjBy::Own;
        b.tail_next = tail_next(layer, blk);
        if (blk == 1) {
            b.want_tok = !last && do_stop; b.prune_here = !last && prune_possible;
            b.want_ls = last || do_stop; b.want_lsneg = b.want_ls && wants_log_assignment;
        }
        b.first_step = 1 + 12 * layer + 6 * blk;
        // every gather projection flips the set, and one runs in each SelfBlock behind a PruneGather step: all layers but the first
        b.buf_set = after_layer(0) == AdaptMode::PruneGather ? layer & 1 : 0;
        return b;
    }

    // the final projection runs as its own launch over every pair (with the weights of the layer each pair stopped at) unless the last tail ran it
    bool final_proj_in_last_tail() const { return tail_next(n_layers - 1, 1) == TailNext::FinalProj; }
};

// has_counts: the call carries per-pair keypoint counts (num0 / num1); tail_supports_next: launch_tail_supports_next(precision, attn_prec), passed in so
// that this header needs no kernel header
inline ForwardPlan plan_forward(const lg_config& cfg, int attn_prec, const ForwardOptions& opt, int n0, int n1, uint32_t io_flags, bool has_counts,
                                bool wants_log_assignment, bool tail_supports_next) {
    ForwardPlan p{};
    p.n_layers = cfg.n_layers; p.debug_stop = opt.debug_stop; p.fused_tail = opt.fused_tail != 0; p.wants_log_assignment = wants_log_assignment;
    p.do_stop = cfg.depth_confidence > 0; p.do_prune = pruning_on(cfg, io_flags);
    p.prune_possible = p.do_prune && (n0 > cfg.pruning_min_kpts || n1 > cfg.pruning_min_kpts);
    p.check_finite = (io_flags & LG_FLAG_EXT) && (io_flags & LG_FLAG_CHECK_FINITE);
    // SIFT stores (uint8 rows, RootSIFT on entry) are read by prep_kernel alone: such a call takes the two-launch form, which is bit-identical
    const bool sift_store = (io_flags & LG_FLAG_EXT) && (io_flags & LG_SIFT_STORE_FLAGS);
    p.fuse_prep = opt.fused_prep && cfg.input_dim == 256 && opt.debug_stop < 0 && opt.tail_timing != 2 && !sift_store;
    p.fuse_next = opt.fused_next && opt.fused_tail && (opt.tail_timing == 0 || opt.tail_timing == 5 || opt.tail_timing == 6) &&
                  opt.debug_stop < 0 && tail_supports_next;
    p.use_gather = opt.adapt_gather && opt.fused_tail && opt.debug_stop < 0 && opt.tail_timing == 0;
    p.sim_planes = cfg.precision == LG_PREC_F16X3 && opt.sim_planes;
    p.split_qkv = attn_prec == LG_PREC_F16X3;
    p.all_rows_live = !p.do_prune && !has_counts && !indexed(io_flags);
    return p;
}

}  // namespace lg
