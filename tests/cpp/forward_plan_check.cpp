// Checks the launch plan of the matcher engine's forward (lightglue_amd/csrc/lg_forward_plan.h) on the host: every rule below is restated from what a
// forward has to do (ref lightglue.py:483-629 and the engine's fusion options), then asserted at every point of the grid.  Stand-alone: built and run by
// tests/test_forward_plan_cpu.py; exit status 0 and "ok <points>" on success, the first violated rule otherwise.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../lightglue_amd/csrc/lg_forward_plan.h"

using namespace lg;

namespace {

struct Point {
    int L, n0, n1, input_dim;
    bool depth, width, counts, wants_log, supports_next;
    uint32_t flags;
    ForwardOptions opt;
};

const int kMinKpts = 64;
long long g_points = 0;

[[noreturn]] void fail(const Point& p, const char* rule, int layer, int blk) {
    std::printf("FAILED: %s at layer %d block %d\n  n_layers %d depth %d width %d flags %u n0 %d n1 %d input_dim %d counts %d log %d\n"
                "  fused_tail %d fused_next %d fused_prep %d adapt_gather %d tail_timing %d debug_stop %d tail_supports_next %d\n",
                rule, layer, blk, p.L, p.depth, p.width, p.flags, p.n0, p.n1, p.input_dim, p.counts, p.wants_log,
                p.opt.fused_tail, p.opt.fused_next, p.opt.fused_prep, p.opt.adapt_gather, p.opt.tail_timing, p.opt.debug_stop, p.supports_next);
    std::exit(1);
}
#define CHECK(cond, rule) do { if (!(cond)) fail(p, rule, layer, blk); } while (0)

void check_point(const Point& p) {
    ++g_points;
    lg_config cfg{};
    cfg.input_dim = p.input_dim; cfg.descriptor_dim = 256; cfg.n_layers = p.L; cfg.num_heads = 4;
    cfg.depth_confidence = p.depth ? 0.95 : -1.0; cfg.width_confidence = p.width ? 0.99 : -1.0;
    cfg.pruning_min_kpts = kMinKpts; cfg.precision = LG_PREC_F16X3; cfg.attn_precision = -1;
    const ForwardPlan plan = plan_forward(cfg, LG_PREC_F16X3, p.opt, p.n0, p.n1, p.flags, p.counts, p.wants_log, p.supports_next);
    int layer = -1, blk = -1;

    // ---- what the call is, in the reference's terms
    const bool pruning = p.width && !(p.flags & LG_FLAG_NO_PRUNING);                 // ref :529
    const bool rows_can_move = pruning && (p.n0 > kMinKpts || p.n1 > kMinKpts);      // ref :551 / :559: a segment at or below the threshold never prunes
    const bool ext = (p.flags & LG_FLAG_EXT) != 0;
    const bool is_indexed = ext && (p.flags & LG_FLAG_INDEXED);
    // ---- what the options allow: the fused forms are the product path only, and a timing tap keeps the kernel it times on its own
    const bool product = p.opt.debug_stop < 0;
    const int t = p.opt.tail_timing;
    const bool next_on = product && p.opt.fused_tail && p.opt.fused_next && (t == 0 || t == 5 || t == 6) && p.supports_next;
    const bool prep_on = product && p.opt.fused_prep && p.input_dim == 256 && t != 2;
    const bool gather_on = product && p.opt.fused_tail && p.opt.adapt_gather && t == 0;

    CHECK(plan.do_stop == p.depth && plan.do_prune == pruning && plan.prune_possible == rows_can_move, "whole-call adaptive decisions");
    CHECK(plan.check_finite == (ext && (p.flags & LG_FLAG_CHECK_FINITE) != 0), "check_finite needs LG_FLAG_EXT and LG_FLAG_CHECK_FINITE");
    CHECK(plan.all_rows_live == !(pruning || p.counts || is_indexed), "all_rows_live is false whenever pruning, num0 / num1 or LG_FLAG_INDEXED is in play");
    CHECK(plan.fuse_prep == prep_on && plan.fuse_next == next_on && plan.use_gather == gather_on, "fusion / gather flags");
    CHECK(plan.fused_tail == (p.opt.fused_tail != 0), "fused_tail");
    CHECK(plan.last_step() == 12 * p.L, "the last step is 12 * n_layers");
    CHECK(plan.stops_at(0) == (p.opt.debug_stop == 0) && plan.stops_at(7) == (p.opt.debug_stop >= 0 && p.opt.debug_stop <= 7) &&
          plan.stops_at(6) == (p.opt.debug_stop >= 0 && p.opt.debug_stop <= 6), "stops_at");

    // ---- walk the forward in launch order, carrying what a sequential launch loop would carry
    bool prev_tail_projected = false;     // the preceding block's tail has produced this block's q/k/v
    bool move_pending = false;          // the preceding layer's adaptive step left the row move to the next SelfBlock projection
    int cur_set = 0;                      // buffer set the residual stream is in
    int final_in_tail = 0;
    for (layer = 0; layer < p.L; ++layer) {
        const bool last = layer + 1 == p.L;
        for (blk = 0; blk < 2; ++blk) {
            const BlockPlan b = plan.block(layer, blk);
            // q/k/v: exactly one producer
            CHECK((b.proj_by == ProjBy::PrevTail) == prev_tail_projected, "q/k/v have exactly one producer: PrevTail exactly when the preceding tail ran NextProj");
            CHECK((b.proj_by == ProjBy::OwnFirst) == (prep_on && layer == 0 && blk == 0), "OwnFirst: the first projection, when the preparation is fused in");
            CHECK((b.proj_by == ProjBy::OwnGather) == (move_pending && blk == 0), "OwnGather only on a SelfBlock whose preceding after_layer is in gather mode");
            if (b.proj_by == ProjBy::OwnGather) { cur_set ^= 1; move_pending = false; }
            CHECK(!move_pending, "a pending row move is taken up by the very next projection");
            CHECK(b.buf_set == cur_set, "the current buffer set flips exactly at a gather projection");
            CHECK(b.first_step == 1 + 12 * layer + 6 * blk, "steps are 1 + 12 * layer + 6 * blk");
            // the tail
            const bool boundary = blk == 1;   // the next block, if any, belongs to the next layer
            if (b.tail_next == TailNext::NextProj) {
                CHECK(!(boundary && last), "no projection behind the last block");
                CHECK(!(boundary && rows_can_move), "no projection is fused across a layer boundary when prune_possible holds");
            }
            if (b.tail_next == TailNext::FinalProj) {
                CHECK(boundary && last, "FinalProj only in the last CrossBlock's tail");
                CHECK(!p.depth, "FinalProj only without early stopping");
                ++final_in_tail;
            }
            if (!next_on) CHECK(b.tail_next == TailNext::None, "no tail fusion under a debug stop, with fused_tail / fused_next off, or while a kernel is timed");
            else CHECK(b.tail_next == (!boundary ? TailNext::NextProj : last ? (p.depth ? TailNext::None : TailNext::FinalProj)
                                                                             : (rows_can_move ? TailNext::None : TailNext::NextProj)), "an enabled tail fusion is used wherever it is valid");
            prev_tail_projected = b.tail_next == TailNext::NextProj;
            // heads of a CrossBlock tail: where a pair may stop, prune or end
            if (blk == 0) CHECK(!b.want_tok && !b.prune_here && !b.want_ls && !b.want_lsneg, "a SelfBlock tail has no heads");
            else {
                CHECK(b.want_tok == (p.depth && !last), "token confidence wherever a stop decision follows");
                CHECK(b.prune_here == (rows_can_move && !last), "matchability sigmoid wherever a pruning step follows");
                CHECK(b.want_ls == (last || p.depth), "matchability terms wherever a pair may end");
                CHECK(b.want_lsneg == (b.want_ls && p.wants_log), "dustbin terms only for the full log assignment");
            }
        }
        blk = -1;
        const AdaptMode m = plan.after_layer(layer);
        if (last) CHECK(m == AdaptMode::None, "no adaptive step behind the last layer");   // ref :544-545
        else if (rows_can_move) CHECK(m == (gather_on ? AdaptMode::PruneGather : AdaptMode::PruneInPlace), "a pruning step, gathering only on the product path");
        else CHECK(m == (p.depth ? AdaptMode::StopOnly : AdaptMode::None), "a stop step only with early stopping");
        CHECK(prunes(m) == plan.block(layer, 1).prune_here, "the tail ahead of a pruning step emits its mask scores");
        move_pending = m == AdaptMode::PruneGather;
    }
    layer = blk = -1;
    CHECK(!prev_tail_projected && !move_pending, "nothing is left pending behind the last block");
    CHECK(final_in_tail <= 1 && plan.final_proj_in_last_tail() == (final_in_tail == 1), "the final projection runs exactly once: in the last tail, or as its own launch");
    CHECK(plan.block(p.L - 1, 1).first_step + 5 == plan.last_step(), "the last block ends at the last step");
}

}  // namespace

int main() {
    const int shapes[5][2] = {{10, 20}, {64, 64}, {64, 65}, {200, 10}, {300, 333}};   // below, at and above pruning_min_kpts (one side, both sides)
    const uint32_t flag_sets[6] = {0, LG_FLAG_EXT, LG_FLAG_EXT | LG_FLAG_INDEXED, LG_FLAG_INDEXED, LG_FLAG_EXT | LG_FLAG_CHECK_FINITE, LG_FLAG_CHECK_FINITE};
    const int layers[3] = {1, 2, 9}, dims[2] = {128, 256}, stops[3] = {-1, 0, 7};
    Point p{};
    for (int L : layers) for (int depth = 0; depth < 2; ++depth) for (int width = 0; width < 3; ++width)   // width 2: on, suppressed by LG_FLAG_NO_PRUNING
    for (const auto& sh : shapes) for (int dim : dims) for (int fusion = 0; fusion < 16; ++fusion) for (int timing = 0; timing <= 6; ++timing)
    for (int stop : stops) for (int supports = 0; supports < 2; ++supports) for (uint32_t fl : flag_sets) for (int extra = 0; extra < 4; ++extra) {
        p.L = L; p.depth = depth != 0; p.width = width != 0; p.n0 = sh[0]; p.n1 = sh[1]; p.input_dim = dim;
        p.flags = fl | (width == 2 ? LG_FLAG_NO_PRUNING : 0u);
        p.opt = ForwardOptions{};
        p.opt.fused_tail = fusion & 1; p.opt.fused_next = (fusion >> 1) & 1; p.opt.fused_prep = (fusion >> 2) & 1; p.opt.adapt_gather = ((fusion >> 3) & 1) != 0;
        p.opt.tail_timing = timing; p.opt.debug_stop = stop;
        p.supports_next = supports != 0; p.counts = (extra & 1) != 0; p.wants_log = (extra & 2) != 0;
        check_point(p);
    }
    // the engine's defaults are the product configuration
    const ForwardOptions def{};
    if (!(def.fused_tail == 1 && def.fused_next == 1 && def.fused_prep == 1 && def.adapt_gather && def.sim_planes && def.sim_chunk == 0 && def.attn_dma && def.attn_rows == 32 &&
          def.attn_auto_rows && def.tail_row_tiles == 0 && def.tail_timing == 0 && def.debug_stop == -1)) { std::printf("FAILED: option defaults\n"); return 1; }
    // similarity on planes / split q, k, v: by precision
    for (int prec : {LG_PREC_F32, LG_PREC_BF16, LG_PREC_F16, LG_PREC_F16X3}) for (int ap : {prec, (int)LG_PREC_F16}) for (int planes = 0; planes < 2; ++planes) {
        lg_config cfg{}; cfg.input_dim = 256; cfg.n_layers = 9; cfg.precision = prec; cfg.pruning_min_kpts = kMinKpts;
        ForwardOptions o{}; o.sim_planes = planes != 0;
        const ForwardPlan plan = plan_forward(cfg, ap, o, 100, 100, 0, false, false, true);
        if (plan.sim_planes != (prec == LG_PREC_F16X3 && planes) || plan.split_qkv != (ap == LG_PREC_F16X3)) { std::printf("FAILED: sim_planes / split_qkv at precision %d / %d\n", prec, ap); return 1; }
    }
    // ---- the storage format of a side (side_format), at all 64 combinations of the six storage flags, with and without LG_FLAG_EXT.  The rule, restated from
    // include/lightglue_amd.h: a side's rows are uint8 with its _U8 flag, binary16 with its _F16 flag, fp32 with neither; both at once is no format;
    // RootSIFT applies to any of them; and without LG_FLAG_EXT none of the flags may be set (nothing is on, and a set flag is a refusal).
    const uint32_t f16[2] = {LG_FLAG_DESC0_F16, LG_FLAG_DESC1_F16}, u8[2] = {LG_FLAG_DESC0_U8, LG_FLAG_DESC1_U8}, root[2] = {LG_FLAG_ROOTSIFT0, LG_FLAG_ROOTSIFT1};
    for (int combo = 0; combo < 64; ++combo) for (int ext = 0; ext < 2; ++ext) for (int other = 0; other < 2; ++other) {
        uint32_t fl = (ext ? LG_FLAG_EXT : 0u) | (other ? LG_FLAG_INDEXED | LG_FLAG_NO_PRUNING | LG_FLAG_CHECK_FINITE : 0u);
        bool any_sift = false;
        for (int side = 0; side < 2; ++side) {
            if (combo >> (3 * side) & 1) fl |= f16[side];
            if (combo >> (3 * side + 1) & 1) { fl |= u8[side]; any_sift = true; }
            if (combo >> (3 * side + 2) & 1) { fl |= root[side]; any_sift = true; }
        }
        for (int side = 0; side < 2; ++side) {
            const bool h = (fl & f16[side]) != 0, b = (fl & u8[side]) != 0, r = (fl & root[side]) != 0;
            const SideFormat f = side_format(fl, side);
            const int kind = !ext ? DESC_F32 : b ? DESC_U8 : h ? DESC_F16 : DESC_F32;
            const bool valid = ext ? !(h && b) : !(h || b || r);
            if (f.valid != valid || (valid && (f.kind != kind || f.rootsift != (ext && r))) || (!ext && (f.kind != DESC_F32 || f.rootsift))) {
                std::printf("FAILED: side_format(flags %u, side %d) = {kind %d, rootsift %d, valid %d}\n", fl, side, f.kind, f.rootsift, f.valid); return 1;
            }
        }
        // a SIFT store is read by the preparation kernel alone: the fused preparation is off exactly when one of its flags is set (with LG_FLAG_EXT)
        lg_config cfg{}; cfg.input_dim = 256; cfg.n_layers = 9; cfg.precision = LG_PREC_F16X3; cfg.pruning_min_kpts = kMinKpts;
        const ForwardPlan plan = plan_forward(cfg, LG_PREC_F16X3, ForwardOptions{}, 100, 100, fl, false, false, true);
        if (plan.fuse_prep != !(ext && any_sift)) { std::printf("FAILED: fuse_prep %d at flags %u\n", plan.fuse_prep, fl); return 1; }
        ++g_points;
    }
    std::printf("ok %lld\n", g_points);
    return 0;
}
