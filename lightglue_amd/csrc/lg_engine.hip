// lightglue_amd — engine: workspace, forward orchestration and the engine's part of the C ABI (include/lightglue_amd.h).
// Replaces LightGlue._forward (ref lightglue.py:483-629) for the hot path; the weights are lg_weights.hip.
#include <cmath>
#include <cstring>
#include <string>

#include "lg_engine.h"

using namespace lg;

namespace {

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
// bytes per element of the q / k / v^T buffers: the split attention keeps an f16 hi and an f16 lo plane
size_t attn_elem_bytes(int attn_prec) { return attn_prec == PREC_F32 ? 4 : attn_prec == PREC_F16X3 ? 4 : 2; }
// compaction chunk flags (lg_adaptive.hip): chunks per segment, and the bytes of [2B][chunks] ints + the error word and the work-item ticket behind them
int compact_chunks(int c0, int c1) { return (c0 > c1 ? c0 : c1) / compact_chunk_rows(); }
size_t cflags_bytes(int B, int c0, int c1) { return (size_t)2 * B * compact_chunks(c0, c1) * 4 + 256; }

}  // namespace

namespace lg {

// The workspace for B pairs of c0 + c1 rows (multiples of 128), described once: measured with base == nullptr, carved into the engine's members and
// `bufs` (lg_engine_debug_read) otherwise (see Arena).  Buffers are laid out densely for the shape given.  Every size below is non-decreasing in each
// of B, c0 and c1, and so is every (256-byte aligned) offset: the bytes measured at the capacity shape hold the carve of any shape inside it.
size_t workspace_layout(lg_engine* e, char* base, int B, int c0, int c1) {
    const size_t R = (size_t)B * (c0 + c1), as = attn_elem_bytes(e->attn_prec);
    const size_t per0 = (size_t)B * c0 * 4, per1 = (size_t)B * c1 * 4, tiles = (size_t)B * (c0 / 32) * c1 * 4;   // one word per image-0 row / image-1 row / (32-row tile, column)
    Arena ar{base};
    if (base) e->bufs.clear();
    auto take = [&](const char* name, auto*& member, size_t bytes) { ar.take(member, bytes); if (base) e->bufs[name] = {member, bytes}; };
    take("X", e->X, R * 256 * 4); take("CTX", e->CTX, R * 256 * 4); take("MSG", e->MSG, R * 256 * 4);
    take("H1", e->H1, R * 512 * 4); take("G", e->G, R * 512 * 4);
    take("COS", e->COS, R * 32 * 4); take("SIN", e->SIN, R * 32 * 4);
    take("MD", e->MD, R * 256 * 4);
    take("SIM", e->SIM, (size_t)B * c0 * c1 * 4);
    take("LS", e->LS, R * 4); take("LSNEG", e->LSNEG, R * 4); take("CONF", e->CONF, R * 4); take("MSCORE", e->MSCORE, R * 4);
    take("LSE_R", e->LSE_R, per0); take("LSE_C", e->LSE_C, per1);
    take("MAX0", e->MAX0, per0); take("MAX1", e->MAX1, per1);
    take("ARG0", e->ARG0, per0); take("ARG1", e->ARG1, per1);
    take("CPM", e->CPM, tiles); take("CPS", e->CPS, tiles); take("CBV", e->CBV, tiles); take("CBI", e->CBI, tiles);
    take("BBOX", e->BBOX, (size_t)B * 8 * 4);
    take("XIN", e->XIN, R * (size_t)e->cfg.input_dim * 4);
    take("Q", e->Q, R * 256 * as); take("K", e->K, R * 256 * as); take("VT", e->VT, R * 256 * as);
    take("IND", e->IND, R * 4); take("DST", e->DST, R * 4);
    take("LEN", e->LEN, (size_t)B * 2 * 4); take("LEN_ORIG", e->LEN_ORIG, (size_t)B * 2 * 4); take("LEN_OLD", e->LEN_OLD, (size_t)B * 2 * 4);
    take("ACTIVE", e->ACTIVE, (size_t)B * 4); take("FINAL_LAYER", e->FINAL_LAYER, (size_t)B * 4);
    take("RANGEF", e->RANGEF, (size_t)B * 4);
    take("XSEL", e->XSEL, (size_t)B * 4);
    take("X2", e->X2, R * 256 * 4); take("COS2", e->COS2, R * 32 * 4); take("SIN2", e->SIN2, R * 32 * 4);   // gather path
    take("CFLAGS", e->CFLAGS, cflags_bytes(B, c0, c1));
    // 16 bytes per row: [R / 64 workgroups][8 waves][8 stamps], or [R / 128][16 half-waves ...] of the split attention's taps
    take("TAILDBG", e->TAILDBG, R * 16); take("TAILDBG2", e->TAILDBG2, R * 16);
    return ar.used;
}

}  // namespace lg

static int ensure_workspace(lg_engine* e, int B, int n0, int n1) {
    const int c0 = round_up(n0 > 0 ? n0 : 1, 128), c1 = round_up(n1 > 0 ? n1 : 1, 128);
    const bool fits = e->ws && B <= e->capB && c0 <= e->cap0 && c1 <= e->cap1;
    if (!fits) {
        if (e->ws) { HIPCHK(hipDeviceSynchronize()); HIPCHK(hipFree(e->ws)); e->ws = nullptr; }
        e->capB = B > e->capB ? B : e->capB; e->cap0 = c0 > e->cap0 ? c0 : e->cap0; e->cap1 = c1 > e->cap1 ? c1 : e->cap1;
        e->ws_bytes = workspace_layout(e, nullptr, e->capB, e->cap0, e->cap1);
        HIPCHK(hipMalloc(&e->ws, e->ws_bytes));
    }
    // carve for the CURRENT (B, c0, c1)
    if (fits && e->curB == B && e->cur_cap0 == c0 && e->cur_cap1 == c1 && !e->bufs.empty()) return LG_OK;
    e->curB = B; e->cur_cap0 = c0; e->cur_cap1 = c1;
    e->cflags_clean = false;
    if (workspace_layout(e, static_cast<char*>(e->ws), B, c0, c1) > e->ws_bytes) return set_error(LG_ERR_STATE, "workspace carve overflow");
    return LG_OK;
}

extern "C" {

int lg_engine_create(const lg_config* cfg, lg_engine** out) {
    if (!cfg || !out) return set_error(LG_ERR_INVALID, "null argument");
    if (cfg->descriptor_dim != 256 || cfg->num_heads != 4) return set_error(LG_ERR_INVALID, "only descriptor_dim=256, num_heads=4 (head_dim 64) are built");
    if (cfg->n_layers < 1 || cfg->n_layers > 64) return set_error(LG_ERR_INVALID, "bad n_layers");
    if (cfg->input_dim <= 0 || cfg->input_dim % 64) return set_error(LG_ERR_INVALID, "input_dim must be a positive multiple of 64");
    if (cfg->precision != LG_PREC_F32 && cfg->precision != LG_PREC_BF16 && cfg->precision != LG_PREC_F16 && cfg->precision != LG_PREC_F16X3) return set_error(LG_ERR_INVALID, "bad precision");
    auto* e = new lg_engine();
    e->cfg = *cfg;
    int ap = cfg->attn_precision;
    if (ap < 0) ap = cfg->precision;   // f16x3 -> split attention; every other precision -> its own element type
    // pairs with a q/k/v projection kernel (lg_proj.hip): a precision with itself, or f16x3 with one f16 plane (the fast opt-in)
    if (!(ap == cfg->precision || (cfg->precision == PREC_F16X3 && ap == PREC_F16))) { delete e; return set_error(LG_ERR_INVALID, "bad attn_precision: must equal `precision`, or LG_PREC_F16 with LG_PREC_F16X3"); }
    e->attn_prec = ap;
    *out = e;
    return LG_OK;
}

void lg_engine_destroy(lg_engine* e) {
    if (!e) return;
    for (auto& sp : e->prof_pool) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
    if (e->ws) (void)hipFree(e->ws);
    if (e->w_arena) (void)hipFree(e->w_arena);
    delete e;
}

// The envelope of include/lightglue_amd.h (LG_MAX_*): inside it every byte / element offset fits the type it is computed in (the raw-buffer
// descriptors and 32-bit offsets of the compaction, lg_adaptive.hip, reach 4 GB; X is B * (cap0 + cap1) KB) — outside it the hardware would DROP
// stores without an error, so the call is refused instead.
static int check_envelope(long long B, long long n0, long long n1) {
    const long long c0 = (n0 + 127) / 128 * 128, c1 = (n1 + 127) / 128 * 128;
    if (n0 > LG_MAX_KEYPOINTS || n1 > LG_MAX_KEYPOINTS)
        return set_error(LG_ERR_INVALID, "more than LG_MAX_KEYPOINTS (8192) keypoints in one image");
    if (B * (c0 + c1) > LG_MAX_ROWS)
        return set_error(LG_ERR_INVALID, "batch * (cap0 + cap1) exceeds LG_MAX_ROWS (2^21 keypoint rows per forward): split the batch across calls");
    if (B * c0 * c1 > LG_MAX_SIM_ELEMS)
        return set_error(LG_ERR_INVALID, "batch * cap0 * cap1 exceeds LG_MAX_SIM_ELEMS (2^31 - 1 similarity entries per forward): split the batch across calls");
    return LG_OK;
}

int lg_engine_reserve(lg_engine* e, int32_t max_batch, int32_t max_n0, int32_t max_n1) {
    if (!e || max_batch < 1 || max_n0 < 0 || max_n1 < 0) return set_error(LG_ERR_INVALID, "bad argument");
    TRY(check_envelope(max_batch, max_n0, max_n1));
    return ensure_workspace(e, max_batch, max_n0, max_n1);
}

int lg_engine_set_option(lg_engine* e, const char* key, int32_t value) {
    if (!e || !key) return set_error(LG_ERR_INVALID, "null argument");
    if (std::strcmp(key, "fused_tail") == 0) { e->opt.fused_tail = value != 0; return LG_OK; }
    if (std::strcmp(key, "fused_next") == 0) { e->opt.fused_next = value != 0; return LG_OK; }
    if (std::strcmp(key, "fused_prep") == 0) { e->opt.fused_prep = value != 0; return LG_OK; }
    if (std::strcmp(key, "attn_dma") == 0) { e->opt.attn_dma = value != 0; return LG_OK; }
    if (std::strcmp(key, "adapt_gather") == 0) { e->opt.adapt_gather = value != 0; return LG_OK; }
    if (std::strcmp(key, "sim_planes") == 0) { e->opt.sim_planes = value != 0; return LG_OK; }
    if (std::strcmp(key, "sim_chunk") == 0) { if (value < 0 || value % 64) return set_error(LG_ERR_INVALID, "sim_chunk: 0 or a multiple of 64"); e->opt.sim_chunk = value; return LG_OK; }
    if (std::strcmp(key, "attn_rows") == 0) { if (value != 16 && value != 32 && value != 64) return set_error(LG_ERR_INVALID, "attn_rows must be 16, 32 or 64"); e->opt.attn_rows = value; e->opt.attn_auto_rows = false; return LG_OK; }
    if (std::strcmp(key, "tail_row_tiles") == 0) { if (value != 0 && value != 1 && value != 2 && value != 4) return set_error(LG_ERR_INVALID, "tail_row_tiles must be 0 (automatic), 1, 2 or 4"); e->opt.tail_row_tiles = value; return LG_OK; }
    if (std::strcmp(key, "profile_only") == 0) { e->prof_only = value; return LG_OK; }   // kernel class index, -1 = all classes
    if (std::strcmp(key, "tail_timing") == 0) { e->opt.tail_timing = value; return LG_OK; }   // which kernel leaves shader-clock stamps: ForwardOptions::tail_timing
    return set_error(LG_ERR_INVALID, std::string("unknown option '") + key + "'");
}

namespace {
// Fused tail: 16-row tiles per workgroup by grid fill.  A 64-row workgroup costs ~114k cycles (matrix-bound), a 32- / 16-row
// one ~69k / ~58k (each streams the full weight set from L2): with R rows on 256 CUs take the shape with the shortest
// critical path — 64 rows as soon as they fill the chip, smaller tiles for single pairs (B = 1, N = 1024: 32 -> 128 workgroups).
int tail_row_tiles_for(int R) {
    int best = 4; long long best_cost = -1;
    const int shapes[3] = {4, 2, 1}; const long long cost[3] = {114, 69, 58};   // measured: 56 / 34 / 28.6 us per launch at B = 1, N = 1024
    for (int i = 0; i < 3; ++i) {
        const long long wgs = R / (16 * shapes[i]), rounds = (wgs + 255) / 256, c = rounds * cost[i];
        if (best_cost < 0 || c < best_cost) { best = shapes[i]; best_cost = c; }
    }
    return best;
}

PairIndex pair_index(const lg_forward_io* io) { return indexed(io->flags) ? PairIndex{io->index0, io->index1, io->images0, io->images1} : PairIndex{}; }

int check_forward_io(const lg_engine* e, const lg_forward_io* io) {
    if (!e || !io) return set_error(LG_ERR_INVALID, "null argument");
    for (int side = 0; side < 2; ++side) {   // each side's storage format (side_format): pure argument checks, ahead of the engine's state: refused on any engine
        const SideFormat f = side_format(io->flags, side);
        if (!f.valid) return set_error(LG_ERR_INVALID, (io->flags & LG_FLAG_EXT) ? "LG_FLAG_DESC*_U8 and LG_FLAG_DESC*_F16 are both set on one side: a store has one format"
                                                                                 : "LG_FLAG_DESC*_F16 / LG_FLAG_DESC*_U8 / LG_FLAG_ROOTSIFT* need LG_FLAG_EXT");
        // binary16 rows are read in 16-byte pieces and are input_dim * 2 bytes long (a multiple of 128), so the base decides; uint8 rows are read in 4-byte
        // pieces and held to the same 16 bytes
        if (f.kind != DESC_F32 && (reinterpret_cast<uintptr_t>(side ? io->desc1 : io->desc0) & 15))
            return set_error(LG_ERR_INVALID, "LG_FLAG_DESC*_F16 / LG_FLAG_DESC*_U8: the descriptor pointer must be 16-byte aligned");
        if ((f.kind == DESC_U8 || f.rootsift) && e->cfg.input_dim % 4) return set_error(LG_ERR_INVALID, "LG_FLAG_DESC*_U8 / LG_FLAG_ROOTSIFT*: input_dim must be a multiple of 4");
        if (f.rootsift && e->cfg.input_dim > 256) return set_error(LG_ERR_INVALID, "LG_FLAG_ROOTSIFT0 / _ROOTSIFT1: input_dim must be at most 256 (one wave holds the row)");
    }
    const bool ext = (io->flags & LG_FLAG_EXT) != 0;            // round-5 extension fields present
    if (io->flags & LG_FLAG_INDEXED) {                          // the pair list: a pure argument check too
        if (!ext || !io->status) return set_error(LG_ERR_INVALID, "lg_engine_forward: LG_FLAG_INDEXED needs LG_FLAG_EXT and a status array");
        TRY(check_pair_list("lg_engine_forward", io->flags, io->index0, io->index1, io->images0, io->images1));
    }
    if (!e->weights_ready) return set_error(LG_ERR_STATE, "weights not finalised");
    const int B = io->batch, n0 = io->n0, n1 = io->n1;
    if (B < 1 || n0 < 0 || n1 < 0) return set_error(LG_ERR_INVALID, "bad batch / keypoint counts");
    TRY(check_envelope(B, n0, n1));
    if (!io->stop || !io->n_matches) return set_error(LG_ERR_INVALID, "null output pointer");
    if ((n0 && (!io->matches0 || !io->scores0)) || (n1 && (!io->matches1 || !io->scores1))) return set_error(LG_ERR_INVALID, "null output pointer");
    if (n0 && n1 && (!io->matches || !io->match_scores)) return set_error(LG_ERR_INVALID, "null match-list pointer");
    if (n0 && n1 && (!io->kpts0 || !io->kpts1 || !io->desc0 || !io->desc1)) return set_error(LG_ERR_INVALID, "null input pointer");
    const bool do_prune = pruning_on(e->cfg, io->flags);
    if (do_prune && ((n0 && !io->prune0) || (n1 && !io->prune1))) return set_error(LG_ERR_INVALID, "prune0/prune1 required when width_confidence > 0");
    if (e->cfg.add_scale_ori && (!io->scales0 || !io->oris0 || !io->scales1 || !io->oris1)) return set_error(LG_ERR_INVALID, "scales/oris required");
    if ((io->flags & LG_FLAG_CHECK_FINITE) && (!ext || !io->status)) return set_error(LG_ERR_INVALID, "LG_FLAG_CHECK_FINITE needs LG_FLAG_EXT and a status array");
    if (ext && io->wire && io->wire_stride < LG_WIRE_WIDTH(n0, n1)) return set_error(LG_ERR_INVALID, "wire_stride < LG_WIRE_WIDTH(n0, n1) = 3 n0 + 3 n1 + 2");
    if (ext && do_prune && ((io->prune0_f32 || io->prune1_f32))) return set_error(LG_ERR_INVALID, "prune0_f32 / prune1_f32 are the outputs of a forward WITHOUT pruning");
    if (ext && !do_prune && ((io->prune0_i64 || io->prune1_i64))) return set_error(LG_ERR_INVALID, "prune0_i64 / prune1_i64 are the outputs of a forward WITH pruning");
    return LG_OK;
}

// the last launch of a forward (lg_outputs.hip): final_layer == nullptr -> every pair's stop is stop_const
hipError_t write_outputs(const lg_engine* e, const lg_forward_io* io, const int* final_layer, int stop_const, const int* range_flag, const int* device_err, hipStream_t s) {
    OutArgs o{};
    o.B = io->batch; o.n0 = io->n0; o.n1 = io->n1; o.L = e->cfg.n_layers; o.kmax = io->n0 < io->n1 ? io->n0 : io->n1;
    o.final_layer = final_layer; o.stop_const = stop_const; o.stop = io->stop;
    o.m0 = io->matches0; o.m1 = io->matches1; o.s0 = io->scores0; o.s1 = io->scores1; o.matches = io->matches; o.n_matches = io->n_matches;
    o.prune0 = io->prune0; o.prune1 = io->prune1; o.num0 = io->num0; o.num1 = io->num1;
    if (io->flags & LG_FLAG_EXT) {
        o.m0_64 = (long long*)io->matches0_i64; o.m1_64 = (long long*)io->matches1_i64; o.matches_64 = (long long*)io->matches_i64; o.stop_64 = (long long*)io->stop_i64;
        o.prune0_64 = (long long*)io->prune0_i64; o.prune1_64 = (long long*)io->prune1_i64; o.prune0_f = io->prune0_f32; o.prune1_f = io->prune1_f32;
        o.wire = io->wire; o.wire_stride = io->wire_stride; o.wire_prune = pruning_on(e->cfg, io->flags) ? 1 : 0; o.status = io->status; o.range_flag = range_flag; o.device_err = device_err;
        o.px = pair_index(io);
    }
    return launch_write_outputs(o, s);
}

// an image without keypoints (ref :539-540, :568-588): the well-formed empty result, stop = 1
int forward_empty(const lg_engine* e, const lg_forward_io* io, hipStream_t s) {
    const int B = io->batch, n0 = io->n0, n1 = io->n1;
    if (n0) { HIPCHK(hipMemsetAsync(io->matches0, 0xFF, sizeof(int) * (size_t)B * n0, s)); HIPCHK(hipMemsetAsync(io->scores0, 0, 4 * (size_t)B * n0, s)); }
    if (n1) { HIPCHK(hipMemsetAsync(io->matches1, 0xFF, sizeof(int) * (size_t)B * n1, s)); HIPCHK(hipMemsetAsync(io->scores1, 0, 4 * (size_t)B * n1, s)); }
    HIPCHK(hipMemsetAsync(io->n_matches, 0, sizeof(int) * (size_t)B, s));
    InitStateArgs is{};   // the prune counters alone
    is.B = B; is.n0 = n0; is.n1 = n1; is.L = e->cfg.n_layers; is.px = pair_index(io);
    if (pruning_on(e->cfg, io->flags)) { is.prune0 = n0 ? io->prune0 : nullptr; is.prune1 = n1 ? io->prune1 : nullptr; }
    HIPCHK(launch_init_state(is, s));
    HIPCHK(write_outputs(e, io, nullptr, 1, nullptr, nullptr, s));   // stop = 1 for every pair (+ the extension outputs of an empty result)
    return LG_OK;
}

// ---- one forward: lg_engine_forward plans it (plan_forward, lg_forward_plan.h) and runs the plan in three stages — forward_prepare, forward_layers,
// forward_assign.  The stages read the plan and decide nothing; what they share is the ForwardCtx.

struct ForwardCtx {
    hipStream_t s;
    RowSpace rs_all, rs_act;   // every pair / the pairs still active
    int R;                     // rows of the carved workspace: B * (cap0 + cap1)
    int* range_flag;           // LG_FLAG_CHECK_FINITE: RANGEF, else nullptr
    int* device_err;           // error word + compaction ticket behind the chunk flags (lg_adaptive.hip)
    PrepArgs prep;             // the per-keypoint preparation: its own launch (forward_prepare), or inside the first projection launch (forward_layers)
};

#define PROFILED(cls, launch) do { TRY(prof_begin(e, cls, c.s)); HIPCHK(launch); TRY(prof_end(e, c.s)); } while (0)   // one launch inside its profile bracket

ForwardCtx forward_ctx(const lg_engine* e, const lg_forward_io* io, const ForwardPlan& plan, hipStream_t s) {
    const int B = io->batch, c0 = e->cur_cap0, c1 = e->cur_cap1;
    ForwardCtx c{};
    c.s = s; c.rs_all = RowSpace{B, c0, c1, e->LEN, nullptr}; c.rs_act = RowSpace{B, c0, c1, e->LEN, e->ACTIVE}; c.R = B * (c0 + c1);
    c.range_flag = plan.check_finite ? e->RANGEF : nullptr;
    c.device_err = e->CFLAGS + (size_t)2 * B * compact_chunks(c0, c1);
    PrepArgs& p = c.prep;
    p.rs = c.rs_all; p.px = pair_index(io);
    p.side[0] = PrepSide{io->kpts0, io->size0, io->scales0, io->oris0, io->desc0, io->n0};
    p.side[1] = PrepSide{io->kpts1, io->size1, io->scales1, io->oris1, io->desc1, io->n1};
    for (int side = 0; side < 2; ++side) { const SideFormat f = side_format(io->flags, side); p.side[side].kind = f.kind; p.side[side].rootsift = f.rootsift; }
    p.Wr = e->Wr; p.pos_dim = 2 + 2 * (e->cfg.add_scale_ori ? 1 : 0); p.input_dim = e->cfg.input_dim;
    p.X = e->X; p.Xin = e->XIN; p.cosb = e->COS; p.sinb = e->SIN; p.ind = e->IND; p.bbox = e->BBOX;
    return c;
}

// a set of residual / rotary buffers (BlockPlan::buf_set): 0 = X / COS / SIN, 1 = X2 / COS2 / SIN2
struct BufSet { float *X, *cosb, *sinb; };
BufSet buf_set(const lg_engine* e, int set) { return set ? BufSet{e->X2, e->COS2, e->SIN2} : BufSet{e->X, e->COS, e->SIN}; }

// per-op GEMM out[R][Nout] = [A | A2] W^T + bias on the weights `w_elems` elements into the layer-major matrix W
GemmArgs gemm_args(const lg_engine* e, const ForwardCtx& c, const RowSpace& rs, const float* A, int lda, const float* A2, int lda2, int K1, int K,
                   const PackedW& W, size_t w_elems, const float* bias, int Nout, float* out) {
    const int prec = e->cfg.precision;
    GemmArgs g{};
    g.rs = rs; g.A = A; g.lda = lda; g.A2 = A2; g.lda2 = lda2; g.K1 = K1; g.K = K; g.bias = bias; g.Nout = Nout; g.out = out; g.ldo = Nout; g.out_scale = 1.f; g.R = c.R;
    g.W = static_cast<char*>(W.hi) + w_elems * elem_size(prec); g.Wlo = W.lo ? static_cast<char*>(W.lo) + w_elems * elem_size(prec) : nullptr;
    return g;
}

// q/k/v projection of block `blk` of `layer` on the rows of buffer set `set` (lg_proj.hip / fused into lg_tail.hip)
ProjArgs proj_args(const lg_engine* e, const ForwardPlan& plan, const ForwardCtx& c, int layer, int blk, int set) {
    const BufSet x = buf_set(e, set);
    ProjArgs pj{};
    pj.rs = c.rs_act; pj.X = x.X; pj.R = c.R; pj.q = e->Q; pj.k = e->K; pj.vt = e->VT; pj.plane = plan.split_qkv ? (long long)c.R * 256 : 0;
    const BlockWeights& bw = e->blocks[blk];
    pj.W = bw.qkv_p + (size_t)layer * bw.qkv_layer_bytes; pj.bias = bw.b_qkv + (size_t)layer * bw.Nout;
    pj.Nout = bw.Nout; pj.n_qk_groups = bw.n_qk_groups;
    if (blk == 0) { pj.cosb = x.cosb; pj.sinb = x.sinb; }   // rotary on q, k of the SelfBlock only
    pj.dbg = nullptr; pj.range_flag = c.range_flag;
    return pj;
}

// final projection (ref :289-291: / d**0.25), lg_proj.hip / fused into the last tail: of the active pairs at the last layer, or — per_pair — of every
// pair with the weights of the layer it stopped at
FinalArgs final_args(const lg_engine* e, const ForwardPlan& plan, const ForwardCtx& c, bool per_pair) {
    const int layer = e->cfg.n_layers - 1;
    FinalArgs f{};
    f.rs = per_pair ? c.rs_all : c.rs_act; f.X = per_pair ? e->X : buf_set(e, plan.block(layer, 1).buf_set).X; f.R = c.R; f.out = e->MD; f.scale = 0.25f;
    f.planes = plan.sim_planes ? 1 : 0;
    if (per_pair) { f.X2 = e->X2; f.xsel = e->XSEL; }    // XSEL stays 0 unless a gather projection ran
    f.W = e->w_final_p + (per_pair ? 0 : (size_t)layer * e->final_layer_bytes); f.bias = e->b_final + (per_pair ? 0 : (size_t)layer * 256);
    f.layer_of_pair = per_pair ? e->FINAL_LAYER : nullptr; f.w_layer_bytes = (long long)e->final_layer_bytes;
    return f;
}

// init_state, prep (or its bounding-box part when the first projection does the rest), input_proj (ref :521-522): debug step 0
int forward_prepare(lg_engine* e, const lg_forward_io* io, const ForwardPlan& plan, const ForwardCtx& c, bool& stopped) {
    const InitStateArgs is{io->batch, io->n0, io->n1, plan.n_layers, io->num0, io->num1, e->LEN, e->LEN_ORIG, e->LEN_OLD, e->ACTIVE, e->FINAL_LAYER,
                           plan.do_prune ? io->prune0 : nullptr, plan.do_prune ? io->prune1 : nullptr, e->RANGEF, c.device_err, e->XSEL, pair_index(io)};
    HIPCHK(launch_init_state(is, c.s));
    TRY(prof_begin(e, PC_PREP, c.s));
    if (plan.fuse_prep) HIPCHK(launch_prep_bbox(c.prep, c.s)); else HIPCHK(launch_prep(c.prep, c.s));
    const int in = e->cfg.input_dim;
    if (in != 256) {
        GemmArgs g = gemm_args(e, c, c.rs_all, e->XIN, in, nullptr, 0, in, in, e->w_in, 0, e->b_in, 256, e->X);
        HIPCHK(launch_gemm(e->cfg.precision, EPI_STORE, g, c.s));
    }
    TRY(prof_end(e, c.s));
    stopped = plan.stops_at(0);
    return LG_OK;
}

// the q/k/v of a block that the previous tail has not produced: one launch in the block's profile class
int launch_block_proj(lg_engine* e, const ForwardPlan& plan, const ForwardCtx& c, int layer, int blk, const BlockPlan& b) {
    const int prec = e->cfg.precision, ap = e->attn_prec;
    ProjArgs pj = proj_args(e, plan, c, layer, blk, b.proj_by == ProjBy::OwnGather ? b.buf_set ^ 1 : b.buf_set);
    pj.dbg = (e->opt.tail_timing == 2 && blk == 0) ? e->TAILDBG : nullptr;
    TRY(prof_begin(e, blk == 0 ? PC_GEMM_QKV_SELF : PC_GEMM_QKV_CROSS, c.s));
    if (b.proj_by == ProjBy::OwnFirst) {
        pj.rs = c.rs_all;                                 // rs_all: what prep covers (pairs with an empty image too)
        if (launch_proj_first(prec, ap, pj, c.prep, c.s) != hipSuccess) {
            //  e.g. the 80 KB of dynamic LDS refused: the separate preparation kernel + the standard projection instead — bit-identical
            (void)hipGetLastError();
            HIPCHK(launch_prep(c.prep, c.s));
            pj.rs = c.rs_act;
            HIPCHK(launch_proj(prec, ap, pj, c.s));
        }
    }
    else if (b.proj_by == ProjBy::OwnGather) {
        // the rows of every pair that prunes move to the other buffer set on their way into the projection; pairs that do not prune at this
        // layer are copied as they are (identity map): one buffer set is current for the whole batch
        const BufSet from = buf_set(e, b.buf_set ^ 1), to = buf_set(e, b.buf_set);
        GatherArgs ga{};
        ga.Xold = from.X; ga.cos_old = from.cosb; ga.sin_old = from.sinb; ga.Xnew = to.X; ga.cos_new = to.cosb; ga.sin_new = to.sinb;
        ga.src = e->DST; ga.len_old = e->LEN_OLD;
        HIPCHK(launch_proj_gather(prec, ap, pj, ga, c.s));
    }
    else HIPCHK(launch_proj(prec, ap, pj, c.s));
    TRY(prof_end(e, c.s));
    return LG_OK;
}

// out_proj + ffn.0 + LayerNorm + GELU + ffn.3 + residual of a block in one kernel (lg_tail.hip), with what the plan appends to it
int launch_block_tail(lg_engine* e, const ForwardPlan& plan, const ForwardCtx& c, int i, int blk, const BlockPlan& b) {
    const BlockWeights& bw = e->blocks[blk];
    const int D = 256, timing = e->opt.tail_timing;
    TailArgs ta{};
    ta.rs = c.rs_act; ta.X = buf_set(e, b.buf_set).X; ta.CTX = e->CTX; ta.range_flag = c.range_flag;
    ta.Wcat = bw.tail_cat + (size_t)i * e->tail_cat_layer_bytes; ta.bcat = bw.b_cat + (size_t)i * 512;
    ta.gamma = bw.ln_g + (size_t)i * 512; ta.beta = bw.ln_b + (size_t)i * 512;
    ta.W2 = bw.tail_2 + (size_t)i * e->tail_2_layer_bytes; ta.b2 = bw.b_f2 + (size_t)i * D;
    // the 256 -> 1 heads of a CrossBlock tail (BlockPlan): token confidence in head 0 when wanted, matchability in the first free head
    if (b.want_tok) { ta.head_w0 = e->w_tok + (size_t)i * D; ta.head_b0 = e->b_tok + i; ta.head_out0 = e->CONF; }
    if (b.prune_here || b.want_ls) {
        float* sig = b.prune_here ? e->MSCORE : nullptr; float* ls = b.want_ls ? e->LS : nullptr;
        float* lsneg = b.want_lsneg ? e->LSNEG : nullptr;
        if (b.want_tok) { ta.head_w1 = e->w_match + (size_t)i * D; ta.head_b1 = e->b_match + i; ta.head_out1 = sig; ta.head_ls1 = ls; ta.head_lsneg1 = lsneg; }
        else { ta.head_w0 = e->w_match + (size_t)i * D; ta.head_b0 = e->b_match + i; ta.head_out0 = sig; ta.head_ls0 = ls; ta.head_lsneg0 = lsneg; }
    }
    ta.dbg = (timing == 1 || (i == 0 && ((timing == 5 && blk == 1) || (timing == 6 && blk == 0)))) ? e->TAILDBG : nullptr;
    ta.row_tiles = e->opt.tail_row_tiles ? e->opt.tail_row_tiles : tail_row_tiles_for(c.R);
    if (b.tail_next == TailNext::NextProj) {
        ta.next = proj_args(e, plan, c, i + blk, blk ^ 1, b.buf_set);   // this layer's CrossBlock, or the next layer's SelfBlock
        if (ta.dbg && timing >= 5) ta.next.dbg = e->TAILDBG2;
    } else if (b.tail_next == TailNext::FinalProj) ta.fin = final_args(e, plan, c, false);
    PROFILED(PC_TAIL, launch_tail(e->cfg.precision, e->attn_prec, ta, c.s));
    return LG_OK;
}

// the adaptive step behind layer `i` (ref :544-566, lg_adaptive.hip): early stop and / or point pruning, in place or leaving the row move to the next projection
int launch_adaptive_step(lg_engine* e, const lg_forward_io* io, const ForwardPlan& plan, const ForwardCtx& c, int i, AdaptMode mode) {
    const int B = io->batch, c0 = e->cur_cap0, c1 = e->cur_cap1, D = 256;
    const bool do_stop = plan.do_stop, prune_now = prunes(mode);
    if (!plan.fused_tail) {   // per-op path: the 256 -> 1 heads as their own pass (the fused CrossBlock tail computes them in its epilogue)
        RowDotArgs rd{};
        rd.rs = c.rs_act; rd.X = e->X;
        if (do_stop) { rd.w0 = e->w_tok + (size_t)i * D; rd.b0 = e->b_tok + i; rd.out0 = e->CONF; rd.act0 = 1; }
        if (do_stop && prune_now) { rd.w1 = e->w_match + (size_t)i * D; rd.b1 = e->b_match + i; rd.out1 = e->MSCORE; rd.act1 = 1; }
        else if (prune_now) { rd.w0 = e->w_match + (size_t)i * D; rd.b0 = e->b_match + i; rd.out0 = e->MSCORE; rd.act0 = 1; }
        PROFILED(PC_ROWDOT, launch_rowdot(rd, c.s));
    }
    AdaptArgs ad{};
    ad.rs = c.rs_act; ad.len = e->LEN; ad.active = e->ACTIVE; ad.len_old = e->LEN_OLD; ad.final_layer = e->FINAL_LAYER;
    ad.ind = e->IND; ad.dst = e->DST; ad.prune0 = io->prune0; ad.prune1 = io->prune1; ad.n0 = io->n0; ad.n1 = io->n1; ad.len_orig = e->LEN_ORIG;
    ad.conf = e->CONF; ad.mscore = e->MSCORE; ad.X = e->X; ad.cosb = e->COS; ad.sinb = e->SIN;
    if (mode == AdaptMode::PruneGather) { ad.gather = 1; ad.src = e->DST; ad.xsel = e->XSEL; ad.xnext = plan.block(i + 1, 0).buf_set; }
    ad.layer = i;
    // ref :631-634 threshold (float32 buffer), :656 and :640 compare in float32
    ad.conf_thr = (float)std::fmin(std::fmax(0.8 + 0.1 * std::exp(-4.0 * i / plan.n_layers), 0.0), 1.0);
    ad.depth_conf = (float)e->cfg.depth_confidence;
    ad.width_conf = (float)(1.0 - e->cfg.width_confidence);
    ad.pruning_min_kpts = e->cfg.pruning_min_kpts;
    ad.do_stop = do_stop; ad.do_prune = prune_now;
    ad.compact_chunks = compact_chunks(c0, c1); ad.compact_flags = e->CFLAGS; ad.compact_err = c.device_err; ad.compact_ticket = c.device_err + 1;
    if (prune_now && !e->cflags_clean) {   // fresh carve: whatever the arena held there must not look like an epoch
        HIPCHK(hipMemsetAsync(e->CFLAGS, 0, cflags_bytes(B, c0, c1), c.s));
        e->cflags_clean = true;
    }
    ad.compact_epoch = ++e->compact_epoch;
    PROFILED(PC_ADAPTIVE, launch_adapt(ad, c.s));
    return LG_OK;
}

// the transformer (ref :541-566): per layer a SelfBlock and a CrossBlock — projection, attention, tail — and the adaptive step behind every layer but the last
int forward_layers(lg_engine* e, const lg_forward_io* io, const ForwardPlan& plan, const ForwardCtx& c, bool& stopped) {
    const int prec = e->cfg.precision, D = 256;
    stopped = true;   // until the last block is through
    for (int i = 0; i < plan.n_layers; ++i) {
        for (int blk = 0; blk < 2; ++blk) {
            const BlockPlan b = plan.block(i, blk);
            const BlockWeights& bw = e->blocks[blk];
            int step = b.first_step;
            if (b.proj_by != ProjBy::PrevTail) TRY(launch_block_proj(e, plan, c, i, blk, b));
            if (plan.stops_at(step++)) return LG_OK;
            {
                AttnArgs at{};
                at.rs = c.rs_act; at.q = e->Q; at.k = e->K; at.vt = e->VT; at.plane = plan.split_qkv ? (long long)c.R * 256 : 0; at.ctx = e->CTX; at.R = c.R; at.cross = blk;
                at.dbg = (e->opt.tail_timing == 3 && blk == 0) ? e->TAILDBG : nullptr;
                at.rows_per_wave = (e->opt.attn_auto_rows && c.R / 128 * 4 < 256) ? 16 : e->opt.attn_rows; at.dma = e->opt.attn_dma ? 1 : 0;   // fewer 128-row workgroups than CUs: 64-row ones
                PROFILED(blk == 0 ? PC_ATTN_SELF : PC_ATTN_CROSS, launch_attention(e->attn_prec, at, c.s));
            }
            if (plan.stops_at(step++)) return LG_OK;
            if (plan.fused_tail) {
                TRY(launch_block_tail(e, plan, c, i, blk, b));
                if (plan.stops_at(step + 3)) return LG_OK;   // the fused tail completes the block's last four steps at once
                continue;
            }
            {
                GemmArgs g = gemm_args(e, c, c.rs_act, e->CTX, D, nullptr, 0, D, D, bw.out, (size_t)i * D * D, bw.b_out + (size_t)i * D, D, e->MSG);
                PROFILED(PC_GEMM_OUT, launch_gemm(prec, EPI_STORE, g, c.s));
            }
            if (plan.stops_at(step++)) return LG_OK;
            {
                GemmArgs g = gemm_args(e, c, c.rs_act, e->X, D, e->MSG, D, D, 512, bw.f1, (size_t)i * 512 * 512, bw.b_f1 + (size_t)i * 512, 512, e->H1);
                PROFILED(PC_GEMM_FFN1, launch_gemm(prec, EPI_STORE, g, c.s));
            }
            if (plan.stops_at(step++)) return LG_OK;
            {
                LnGeluArgs ln{c.rs_act, e->H1, e->G, bw.ln_g + (size_t)i * 512, bw.ln_b + (size_t)i * 512, c.R};
                PROFILED(PC_LN_GELU, launch_ln_gelu(ln, c.s));
            }
            if (plan.stops_at(step++)) return LG_OK;
            {
                GemmArgs g = gemm_args(e, c, c.rs_act, e->G, 512, nullptr, 0, 512, 512, bw.f2, (size_t)i * D * 512, bw.b_f2 + (size_t)i * D, D, e->X);
                PROFILED(PC_GEMM_FFN2, launch_gemm(prec, EPI_RESID, g, c.s));
            }
            if (plan.stops_at(step++)) return LG_OK;
        }
        const AdaptMode mode = plan.after_layer(i);
        if (mode != AdaptMode::None) TRY(launch_adaptive_step(e, io, plan, c, i, mode));
    }
    stopped = false;
    return LG_OK;
}

// log assignment with the weights of the layer each pair stopped at (ref :591): matchability terms, final projection, similarity, assignment, outputs
int forward_assign(lg_engine* e, const lg_forward_io* io, const ForwardPlan& plan, const ForwardCtx& c) {
    const int prec = e->cfg.precision, n0 = io->n0, n1 = io->n1, D = 256;
    if (!plan.fused_tail) {   // per-op path: matchability terms as their own pass (the fused CrossBlock tails emit them from their heads)
        RowDotArgs rd{};
        rd.rs = c.rs_all; rd.X = e->X; rd.w0 = e->w_match; rd.b0 = e->b_match; rd.out0 = e->LS; rd.act0 = 2;
        rd.layer_of_pair = e->FINAL_LAYER; rd.w_layer_stride = D; rd.ignore_active = 1;
        if (plan.wants_log_assignment) { rd.w1 = e->w_match; rd.b1 = e->b_match; rd.out1 = e->LSNEG; rd.act1 = 3; }  // dustbin terms
        PROFILED(PC_ROWDOT, launch_rowdot(rd, c.s));
    }
    if (!plan.final_proj_in_last_tail()) PROFILED(PC_GEMM_FINAL, launch_final_proj(prec, final_args(e, plan, c, true), c.s));
    TRY(prof_begin(e, PC_SIM, c.s));
    if (plan.sim_planes) {
        SimPlanesArgs sp{c.rs_all, reinterpret_cast<const f16_t*>(e->MD), (long long)c.R * 256, D, e->SIM, e->opt.sim_chunk};
        HIPCHK(launch_sim_planes(sp, c.s));
    } else {
        SimArgs sm{c.rs_all, e->MD, D, D, e->SIM};
        HIPCHK(launch_sim(prec, sm, c.s));
    }
    TRY(prof_end(e, c.s));
    AssignArgs as{};
    as.rs = c.rs_all; as.sim = e->SIM; as.ls = e->LS; as.lse_r = e->LSE_R; as.lse_c = e->LSE_C; as.max0 = e->MAX0; as.arg0 = e->ARG0;
    as.max1 = e->MAX1; as.arg1 = e->ARG1; as.cpm = e->CPM; as.cps = e->CPS; as.cbv = e->CBV; as.cbi = e->CBI; as.ind = e->IND; as.n0 = n0; as.n1 = n1; as.filter_threshold = (float)e->cfg.filter_threshold;
    as.m0 = io->matches0; as.m1 = io->matches1; as.s0 = io->scores0; as.s1 = io->scores1;
    as.matches = io->matches; as.mscores = io->match_scores; as.n_matches = io->n_matches; as.max_matches = n0 < n1 ? n0 : n1;
    as.log_assignment = io->log_assignment; as.lsneg = e->LSNEG;
    as.dbg = e->opt.tail_timing == 4 ? e->TAILDBG : nullptr;
    as.all_rows_live = plan.all_rows_live ? 1 : 0;
    PROFILED(PC_ASSIGN, launch_assign(as, c.s));
    HIPCHK(write_outputs(e, io, e->FINAL_LAYER, 0, c.range_flag, c.device_err, c.s));
    return LG_OK;
}
#undef PROFILED
}  // namespace

int lg_engine_forward(lg_engine* e, const lg_forward_io* io, void* hip_stream) {
    TRY(check_forward_io(e, io));
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (io->n0 == 0 || io->n1 == 0) return forward_empty(e, io, s);
    TRY(ensure_workspace(e, io->batch, io->n0, io->n1));
    const ForwardPlan plan = plan_forward(e->cfg, e->attn_prec, e->opt, io->n0, io->n1, io->flags, io->num0 || io->num1, io->log_assignment != nullptr,
                                          launch_tail_supports_next(e->cfg.precision, e->attn_prec));
    const ForwardCtx c = forward_ctx(e, io, plan, s);
    bool stopped = false;   // lg_engine_debug_stop_after: the step asked for is done
    TRY(forward_prepare(e, io, plan, c, stopped));
    if (stopped) return LG_OK;
    TRY(forward_layers(e, io, plan, c, stopped));
    if (stopped) return LG_OK;
    return forward_assign(e, io, plan, c);
}

}  // extern "C"
