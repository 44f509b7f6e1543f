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
    if (std::strcmp(key, "fused_tail") == 0) { e->fused_tail = value != 0; return LG_OK; }
    if (std::strcmp(key, "fused_next") == 0) { e->fused_next = value != 0; return LG_OK; }
    if (std::strcmp(key, "fused_prep") == 0) { e->fused_prep = value != 0; return LG_OK; }
    if (std::strcmp(key, "attn_dma") == 0) { e->attn_dma = value != 0; return LG_OK; }
    if (std::strcmp(key, "adapt_gather") == 0) { e->adapt_gather = value != 0; return LG_OK; }
    if (std::strcmp(key, "sim_planes") == 0) { e->sim_planes = value != 0; return LG_OK; }
    if (std::strcmp(key, "sim_chunk") == 0) { if (value < 0 || value % 64) return set_error(LG_ERR_INVALID, "sim_chunk: 0 or a multiple of 64"); e->sim_chunk = value; return LG_OK; }
    if (std::strcmp(key, "attn_rows") == 0) { if (value != 16 && value != 32 && value != 64) return set_error(LG_ERR_INVALID, "attn_rows must be 16, 32 or 64"); e->attn_rows = value; e->attn_auto_rows = false; return LG_OK; }
    if (std::strcmp(key, "tail_row_tiles") == 0) { if (value != 0 && value != 1 && value != 2 && value != 4) return set_error(LG_ERR_INVALID, "tail_row_tiles must be 0 (automatic), 1, 2 or 4"); e->tail_row_tiles = value; return LG_OK; }
    if (std::strcmp(key, "profile_only") == 0) { e->prof_only = value; return LG_OK; }   // kernel class index, -1 = all classes
    if (std::strcmp(key, "tail_timing") == 0) { e->tail_timing = value; return LG_OK; }   // 1: tail kernel, 2: self projection, 3: self attention (LG_ATTN_TIMING builds), 4: assign sweeps, 5 / 6: layer 0's CrossBlock / SelfBlock tail WITH its fused next projection (stamps of the projection in TAILDBG2)
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

bool pruning_on(const lg_engine* e, const lg_forward_io* io) { return e->cfg.width_confidence > 0 && !(io->flags & LG_FLAG_NO_PRUNING); }
// LG_FLAG_INDEXED: the index fields sit behind the round-5 extension, so they are read only when both flags are set (check_forward_io refuses one without the other)
bool indexed(const lg_forward_io* io) { return (io->flags & LG_FLAG_EXT) && (io->flags & LG_FLAG_INDEXED); }
// bit `side` set: desc0 / desc1 hold binary16 rows (LG_FLAG_DESC0_F16 / _DESC1_F16; check_forward_io refuses them without LG_FLAG_EXT)
int desc_f16_sides(const lg_forward_io* io) { return ((io->flags & LG_FLAG_DESC0_F16) ? 1 : 0) | ((io->flags & LG_FLAG_DESC1_F16) ? 2 : 0); }
PairIndex pair_index(const lg_forward_io* io) { return indexed(io) ? PairIndex{io->index0, io->index1, io->images0, io->images1} : PairIndex{}; }

int check_forward_io(const lg_engine* e, const lg_forward_io* io) {
    if (!e || !io) return set_error(LG_ERR_INVALID, "null argument");
    if (io->flags & (LG_FLAG_DESC0_F16 | LG_FLAG_DESC1_F16)) {   // pure argument checks, ahead of the engine's state: refused on any engine
        if (!(io->flags & LG_FLAG_EXT)) return set_error(LG_ERR_INVALID, "LG_FLAG_DESC0_F16 / LG_FLAG_DESC1_F16 need LG_FLAG_EXT");
        // the kernels read a binary16 row in 16-byte pieces: rows are input_dim * 2 bytes (a multiple of 128), so the base decides
        if (((io->flags & LG_FLAG_DESC0_F16) && (reinterpret_cast<uintptr_t>(io->desc0) & 15)) ||
            ((io->flags & LG_FLAG_DESC1_F16) && (reinterpret_cast<uintptr_t>(io->desc1) & 15)))
            return set_error(LG_ERR_INVALID, "LG_FLAG_DESC0_F16 / LG_FLAG_DESC1_F16: the descriptor pointer must be 16-byte aligned");
    }
    if (!e->weights_ready) return set_error(LG_ERR_STATE, "weights not finalised");
    const int B = io->batch, n0 = io->n0, n1 = io->n1;
    if (B < 1 || n0 < 0 || n1 < 0) return set_error(LG_ERR_INVALID, "bad batch / keypoint counts");
    TRY(check_envelope(B, n0, n1));
    if (!io->stop || !io->n_matches) return set_error(LG_ERR_INVALID, "null output pointer");
    if ((n0 && (!io->matches0 || !io->scores0)) || (n1 && (!io->matches1 || !io->scores1))) return set_error(LG_ERR_INVALID, "null output pointer");
    if (n0 && n1 && (!io->matches || !io->match_scores)) return set_error(LG_ERR_INVALID, "null match-list pointer");
    if (n0 && n1 && (!io->kpts0 || !io->kpts1 || !io->desc0 || !io->desc1)) return set_error(LG_ERR_INVALID, "null input pointer");
    const bool do_prune = pruning_on(e, io);
    if (do_prune && ((n0 && !io->prune0) || (n1 && !io->prune1))) return set_error(LG_ERR_INVALID, "prune0/prune1 required when width_confidence > 0");
    if (e->cfg.add_scale_ori && (!io->scales0 || !io->oris0 || !io->scales1 || !io->oris1)) return set_error(LG_ERR_INVALID, "scales/oris required");
    const bool ext = (io->flags & LG_FLAG_EXT) != 0;            // round-5 extension fields present
    if ((io->flags & LG_FLAG_CHECK_FINITE) && (!ext || !io->status)) return set_error(LG_ERR_INVALID, "LG_FLAG_CHECK_FINITE needs LG_FLAG_EXT and a status array");
    if (io->flags & LG_FLAG_INDEXED) {
        if (!ext || !io->status) return set_error(LG_ERR_INVALID, "LG_FLAG_INDEXED needs LG_FLAG_EXT and a status array");
        if (!io->index0 || !io->index1) return set_error(LG_ERR_INVALID, "LG_FLAG_INDEXED: null index0 / index1");
        if (io->images0 < 1 || io->images1 < 1) return set_error(LG_ERR_INVALID, "LG_FLAG_INDEXED: images0 and images1 must be at least 1");
    }
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
        o.wire = io->wire; o.wire_stride = io->wire_stride; o.wire_prune = pruning_on(e, io) ? 1 : 0; o.status = io->status; o.range_flag = range_flag; o.device_err = device_err;
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
    if (pruning_on(e, io)) { is.prune0 = n0 ? io->prune0 : nullptr; is.prune1 = n1 ? io->prune1 : nullptr; }
    HIPCHK(launch_init_state(is, s));
    HIPCHK(write_outputs(e, io, nullptr, 1, nullptr, nullptr, s));   // stop = 1 for every pair (+ the extension outputs of an empty result)
    return LG_OK;
}
}  // namespace

int lg_engine_forward(lg_engine* e, const lg_forward_io* io, void* hip_stream) {
    TRY(check_forward_io(e, io));
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const int B = io->batch, n0 = io->n0, n1 = io->n1, L = e->cfg.n_layers, D = 256;
    if (n0 == 0 || n1 == 0) return forward_empty(e, io, s);
    const bool do_stop = e->cfg.depth_confidence > 0, do_prune = pruning_on(e, io);
    const bool check_finite = (io->flags & LG_FLAG_EXT) && (io->flags & LG_FLAG_CHECK_FINITE);
    const int max_matches = n0 < n1 ? n0 : n1;

    TRY(ensure_workspace(e, B, n0, n1));
    const int c0 = e->cur_cap0, c1 = e->cur_cap1, R = B * (c0 + c1);
    RowSpace rs_all{B, c0, c1, e->LEN, nullptr};
    RowSpace rs_act{B, c0, c1, e->LEN, e->ACTIVE};
    const int prec = e->cfg.precision, ap = e->attn_prec;
    int step = 0;
#define STEP_DONE() do { if (e->debug_stop >= 0 && step >= e->debug_stop) return LG_OK; ++step; } while (0)
#define PROFILED(cls, launch) do { TRY(prof_begin(e, cls, s)); HIPCHK(launch); TRY(prof_end(e, s)); } while (0)   // one launch inside its profile bracket

    int* const device_err = e->CFLAGS + (size_t)2 * B * compact_chunks(c0, c1);   // error word + compaction ticket behind the chunk flags (lg_adaptive.hip)
    const InitStateArgs is{B, n0, n1, L, io->num0, io->num1, e->LEN, e->LEN_ORIG, e->LEN_OLD, e->ACTIVE, e->FINAL_LAYER,
                           do_prune ? io->prune0 : nullptr, do_prune ? io->prune1 : nullptr, e->RANGEF, device_err, e->XSEL, pair_index(io)};
    HIPCHK(launch_init_state(is, s));
    int* const range_flag = check_finite ? e->RANGEF : nullptr;
    // prep (+ descriptor copy) as its own launch, or — input_dim == 256, no debug stop — inside the first projection launch (lg_proj.hip proj_rows_kernel<FirstRows>)
    const bool fuse_prep = e->fused_prep && e->cfg.input_dim == D && e->debug_stop < 0 && e->tail_timing != 2;
    PrepArgs p{};
    p.rs = rs_all; p.n0 = n0; p.n1 = n1; p.px = pair_index(io); p.kpts0 = io->kpts0; p.kpts1 = io->kpts1; p.size0 = io->size0; p.size1 = io->size1;
    p.scales0 = io->scales0; p.oris0 = io->oris0; p.scales1 = io->scales1; p.oris1 = io->oris1;
    p.Wr = e->Wr; p.pos_dim = 2 + 2 * (e->cfg.add_scale_ori ? 1 : 0);
    p.desc0 = io->desc0; p.desc1 = io->desc1; p.input_dim = e->cfg.input_dim; p.desc_f16 = desc_f16_sides(io);
    p.X = e->X; p.Xin = e->XIN; p.cosb = e->COS; p.sinb = e->SIN; p.ind = e->IND; p.bbox = e->BBOX;
    TRY(prof_begin(e, PC_PREP, s));
    if (fuse_prep) HIPCHK(launch_prep_bbox(p, s)); else HIPCHK(launch_prep(p, s));
    // per-op GEMM out[R][Nout] = [A | A2] W^T + bias on the weights `w_elems` elements into the layer-major matrix W
    auto gemm = [&](const RowSpace& rs, const float* A, int lda, const float* A2, int lda2, int K1, int K, const PackedW& W, size_t w_elems, const float* bias, int Nout, float* out) {
        GemmArgs g{};
        g.rs = rs; g.A = A; g.lda = lda; g.A2 = A2; g.lda2 = lda2; g.K1 = K1; g.K = K; g.bias = bias; g.Nout = Nout; g.out = out; g.ldo = Nout; g.out_scale = 1.f; g.R = R;
        g.W = static_cast<char*>(W.hi) + w_elems * elem_size(prec); g.Wlo = W.lo ? static_cast<char*>(W.lo) + w_elems * elem_size(prec) : nullptr;
        return g;
    };
    if (e->cfg.input_dim != D) {  // ref :521-522
        GemmArgs g = gemm(rs_all, e->XIN, e->cfg.input_dim, nullptr, 0, e->cfg.input_dim, e->cfg.input_dim, e->w_in, 0, e->b_in, D, e->X);
        HIPCHK(launch_gemm(prec, EPI_STORE, g, s));
    }
    TRY(prof_end(e, s));
    STEP_DONE();
    const long long qkv_plane = ap == PREC_F16X3 ? (long long)R * 256 : 0;   // split attention: hi plane, then lo plane, of q / k / v^T

    // current set of residual / rotary buffers: set 0 = X / COS / SIN, set 1 = X2 / COS2 / SIN2; flipped by every gather projection (adaptive width)
    int xcur = 0;
    float* Xs[2] = {e->X, e->X2}; float* Cs[2] = {e->COS, e->COS2}; float* Ss[2] = {e->SIN, e->SIN2};
    bool gather_pending = false;   // the decide step of the previous layer ran in gather mode: the next SelfBlock projection moves the rows
    auto make_proj = [&](int layer, int blk) {   // q/k/v projection of block `blk` of `layer` (lg_proj.hip / fused into lg_tail.hip)
        ProjArgs pj{};
        pj.rs = rs_act; pj.X = Xs[xcur]; pj.R = R; pj.q = e->Q; pj.k = e->K; pj.vt = e->VT; pj.plane = qkv_plane;
        const BlockWeights& bw = e->blocks[blk];
        pj.W = bw.qkv_p + (size_t)layer * bw.qkv_layer_bytes; pj.bias = bw.b_qkv + (size_t)layer * bw.Nout;
        pj.Nout = bw.Nout; pj.n_qk_groups = bw.n_qk_groups;
        if (blk == 0) { pj.cosb = Cs[xcur]; pj.sinb = Ss[xcur]; }   // rotary on q, k of the SelfBlock only
        pj.dbg = nullptr; pj.range_flag = range_flag;
        return pj;
    };
    // fused_next: a tail kernel also runs the NEXT block's projection on the x tile it has just produced.  Across a
    // layer boundary that is only valid when nothing re-orders rows in between (no early stop / pruning step).
    const bool fuse_next = e->fused_next && e->fused_tail && (e->tail_timing == 0 || e->tail_timing == 5 || e->tail_timing == 6) &&
                           e->debug_stop < 0 && launch_tail_supports_next(prec, ap);
    const bool prune_possible = do_prune && (n0 > e->cfg.pruning_min_kpts || n1 > e->cfg.pruning_min_kpts);
    // gather path: the product configuration only (the per-op / debug-stop paths keep the in-place compaction kernel, which the tests compare it with)
    const bool use_gather = e->adapt_gather && e->fused_tail && e->debug_stop < 0 && e->tail_timing == 0;
    bool proj_done = false, final_done = false;
    auto make_final = [&](const RowSpace& rs, int layer, bool per_pair) {   // final projection (ref :289-291: / d**0.25), lg_proj.hip / fused into the last tail
        FinalArgs f{};
        f.rs = rs; f.X = per_pair ? e->X : Xs[xcur]; f.R = R; f.out = e->MD; f.scale = 0.25f;
        f.planes = (prec == PREC_F16X3 && e->sim_planes) ? 1 : 0;
        if (per_pair) { f.X2 = e->X2; f.xsel = e->XSEL; }    // XSEL stays 0 unless a gather projection ran
        f.W = e->w_final_p + (per_pair ? 0 : (size_t)layer * e->final_layer_bytes); f.bias = e->b_final + (per_pair ? 0 : (size_t)layer * D);
        f.layer_of_pair = per_pair ? e->FINAL_LAYER : nullptr; f.w_layer_bytes = (long long)e->final_layer_bytes;
        return f;
    };
    for (int i = 0; i < L; ++i) {
        for (int blk = 0; blk < 2; ++blk) {  // 0 = SelfBlock (ref :159-172), 1 = CrossBlock (ref :201-230)
            const BlockWeights& bw = e->blocks[blk];
            if (!proj_done) {   // otherwise the previous block's tail kernel has already produced q/k/v (fused_next)
                ProjArgs pj = make_proj(i, blk);
                pj.dbg = (e->tail_timing == 2 && blk == 0) ? e->TAILDBG : nullptr;
                TRY(prof_begin(e, blk == 0 ? PC_GEMM_QKV_SELF : PC_GEMM_QKV_CROSS, s));
                if (fuse_prep && i == 0 && blk == 0) {
                    pj.rs = rs_all;                                 // rs_all: what prep covers (pairs with an empty image too)
                    if (launch_proj_first(prec, ap, pj, p, s) != hipSuccess) {
                        //  e.g. the 80 KB of dynamic LDS refused: the separate preparation kernel + the standard projection instead — bit-identical
                        (void)hipGetLastError();
                        HIPCHK(launch_prep(p, s));
                        pj.rs = rs_act;
                        HIPCHK(launch_proj(prec, ap, pj, s));
                    }
                }
                else if (gather_pending && blk == 0) {
                    // the rows of every pair that prunes move to the other buffer set on their way into the projection; pairs that do not prune at this
                    // layer are copied as they are (identity map): one buffer set is current for the whole batch
                    GatherArgs ga{};
                    ga.Xold = Xs[xcur]; ga.cos_old = Cs[xcur]; ga.sin_old = Ss[xcur]; ga.Xnew = Xs[xcur ^ 1]; ga.cos_new = Cs[xcur ^ 1]; ga.sin_new = Ss[xcur ^ 1];
                    ga.src = e->DST; ga.len_old = e->LEN_OLD;
                    HIPCHK(launch_proj_gather(prec, ap, pj, ga, s));
                    xcur ^= 1; gather_pending = false;
                }
                else HIPCHK(launch_proj(prec, ap, pj, s));
                TRY(prof_end(e, s));
            }
            proj_done = false;
            STEP_DONE();
            {
                AttnArgs at{};
                at.rs = rs_act; at.q = e->Q; at.k = e->K; at.vt = e->VT; at.plane = qkv_plane; at.ctx = e->CTX; at.R = R; at.cross = blk;
                at.dbg = (e->tail_timing == 3 && blk == 0) ? e->TAILDBG : nullptr;
                at.rows_per_wave = (e->attn_auto_rows && R / 128 * 4 < 256) ? 16 : e->attn_rows; at.dma = e->attn_dma ? 1 : 0;   // fewer 128-row workgroups than CUs: 64-row ones
                PROFILED(blk == 0 ? PC_ATTN_SELF : PC_ATTN_CROSS, launch_attention(ap, at, s));
            }
            STEP_DONE();
            if (e->fused_tail) {   // out_proj + ffn.0 + LayerNorm + GELU + ffn.3 + residual in one kernel (lg_tail.hip)
                TailArgs ta{};
                ta.rs = rs_act; ta.X = Xs[xcur]; ta.CTX = e->CTX; ta.range_flag = range_flag;
                ta.Wcat = bw.tail_cat + (size_t)i * e->tail_cat_layer_bytes; ta.bcat = bw.b_cat + (size_t)i * 512;
                ta.gamma = bw.ln_g + (size_t)i * 512; ta.beta = bw.ln_b + (size_t)i * 512;
                ta.W2 = bw.tail_2 + (size_t)i * e->tail_2_layer_bytes; ta.b2 = bw.b_f2 + (size_t)i * D;
                if (blk == 1) {   // 256 -> 1 heads on the rows this CrossBlock tail produces
                    // token confidence of layer i (ref :548) for the stop decision; matchability of layer i (ref :298-299): its sigmoid for
                    // the pruning mask (ref :553) and its log-sigmoids as the assignment's matchability terms (ref :268-276) wherever a pair
                    // may END at this layer — the last one, or any one with early stopping
                    const bool last = i + 1 == L;
                    const bool prune_here = !last && do_prune && prune_possible;
                    const bool want_tok = !last && do_stop, want_ls = last || do_stop;
                    if (want_tok) { ta.head_w0 = e->w_tok + (size_t)i * D; ta.head_b0 = e->b_tok + i; ta.head_out0 = e->CONF; }
                    if (prune_here || want_ls) {
                        float* sig = prune_here ? e->MSCORE : nullptr; float* ls = want_ls ? e->LS : nullptr;
                        float* lsneg = (want_ls && io->log_assignment) ? e->LSNEG : nullptr;
                        if (want_tok) { ta.head_w1 = e->w_match + (size_t)i * D; ta.head_b1 = e->b_match + i; ta.head_out1 = sig; ta.head_ls1 = ls; ta.head_lsneg1 = lsneg; }
                        else { ta.head_w0 = e->w_match + (size_t)i * D; ta.head_b0 = e->b_match + i; ta.head_out0 = sig; ta.head_ls0 = ls; ta.head_lsneg0 = lsneg; }
                    }
                }
                ta.dbg = (e->tail_timing == 1 || (i == 0 && ((e->tail_timing == 5 && blk == 1) || (e->tail_timing == 6 && blk == 0)))) ? e->TAILDBG : nullptr;
                ta.row_tiles = e->tail_row_tiles ? e->tail_row_tiles : tail_row_tiles_for(R);
                // Across a layer boundary the fusion is valid whenever no row can MOVE in between: early stop alone only
                // deactivates a pair (its speculative projection is never read), pruning re-orders rows — but it cannot
                // happen while every segment is at or below the pruning threshold (ref :551 / :559; lengths only shrink).
                if (fuse_next && (blk == 0 || (i + 1 < L && !prune_possible))) {
                    ta.next = make_proj(i + blk, blk ^ 1);   // this layer's CrossBlock, or the next layer's SelfBlock
                    if (ta.dbg && e->tail_timing >= 5) ta.next.dbg = e->TAILDBG2;
                    proj_done = true;
                } else if (fuse_next && blk == 1 && i + 1 == L && !do_stop) {
                    // fixed depth: every live pair ends here, so the LAST tail also runs the final projection of the log assignment on its x tile
                    ta.fin = make_final(rs_act, L - 1, false);
                    final_done = true;
                }
                PROFILED(PC_TAIL, launch_tail(prec, ap, ta, s));
                STEP_DONE(); STEP_DONE(); STEP_DONE(); STEP_DONE();
                continue;
            }
            {
                GemmArgs g = gemm(rs_act, e->CTX, D, nullptr, 0, D, D, bw.out, (size_t)i * D * D, bw.b_out + (size_t)i * D, D, e->MSG);
                PROFILED(PC_GEMM_OUT, launch_gemm(prec, EPI_STORE, g, s));
            }
            STEP_DONE();
            {
                GemmArgs g = gemm(rs_act, e->X, D, e->MSG, D, D, 512, bw.f1, (size_t)i * 512 * 512, bw.b_f1 + (size_t)i * 512, 512, e->H1);
                PROFILED(PC_GEMM_FFN1, launch_gemm(prec, EPI_STORE, g, s));
            }
            STEP_DONE();
            {
                LnGeluArgs ln{rs_act, e->H1, e->G, bw.ln_g + (size_t)i * 512, bw.ln_b + (size_t)i * 512, R};
                PROFILED(PC_LN_GELU, launch_ln_gelu(ln, s));
            }
            STEP_DONE();
            {
                GemmArgs g = gemm(rs_act, e->G, 512, nullptr, 0, 512, 512, bw.f2, (size_t)i * D * 512, bw.b_f2 + (size_t)i * D, D, e->X);
                PROFILED(PC_GEMM_FFN2, launch_gemm(prec, EPI_RESID, g, s));
            }
            STEP_DONE();
        }
        if (i == L - 1) break;  // ref :544-545
        const bool prune_now = do_prune && prune_possible;   // below the threshold the pruning branch is never taken (ref :551 / :559)
        if (do_stop || prune_now) {
            if (!e->fused_tail) {   // per-op path: the 256 -> 1 heads as their own pass (the fused CrossBlock tail computes them in its epilogue)
                RowDotArgs rd{};
                rd.rs = rs_act; rd.X = e->X;
                if (do_stop) { rd.w0 = e->w_tok + (size_t)i * D; rd.b0 = e->b_tok + i; rd.out0 = e->CONF; rd.act0 = 1; }
                if (do_stop && prune_now) { rd.w1 = e->w_match + (size_t)i * D; rd.b1 = e->b_match + i; rd.out1 = e->MSCORE; rd.act1 = 1; }
                else if (prune_now) { rd.w0 = e->w_match + (size_t)i * D; rd.b0 = e->b_match + i; rd.out0 = e->MSCORE; rd.act0 = 1; }
                PROFILED(PC_ROWDOT, launch_rowdot(rd, s));
            }
            AdaptArgs ad{};
            ad.rs = rs_act; ad.len = e->LEN; ad.active = e->ACTIVE; ad.len_old = e->LEN_OLD; ad.final_layer = e->FINAL_LAYER;
            ad.ind = e->IND; ad.dst = e->DST; ad.prune0 = io->prune0; ad.prune1 = io->prune1; ad.n0 = n0; ad.n1 = n1; ad.len_orig = e->LEN_ORIG;
            ad.conf = e->CONF; ad.mscore = e->MSCORE; ad.X = e->X; ad.cosb = e->COS; ad.sinb = e->SIN;
            if (use_gather && prune_now) { ad.gather = 1; ad.src = e->DST; ad.xsel = e->XSEL; ad.xnext = xcur ^ 1; gather_pending = true; }
            ad.layer = i;
            // ref :631-634 threshold (float32 buffer), :656 and :640 compare in float32
            ad.conf_thr = (float)std::fmin(std::fmax(0.8 + 0.1 * std::exp(-4.0 * i / L), 0.0), 1.0);
            ad.depth_conf = (float)e->cfg.depth_confidence;
            ad.width_conf = (float)(1.0 - e->cfg.width_confidence);
            ad.pruning_min_kpts = e->cfg.pruning_min_kpts;
            ad.do_stop = do_stop; ad.do_prune = prune_now;
            ad.compact_chunks = compact_chunks(c0, c1); ad.compact_flags = e->CFLAGS; ad.compact_err = device_err; ad.compact_ticket = device_err + 1;
            if (prune_now && !e->cflags_clean) {   // fresh carve: whatever the arena held there must not look like an epoch
                HIPCHK(hipMemsetAsync(e->CFLAGS, 0, cflags_bytes(B, c0, c1), s));
                e->cflags_clean = true;
            }
            ad.compact_epoch = ++e->compact_epoch;
            PROFILED(PC_ADAPTIVE, launch_adapt(ad, s));
        }
    }
    // ---- log assignment with the weights of the layer each pair stopped at (ref :591)
    {
        if (!e->fused_tail) {   // per-op path: matchability terms as their own pass (the fused CrossBlock tails emit them from their heads)
            RowDotArgs rd{};
            rd.rs = rs_all; rd.X = e->X; rd.w0 = e->w_match; rd.b0 = e->b_match; rd.out0 = e->LS; rd.act0 = 2;
            rd.layer_of_pair = e->FINAL_LAYER; rd.w_layer_stride = D; rd.ignore_active = 1;
            if (io->log_assignment) { rd.w1 = e->w_match; rd.b1 = e->b_match; rd.out1 = e->LSNEG; rd.act1 = 3; }  // dustbin terms
            PROFILED(PC_ROWDOT, launch_rowdot(rd, s));
        }
        if (!final_done) {
            PROFILED(PC_GEMM_FINAL, launch_final_proj(prec, make_final(rs_all, 0, true), s));
        }
        TRY(prof_begin(e, PC_SIM, s));
        if (prec == PREC_F16X3 && e->sim_planes) {
            SimPlanesArgs sp{rs_all, reinterpret_cast<const f16_t*>(e->MD), (long long)R * 256, D, e->SIM, e->sim_chunk};
            HIPCHK(launch_sim_planes(sp, s));
        } else {
            SimArgs sm{rs_all, e->MD, D, D, e->SIM};
            HIPCHK(launch_sim(prec, sm, s));
        }
        TRY(prof_end(e, s));
        AssignArgs as{};
        as.rs = rs_all; as.sim = e->SIM; as.ls = e->LS; as.lse_r = e->LSE_R; as.lse_c = e->LSE_C; as.max0 = e->MAX0; as.arg0 = e->ARG0;
        as.max1 = e->MAX1; as.arg1 = e->ARG1; as.cpm = e->CPM; as.cps = e->CPS; as.cbv = e->CBV; as.cbi = e->CBI; as.ind = e->IND; as.n0 = n0; as.n1 = n1; as.filter_threshold = (float)e->cfg.filter_threshold;
        as.m0 = io->matches0; as.m1 = io->matches1; as.s0 = io->scores0; as.s1 = io->scores1;
        as.matches = io->matches; as.mscores = io->match_scores; as.n_matches = io->n_matches; as.max_matches = max_matches;
        as.log_assignment = io->log_assignment; as.lsneg = e->LSNEG;
        as.dbg = e->tail_timing == 4 ? e->TAILDBG : nullptr;
        as.all_rows_live = (!do_prune && !io->num0 && !io->num1 && !indexed(io)) ? 1 : 0;   // indexed: a pair whose index is out of range has no live row
        PROFILED(PC_ASSIGN, launch_assign(as, s));
        HIPCHK(write_outputs(e, io, e->FINAL_LAYER, 0, range_flag, device_err, s));
    }
#undef PROFILED
#undef STEP_DONE
    return LG_OK;
}

}  // extern "C"
