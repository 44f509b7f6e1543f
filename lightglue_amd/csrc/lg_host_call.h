// lightglue_amd — the host side the entry points over a pair list or a caller's workspace share (lg_engine_forward, lg_nn_match, lg_twoview_verify,
// lg_relpose_estimate, lg_abspose_estimate, lg_sift_filter) and the solvers (lg_bundle_adjust*, lg_posegraph_solve, lg_positioning_solve): their refusals, the
// carving of a workspace, the stateless entry points' layouts, the cut of a pair list into launches, the panel loop of the Cholesky, and the whole opening of
// a call of the three hypothesise-and-verify estimators (check_estimator_call).  Host-only C++17
// like lg_forward_plan.h (no HIP header, no device type): tests/cpp/host_call_check.cpp walks it with any host compiler, and under its address sanitizer.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/lightglue_amd.h"

namespace lg {

// the error every C entry point reports: sets the message lg_last_error() returns (lg_api.hip) and returns `code`
int set_error(int code, const std::string& msg);

// ---------------------------------------------------------------- refusals; every message starts with the entry point's name (`stage`)
// THE LG_FLAG_INDEXED rule.  (The engine also asks for LG_FLAG_EXT and a status array, check_forward_io: its index fields sit behind the round-5 extension.)
inline int check_pair_list(const char* stage, uint32_t flags, const void* index0, const void* index1, long long images0, long long images1) {
    if ((flags & LG_FLAG_INDEXED) && (!index0 || !index1 || images0 < 1 || images1 < 1))
        return set_error(LG_ERR_INVALID, std::string(stage) + ": LG_FLAG_INDEXED needs index0, index1 and images0, images1 >= 1");
    return LG_OK;
}
// A caller's workspace of `need` bytes (what `size_function` returns): null — accepted for 0 bytes with null_if_empty, lg_nn_match over empty stores —, too small, not aligned
inline int check_workspace(const char* stage, const char* size_function, const void* ptr, long long bytes, long long need, bool null_if_empty = false) {
    if (!ptr && !(null_if_empty && need == 0)) return set_error(LG_ERR_INVALID, std::string(stage) + ": null workspace");
    if (bytes < need)
        return set_error(LG_ERR_INVALID, std::string(stage) + ": the workspace holds " + std::to_string(bytes) + " bytes, " + size_function + " = " + std::to_string(need));
    if (reinterpret_cast<uintptr_t>(ptr) & 255) return set_error(LG_ERR_INVALID, std::string(stage) + ": the workspace must be 256-byte aligned");
    return LG_OK;
}
// THE "> 0 (and finite)" test of every fp64 setting
inline bool positive(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }
// keypoint rows per image of a call: nullptr, or why they are refused
inline const char* keypoint_counts_error(int n0, int n1 = 0) {
    return n0 < 0 || n1 < 0 || n0 > LG_MAX_KEYPOINTS || n1 > LG_MAX_KEYPOINTS ? "n0, n1 must lie in [0, LG_MAX_KEYPOINTS]" : nullptr;
}

// ---------------------------------------------------------------- workspace carving (every piece at a 256-byte aligned offset) and the three layouts
struct Bump {
    long long used = 0;
    long long take(long long bytes) { const long long o = used; used += (bytes + 255) / 256 * 256; return o; }
};
// typed pointers into a workspace at a layout's offsets
struct Carved {
    char* base;
    explicit Carved(void* workspace) : base(static_cast<char*>(workspace)) {}
    template <class T> T* as(long long at) const { return reinterpret_cast<T*>(base + at); }
    int* ints(long long at) const { return as<int>(at); }
    double* f64(long long at) const { return as<double>(at); }
};
// lg_nn_match: the normalised fp32 rows of either store, one "touched" byte per image of either store.  No pair count: the size depends on the stores alone.
constexpr uint32_t NN_KNOWN_FLAGS = LG_FLAG_INDEXED | LG_FLAG_DESC0_F16 | LG_FLAG_DESC1_F16 | LG_SIFT_STORE_FLAGS | LG_FLAG_NN_MUTUAL;
struct NnLayout { long long rows0, rows1, ws0, ws1, touched0, touched1, total; };
inline const char* nn_layout(long long images0, long long images1, int n0, int n1, int dim, uint32_t flags, NnLayout& L) {
    if (dim < 16 || dim > 256 || dim % 16) return "dim must be a multiple of 16 in [16, 256]";
    if (const char* why = keypoint_counts_error(n0, n1)) return why;
    if (images0 < 0 || images1 < 0) return "negative image count";
    if (flags & ~NN_KNOWN_FLAGS) return "unknown flag bits (the nearest-neighbour matcher reads LG_FLAG_INDEXED, the per-side descriptor flags and LG_FLAG_NN_MUTUAL)";
    if (((flags & LG_FLAG_DESC0_F16) && (flags & LG_FLAG_DESC0_U8)) || ((flags & LG_FLAG_DESC1_F16) && (flags & LG_FLAG_DESC1_U8)))
        return "a side is stored as binary16 or as uint8, not both";
    L.rows0 = images0 * n0; L.rows1 = images1 * n1;
    if (L.rows0 > 0x7FFFFFFFLL || L.rows1 > 0x7FFFFFFFLL) return "a store of more than 2^31 - 1 rows";
    Bump bp;
    L.ws0 = bp.take(L.rows0 * dim * 4); L.ws1 = bp.take(L.rows1 * dim * 4); L.touched0 = bp.take(images0); L.touched1 = bp.take(images1); L.total = bp.used;
    return nullptr;
}
// the three hypothesise-and-verify estimators: the budget, and what their layouts refuse first (the pair count, n0, flag bits outside `known`)
inline const char* hypothesis_budget_error(long long num_hypotheses) {
    return num_hypotheses < 256 || num_hypotheses > 65536 || num_hypotheses % 256 ? "num_hypotheses must be a multiple of 256 in [256, 65536]" : nullptr;
}
inline const char* pair_rows_error(long long pairs, int n0, uint32_t flags, uint32_t known, const char* undefined_bits) {
    if (pairs < 0 || pairs > 0x7FFFFFFFLL) return "the pair count must lie in [0, 2^31 - 1]";
    if (const char* why = keypoint_counts_error(n0)) return why;
    return flags & ~known ? undefined_bits : nullptr;
}
// lg_twoview_verify: one 32-byte record per pair, the correspondence list (16 bytes per row) and its image-0 rows (4 bytes per row) of every pair
constexpr uint32_t TV_KNOWN_FLAGS = LG_FLAG_INDEXED | LG_TWOVIEW_HOMOGRAPHY | LG_TWOVIEW_FUNDAMENTAL | LG_TWOVIEW_REFINE | LG_TWOVIEW_GIVEN_MODELS;
struct TvLayout { long long head, corr, rows, total; };
inline const char* tv_layout(long long pairs, int n0, uint32_t flags, TvLayout& L) {
    if (const char* why = pair_rows_error(pairs, n0, flags, TV_KNOWN_FLAGS, "undefined flag bits (the verifier reads LG_FLAG_INDEXED and the LG_TWOVIEW_* bits)")) return why;
    if (!(flags & LG_TWOVIEW_HOMOGRAPHY) == !(flags & LG_TWOVIEW_FUNDAMENTAL)) return "exactly one of LG_TWOVIEW_HOMOGRAPHY and LG_TWOVIEW_FUNDAMENTAL must be set";
    Bump bp;
    L.head = bp.take(pairs * 32); L.corr = bp.take(pairs * n0 * 16); L.rows = bp.take(pairs * n0 * 4); L.total = bp.used;
    return nullptr;
}
// lg_relpose_estimate: the verifier's record, list and rows per pair, a 48-byte record per pair (the 64-bit key, the two cameras) and the candidate models:
// LG_RELPOSE_ROOTS x 9 floats per hypothesis and pair
constexpr uint32_t RP_KNOWN_FLAGS = LG_FLAG_INDEXED | LG_RELPOSE_REFINE;
struct RpLayout { long long head, ext, corr, rows, cand, total; };
inline const char* rp_layout(long long pairs, int n0, long long num_hypotheses, uint32_t flags, RpLayout& L) {
    if (const char* why = pair_rows_error(pairs, n0, flags, RP_KNOWN_FLAGS, "undefined flag bits (the pose estimator reads LG_FLAG_INDEXED and LG_RELPOSE_REFINE)")) return why;
    if (const char* why = hypothesis_budget_error(num_hypotheses)) return why;
    Bump bp;
    L.head = bp.take(pairs * 32); L.ext = bp.take(pairs * 48); L.corr = bp.take(pairs * n0 * 16); L.rows = bp.take(pairs * n0 * 4);
    L.cand = bp.take(pairs * num_hypotheses * LG_RELPOSE_ROOTS * 36); L.total = bp.used;
    return nullptr;
}
// lg_abspose_estimate: a 64-byte record per pair (a problem is at most every pair on its own) and, per row of matches0, the correspondence (x, y, X', Y' as one
// float4, Z' as one float2) and the row's place in its problem
constexpr uint32_t AP_KNOWN_FLAGS = LG_FLAG_INDEXED | LG_ABSPOSE_REFINE | LG_ABSPOSE_GROUPED | LG_ABSPOSE_GIVEN_POSES;
struct ApLayout { long long head, ca, cb, rows, total; };
inline const char* ap_layout(long long pairs, int n0, long long num_hypotheses, uint32_t flags, ApLayout& L) {
    if (const char* why = pair_rows_error(pairs, n0, flags, AP_KNOWN_FLAGS, "undefined flag bits (the absolute-pose estimator reads LG_FLAG_INDEXED and the LG_ABSPOSE_* bits)"))
        return why;
    if (const char* why = hypothesis_budget_error(num_hypotheses)) return why;
    if ((flags & LG_ABSPOSE_GROUPED) && pairs * n0 > LG_MAX_ROWS) return "with LG_ABSPOSE_GROUPED pairs x n0 must not exceed LG_MAX_ROWS";
    Bump bp;
    L.head = bp.take(pairs * 64); L.ca = bp.take(pairs * n0 * 16); L.cb = bp.take(pairs * n0 * 8); L.rows = bp.take(pairs * n0 * 4); L.total = bp.used;
    return nullptr;
}
// ---------------------------------------------------------------- the opening of a call of lg_twoview_verify / lg_relpose_estimate / lg_abspose_estimate.  What differs
// per entry point is its layout and the pointers it needs, one overload each; the refusals and their order are written once
inline const char* io_layout(const lg_twoview_io& io, TvLayout& L) { return tv_layout(io.pairs, io.n0, io.flags, L); }
inline const char* io_layout(const lg_relpose_io& io, RpLayout& L) { return rp_layout(io.pairs, io.n0, io.num_hypotheses, io.flags, L); }
inline const char* io_layout(const lg_abspose_io& io, ApLayout& L) { return ap_layout(io.pairs, io.n0, io.num_hypotheses, io.flags, L); }
inline const char* io_pointers_error(const lg_twoview_io& io) {
    const int n0 = io.n0, n1 = io.n1;
    if (!io.models || !io.num_inliers || !io.status || (n0 && (!io.inliers0 || !io.matches0)) || (n0 && n1 && (!io.kpts0 || !io.kpts1)) ||
        ((io.flags & LG_TWOVIEW_GIVEN_MODELS) && !io.models_in))
        return "null pointer among kpts0, kpts1, matches0, models_in, models, inliers0, num_inliers, status";
    return nullptr;
}
inline const char* io_pointers_error(const lg_relpose_io& io) {
    const int n0 = io.n0, n1 = io.n1;
    if (!io.cameras0 || !io.cameras1 || !io.rotations || !io.translations || !io.essentials || !io.models || !io.num_inliers || !io.num_in_front || !io.status ||
        (n0 && (!io.inliers0 || !io.matches0)) || (n0 && n1 && (!io.kpts0 || !io.kpts1)))
        return "null pointer among kpts0, kpts1, matches0, cameras0, cameras1, rotations, translations, essentials, models, inliers0, num_inliers, num_in_front, status";
    return nullptr;
}
inline const char* io_pointers_error(const lg_abspose_io& io) {
    const int n0 = io.n0, n1 = io.n1;
    const bool grouped = io.flags & LG_ABSPOSE_GROUPED;
    if (!io.cameras0 || !io.rotations || !io.translations || !io.num_inliers || !io.pair_num_inliers || !io.status || ((io.flags & LG_ABSPOSE_GIVEN_POSES) && !io.poses_in) ||
        (n0 && (!io.inliers0 || !io.matches0 || !io.kpts0)) || (n0 && n1 && !io.points3d1))
        return "null pointer among kpts0, points3d1, matches0, cameras0, poses_in (LG_ABSPOSE_GIVEN_POSES), rotations, translations, num_inliers, inliers0, pair_num_inliers, status";
    if (grouped && (!io.group_offsets || !io.group_pairs)) return "null pointer: LG_ABSPOSE_GROUPED needs group_offsets and group_pairs";
    if (grouped && io.pairs > 0 && (io.groups < 1 || io.groups > io.pairs)) return "with LG_ABSPOSE_GROUPED groups must lie in [1, pairs]";
    return nullptr;
}
// LG_OK and the layout in L, or the first refusal in this order: null io, the layout's, n1, the hypothesis budget, the threshold, the pair list, the entry
// point's pointers, the workspace (`size_function` names what sizes it)
template <class IO, class Layout> int check_estimator_call(const char* stage, const char* size_function, const IO* io, Layout& L) {
    const auto refuse = [stage](const char* why) { return set_error(LG_ERR_INVALID, std::string(stage) + ": " + why); };
    if (!io) return refuse("null io");
    if (const char* why = io_layout(*io, L)) return refuse(why);
    if (const char* why = keypoint_counts_error(0, io->n1)) return refuse(why);
    if (const char* why = hypothesis_budget_error(io->num_hypotheses)) return refuse(why);       // two-view only: the pose layouts have refused it already
    if (!(io->threshold > 0.f) || !(io->threshold <= 3.0e18f)) return refuse("threshold must be > 0 (and finite)");
    if (const int rc = check_pair_list(stage, io->flags, io->index0, io->index1, io->images0, io->images1)) return rc;
    if (const char* why = io_pointers_error(*io)) return refuse(why);
    return check_workspace(stage, size_function, io->workspace, io->workspace_bytes, L.total);
}

// lg_triangulate: a 256-byte record of the call, a 160-byte record per image, seven int32 per node (parent, root, count, list offset, component, fill cursor,
// list entry) and, per possible track (at most every second node), its root, state, dense id and (X, Y, Z, error)
constexpr uint32_t TRI_KNOWN_FLAGS = LG_TRI_REFINE | LG_TRI_TRACKS_ONLY;
struct TriLayout { long long nodes, tracks, head, rec, parent, root, cnt, off, comp, cursor, list, croot, cstate, tid, cres, total; };
inline const char* tri_layout(long long images, long long n, uint32_t flags, TriLayout& L) {
    if (flags & ~TRI_KNOWN_FLAGS) return "undefined flag bits (the triangulator reads LG_TRI_REFINE and LG_TRI_TRACKS_ONLY)";
    if (n < 0 || n > LG_MAX_KEYPOINTS) return "n must lie in [0, LG_MAX_KEYPOINTS]";
    if (images < 0 || images > LG_MAX_ROWS || images * n > LG_MAX_ROWS) return "images and images x n must lie in [0, LG_MAX_ROWS]";
    L.nodes = images * n; L.tracks = L.nodes / 2;
    Bump bp;
    L.head = bp.take(256); L.rec = bp.take(images * 160);
    L.parent = bp.take(L.nodes * 4); L.root = bp.take(L.nodes * 4); L.cnt = bp.take(L.nodes * 4); L.off = bp.take(L.nodes * 4); L.comp = bp.take(L.nodes * 4);
    L.cursor = bp.take(L.nodes * 4); L.list = bp.take(L.nodes * 4);
    L.croot = bp.take(L.tracks * 4); L.cstate = bp.take(L.tracks * 4); L.tid = bp.take(L.tracks * 4); L.cres = bp.take(L.tracks * 16); L.total = bp.used;
    return nullptr;
}
// lg_triangulate_robust: lg_triangulate's layout, then two more int32 per node (the consensus list of the running round, the round that took the node) and,
// per slot (possible component x max_tracks), its state, dense id, consensus size and (X, Y, Z, error)
struct TriRobustLayout { TriLayout base; long long cons, nround, sstate, stid, slen, sres, total; };
inline const char* tri_robust_layout(long long images, long long n, uint32_t flags, long long max_tracks, TriRobustLayout& L) {
    if (flags & ~LG_TRI_REFINE) return "undefined flag bits (the robust triangulator reads LG_TRI_REFINE)";
    if (const char* why = tri_layout(images, n, flags, L.base)) return why;
    if (max_tracks < 1 || max_tracks > LG_TRI_MAX_TRACKS) return "max_tracks must lie in [1, LG_TRI_MAX_TRACKS]";
    const long long nodes = L.base.nodes, slots = L.base.tracks * max_tracks;
    Bump bp;
    bp.used = L.base.total;
    L.cons = bp.take(nodes * 4); L.nround = bp.take(nodes * 4);
    L.sstate = bp.take(slots * 4); L.stid = bp.take(slots * 4); L.slen = bp.take(slots * 4); L.sres = bp.take(slots * 16); L.total = bp.used;
    return nullptr;
}
// lg_bundle_adjust: a 256-byte record of the call; per image a 64-byte record, the pose twice in fp64 (the state and the trial: 192 bytes), its step (48) and
// its cost (8); the reduced camera system with its right-hand side as one more row ((6 images + 1) x 6 images fp64); per node its track-list entry and that
// entry's image (8 bytes); per track three int32 (count, offset, cursor) and fifteen + three fp64 (the point twice, the inverse of its damped 3 x 3 block, that
// inverse times its gradient: 156 bytes in all).  W is not stored: it is formed again from the pose and the point where it is needed
constexpr uint32_t BA_KNOWN_FLAGS = 0u;
struct BaLayout { long long nodes, dim, head, rec, pose, delta, icost, S, list, limg, tcnt, toff, tcur, X, Vinv, y, total; };
// dense = false (lg_bundle_adjust_pcg): no S, and the image bound is LG_BA_PCG_MAX_IMAGES
inline const char* ba_layout(long long images, long long n, long long tracks, uint32_t flags, BaLayout& L, long long cols = 6, bool dense = true) {   // cols: unknowns per image
    if (flags & ~BA_KNOWN_FLAGS) return "undefined flag bits (the bundle adjuster defines none)";
    if (n < 0 || n > LG_MAX_KEYPOINTS) return "n must lie in [0, LG_MAX_KEYPOINTS]";
    if (dense && (images < 1 || images > LG_BA_MAX_IMAGES)) return "images must lie in [1, LG_BA_MAX_IMAGES]";
    if (!dense && (images < 1 || images > LG_BA_PCG_MAX_IMAGES)) return "images must lie in [1, LG_BA_PCG_MAX_IMAGES]";
    if (images * n > LG_MAX_ROWS) return "images x n must lie in [0, LG_MAX_ROWS]";
    if (tracks < 0 || tracks > images * n / 2) return "tracks must lie in [0, images x n / 2]";
    L.nodes = images * n; L.dim = cols * images;
    Bump bp;
    L.head = bp.take(256); L.rec = bp.take(images * 64); L.pose = bp.take(images * 192); L.delta = bp.take(images * cols * 8); L.icost = bp.take(images * 8);
    L.S = bp.take(dense ? (L.dim + 1) * L.dim * 8 : 0);
    L.list = bp.take(L.nodes * 4); L.limg = bp.take(L.nodes * 4);
    L.tcnt = bp.take(tracks * 4); L.toff = bp.take(tracks * 4); L.tcur = bp.take(tracks * 4);
    L.X = bp.take(tracks * 48); L.Vinv = bp.take(tracks * 72); L.y = bp.take(tracks * 24); L.total = bp.used;
    return nullptr;
}
// what lg_bundle_adjust and lg_bundle_adjust_robust refuse once the layout stands, in this order: the budget, damping and tolerance, a null pointer, the
// workspace of `need` bytes (`size_function` names what sizes it)
inline int ba_check_settings(const char* stage, const char* size_function, const lg_bundle_io& io, long long nodes, long long need) {
    const auto refuse = [stage](const char* why) { return set_error(LG_ERR_INVALID, std::string(stage) + ": " + why); };
    if (io.num_iterations < 1 || io.num_iterations > LG_BA_MAX_ITERATIONS) return refuse("num_iterations must lie in [1, LG_BA_MAX_ITERATIONS]");
    if (!positive(io.initial_damping) || !positive(io.function_tolerance)) return refuse("initial_damping and function_tolerance must be > 0 (and finite)");
    if (!io.cameras || !io.poses || !io.constant_pose || !io.poses_out || !io.summary || !io.status || (io.tracks && (!io.xyz || !io.xyz_out)) ||
        (nodes && (!io.kpts || !io.track_id || !io.points3d || !io.node_state || !io.observation_error)))
        return refuse("null pointer among kpts, track_id, xyz, cameras, poses, constant_pose, poses_out, xyz_out, points3d, node_state, observation_error, summary, status");
    return check_workspace(stage, size_function, io.workspace, io.workspace_bytes, need);
}
// lg_bundle_adjust_robust: lg_bundle_adjust's layout, then one int32 per track (it moved in an earlier stage)
struct BaRobustLayout { BaLayout base; long long tmov, total; };
inline const char* ba_robust_layout(long long images, long long n, long long tracks, uint32_t flags, BaRobustLayout& L, long long cols = 6, bool dense = true) {
    if (const char* why = ba_layout(images, n, tracks, flags, L.base, cols, dense)) return why;
    Bump bp;
    bp.used = L.base.total;
    L.tmov = bp.take(tracks * 4); L.total = bp.used;
    return nullptr;
}
inline const char* ba_robust_settings_error(long long loss, double loss_scale, long long filter_rounds, double max_reproj_error) {
    if (loss < LG_BA_LOSS_SQUARED || loss > LG_BA_LOSS_CAUCHY) return "loss must be LG_BA_LOSS_SQUARED, LG_BA_LOSS_HUBER or LG_BA_LOSS_CAUCHY";
    if (loss != LG_BA_LOSS_SQUARED && !positive(loss_scale)) return "loss_scale must be > 0 (and finite) with a robust loss";
    if (filter_rounds < 0 || filter_rounds > LG_BA_MAX_FILTER_ROUNDS) return "filter_rounds must lie in [0, LG_BA_MAX_FILTER_ROUNDS]";
    if (filter_rounds > 0 && !positive(max_reproj_error)) return "max_reproj_error must be > 0 (and finite) with filter_rounds > 0";
    return nullptr;
}
// lg_bundle_adjust_pcg: lg_bundle_adjust_robust's layout without S, then a 256-byte record of the solver; per image r, z, p, q (4 x 48 bytes), U' and M
// (2 x 288) and its partials of p.q and r.z (2 x 8): 784 bytes; per track u (24 bytes).  x is the step (`delta`) of lg_bundle_adjust's layout
struct BaPcgLayout { BaRobustLayout base; long long head, r, z, p, q, U, M, pq, rz, u, total; };
inline const char* ba_pcg_layout(long long images, long long n, long long tracks, uint32_t flags, BaPcgLayout& L) {
    if (const char* why = ba_robust_layout(images, n, tracks, flags, L.base, 6, false)) return why;
    Bump bp;
    bp.used = L.base.total;
    L.head = bp.take(256); L.r = bp.take(images * 48); L.z = bp.take(images * 48); L.p = bp.take(images * 48); L.q = bp.take(images * 48);
    L.U = bp.take(images * 288); L.M = bp.take(images * 288); L.pq = bp.take(images * 8); L.rz = bp.take(images * 8); L.u = bp.take(tracks * 24); L.total = bp.used;
    return nullptr;
}
// the solver's own settings; the product counts the solver iterations the call enqueues
inline const char* ba_pcg_settings_error(long long num_iterations, long long filter_rounds, long long max_cg_iterations, long long pad, double cg_tolerance) {
    if (pad != 0) return "pad must be 0";
    if (max_cg_iterations < 1 || max_cg_iterations > LG_BA_PCG_MAX_CG_ITERATIONS) return "max_cg_iterations must lie in [1, LG_BA_PCG_MAX_CG_ITERATIONS]";
    if (!(cg_tolerance > 0.0 && cg_tolerance < 1.0)) return "cg_tolerance must lie in (0, 1)";
    if (num_iterations >= 1 && filter_rounds >= 0 && num_iterations * (filter_rounds + 1) * max_cg_iterations > LG_BA_PCG_MAX_SOLVER_ITERATIONS)
        return "num_iterations x (filter_rounds + 1) x max_cg_iterations must not exceed LG_BA_PCG_MAX_SOLVER_ITERATIONS";
    return nullptr;
}
// lg_bundle_adjust_focal: lg_bundle_adjust_robust's layout with 7 unknowns per image (the step is 56 bytes, S is (7 images + 1) x 7 images), then the camera
// state twice in fp64 (64 bytes per image)
struct BaFocalLayout { BaRobustLayout base; long long cam, total; };
inline const char* ba_focal_layout(long long images, long long n, long long tracks, uint32_t flags, BaFocalLayout& L) {
    if (const char* why = ba_robust_layout(images, n, tracks, flags, L.base, 7)) return why;
    Bump bp;
    bp.used = L.base.total;
    L.cam = bp.take(images * 64); L.total = bp.used;
    return nullptr;
}
// what lg_bundle_adjust_focal refuses once the layout stands, in this order: the robust settings, cameras_out, lg_bundle_adjust's list (ba_check_settings)
inline int ba_focal_check_settings(const char* stage, const lg_bundle_focal_io& io, const BaFocalLayout& L) {
    const auto refuse = [stage](const char* why) { return set_error(LG_ERR_INVALID, std::string(stage) + ": " + why); };
    const lg_bundle_robust_io& r = io.base;
    if (const char* why = ba_robust_settings_error(r.loss, r.loss_scale, r.filter_rounds, r.max_reproj_error)) return refuse(why);
    if (!io.cameras_out) return refuse("null pointer cameras_out");
    return ba_check_settings(stage, "lg_bundle_focal_workspace_bytes", r.base, L.base.base.nodes, L.total);
}
// lg_posegraph_solve: a 256-byte record of the call; per image its rotation and centre in fp64 (96 bytes) and five int32 (level, present, list count, list
// offset, fill cursor; the offsets hold one more entry); per pair its state (4), its rotation error (8), its direction (24) and its two adjacency entries
// (16); the larger of the two systems with its right-hand side row: (3 images + 1) x 3 images fp64 (the rotation system, (images + 3) x images, fits in it)
constexpr uint32_t PG_KNOWN_FLAGS = 0u;
constexpr long long PG_MAX_PAIRS = 1LL << 20;
struct PgLayout { long long head, rot, cen, level, present, acount, aoff, acur, pstate, perr, dir, adj, S, total; };
inline const char* pg_layout(long long images, long long pairs, uint32_t flags, PgLayout& L) {
    if (flags & ~PG_KNOWN_FLAGS) return "undefined flag bits (the pose-graph solver defines none)";
    if (images < 2 || images > LG_BA_MAX_IMAGES) return "images must lie in [2, LG_BA_MAX_IMAGES]";
    if (pairs < 1 || pairs > PG_MAX_PAIRS) return "pairs must lie in [1, 2^20]";
    Bump bp;
    L.head = bp.take(256); L.rot = bp.take(images * 72); L.cen = bp.take(images * 24);
    L.level = bp.take(images * 4); L.present = bp.take(images * 4); L.acount = bp.take(images * 4); L.aoff = bp.take((images + 1) * 4); L.acur = bp.take(images * 4);
    L.pstate = bp.take(pairs * 4); L.perr = bp.take(pairs * 8); L.dir = bp.take(pairs * 24); L.adj = bp.take(pairs * 16);
    L.S = bp.take((3 * images + 1) * 3 * images * 8); L.total = bp.used;
    return nullptr;
}
inline const char* pg_settings_error(long long images, long long num_iterations, long long origin, long long baseline, double rotation_scale,
                                     double max_rotation_error, double direction_scale) {
    if (num_iterations < LG_PG_MIN_ITERATIONS || num_iterations > LG_BA_MAX_ITERATIONS) return "num_iterations must lie in [LG_PG_MIN_ITERATIONS, LG_BA_MAX_ITERATIONS]";
    if (origin < 0 || origin >= images) return "origin must name an image";
    if (baseline < -1 || baseline >= images || baseline == origin) return "baseline must be -1 or name an image other than origin";
    if (!positive(rotation_scale) || !positive(max_rotation_error) || !positive(direction_scale))
        return "rotation_scale, max_rotation_error and direction_scale must be > 0 (and finite)";
    return nullptr;
}
// lg_posegraph_solve_pcg: lg_posegraph_solve's layout without S and with the image bound LG_BA_PCG_MAX_IMAGES, then a 256-byte record of the solver; per
// pair six fp64 (w' and w' omega, or the six entries of M: 48 bytes); per image r, z, p, q, x (5 x 24 bytes), D (48), D^-1 (72) and its partials of p.q
// and r.z (2 x 8): 256 bytes.  Bytes: 512 + 116 images + 4 + 100 pairs + 256 images, every piece rounded up to 256 bytes
struct PgPcgLayout { PgLayout base; long long head, pm, r, z, p, q, x, D, Di, pq, rz, total; };
inline const char* pg_pcg_layout(long long images, long long pairs, uint32_t flags, PgPcgLayout& L) {
    if (flags & ~PG_KNOWN_FLAGS) return "undefined flag bits (the pose-graph solver defines none)";
    if (images < 2 || images > LG_BA_PCG_MAX_IMAGES) return "images must lie in [2, LG_BA_PCG_MAX_IMAGES]";
    if (pairs < 1 || pairs > PG_MAX_PAIRS) return "pairs must lie in [1, 2^20]";
    PgLayout& B = L.base;
    Bump bp;
    B.head = bp.take(256); B.rot = bp.take(images * 72); B.cen = bp.take(images * 24);
    B.level = bp.take(images * 4); B.present = bp.take(images * 4); B.acount = bp.take(images * 4); B.aoff = bp.take((images + 1) * 4); B.acur = bp.take(images * 4);
    B.pstate = bp.take(pairs * 4); B.perr = bp.take(pairs * 8); B.dir = bp.take(pairs * 24); B.adj = bp.take(pairs * 16);
    B.S = bp.used; B.total = bp.used;                       // no S
    L.head = bp.take(256); L.pm = bp.take(pairs * 48);
    L.r = bp.take(images * 24); L.z = bp.take(images * 24); L.p = bp.take(images * 24); L.q = bp.take(images * 24); L.x = bp.take(images * 24);
    L.D = bp.take(images * 48); L.Di = bp.take(images * 72); L.pq = bp.take(images * 8); L.rz = bp.take(images * 8); L.total = bp.used;
    return nullptr;
}
// the solver's own settings, refused in this order; the product counts the solver iterations the call enqueues
inline const char* pg_pcg_settings_error(long long num_iterations, long long rotation_cg_iterations, long long position_cg_iterations, double cg_tolerance) {
    if (rotation_cg_iterations < 1 || rotation_cg_iterations > LG_BA_PCG_MAX_CG_ITERATIONS)
        return "rotation_cg_iterations must lie in [1, LG_BA_PCG_MAX_CG_ITERATIONS]";
    if (position_cg_iterations < 1 || position_cg_iterations > LG_BA_PCG_MAX_CG_ITERATIONS)
        return "position_cg_iterations must lie in [1, LG_BA_PCG_MAX_CG_ITERATIONS]";
    if (!(cg_tolerance > 0.0 && cg_tolerance < 1.0)) return "cg_tolerance must lie in (0, 1)";
    if (num_iterations * (rotation_cg_iterations + position_cg_iterations) > LG_BA_PCG_MAX_SOLVER_ITERATIONS)
        return "num_iterations x (rotation_cg_iterations + position_cg_iterations) must not exceed LG_BA_PCG_MAX_SOLVER_ITERATIONS";
    return nullptr;
}
// lg_positioning_solve: a 256-byte record of the call; per image a 128-byte record (camera, rotation, held centre), its flags (4) and its centre twice in fp64
// (48); the position system with its right-hand side row, (3 images + 1) x 3 images fp64; per node its track-list entry and that entry's image (8), its ray
// (24) and its weight (8); per track five int32 (count, offset, cursor, state, reached) and fifteen fp64 (the point, Vi, g: 120 bytes)
constexpr uint32_t POS_KNOWN_FLAGS = 0u;
struct PosLayout { long long nodes, head, rec, iflag, cen, S, list, limg, ray, rho, tcnt, toff, tcur, tin, treach, X, Vinv, g, total; };
inline const char* pos_layout(long long images, long long n, long long tracks, uint32_t flags, PosLayout& L) {
    if (flags & ~POS_KNOWN_FLAGS) return "undefined flag bits (the positioner defines none)";
    if (n < 0 || n > LG_MAX_KEYPOINTS) return "n must lie in [0, LG_MAX_KEYPOINTS]";
    if (images < 2 || images > LG_BA_MAX_IMAGES) return "images must lie in [2, LG_BA_MAX_IMAGES]";
    if (images * n > LG_MAX_ROWS) return "images x n must lie in [0, LG_MAX_ROWS]";
    if (tracks < 0 || tracks > images * n / 2) return "tracks must lie in [0, images x n / 2]";
    L.nodes = images * n;
    Bump bp;
    L.head = bp.take(256); L.rec = bp.take(images * 128); L.iflag = bp.take(images * 4); L.cen = bp.take(images * 48);
    L.S = bp.take((3 * images + 1) * 3 * images * 8);
    L.list = bp.take(L.nodes * 4); L.limg = bp.take(L.nodes * 4); L.ray = bp.take(L.nodes * 24); L.rho = bp.take(L.nodes * 8);
    L.tcnt = bp.take(tracks * 4); L.toff = bp.take(tracks * 4); L.tcur = bp.take(tracks * 4); L.tin = bp.take(tracks * 4); L.treach = bp.take(tracks * 4);
    L.X = bp.take(tracks * 24); L.Vinv = bp.take(tracks * 72); L.g = bp.take(tracks * 24); L.total = bp.used;
    return nullptr;
}
inline const char* pos_settings_error(long long num_iterations, double angle_scale, double max_angle_error) {
    if (num_iterations < LG_PG_MIN_ITERATIONS || num_iterations > LG_BA_MAX_ITERATIONS) return "num_iterations must lie in [LG_PG_MIN_ITERATIONS, LG_BA_MAX_ITERATIONS]";
    if (!positive(angle_scale) || !positive(max_angle_error)) return "angle_scale and max_angle_error must be > 0 (and finite)";
    return nullptr;
}
// lg_sift_filter: two int32 rasters per image (m1 | m2 contiguous: one clear) and one flag per detection
struct SiftFilterLayout { long long m1, m2, flags, total; };
inline bool sift_filter_layout(int images, int n, int max_h, int max_w, SiftFilterLayout& L) {
    if (images < 1 || images > 65535 || n < 0 || n > (1 << 24) || max_h < 1 || max_w < 1 || (long long)max_h * max_w > 2147483647LL) return false;
    const long long raster = (long long)images * max_h * max_w * 4;
    if (raster > (1LL << 40)) return false;
    Bump bp;
    L.m1 = bp.take(raster); L.m2 = bp.take(raster); L.flags = bp.take((long long)images * n); L.total = bp.used;
    return true;
}

// ---------------------------------------------------------------- the launches of the blocked Cholesky (lg_cholesky.h) of a dim x dim system with nrhs
// right-hand sides as further rows: visit(panel, tiles_below) per panel of LG_BA_CHOLESKY_BLOCK columns, in order; tiles_below: the row tiles from the
// panel's own down to the last (the rows launch's grid)
template <class F> void for_cholesky_panels(int dim, int nrhs, F visit) {
    constexpr int NB = LG_BA_CHOLESKY_BLOCK;
    const int panels = (dim + NB - 1) / NB, tiles = (dim + nrhs + NB - 1) / NB;
    for (int p = 0; p < panels; ++p) visit(p, tiles - p);
}

// ---------------------------------------------------------------- pairs are grid.x: 2^20 x 512 threads stays below the 2^32 threads per grid axis HIP accepts,
// and a longer list is cut into launches.  launch(first pair, count) -> LG_*
constexpr int PAIRS_PER_LAUNCH = 1 << 20;
template <class F> int for_pair_launches(int pairs, F launch) {
    for (long long p0 = 0; p0 < pairs; p0 += PAIRS_PER_LAUNCH)       // (64-bit: the step past the last launch of a list near 2^31 pairs)
        if (const int rc = launch((int)p0, pairs - p0 < PAIRS_PER_LAUNCH ? (int)(pairs - p0) : PAIRS_PER_LAUNCH)) return rc;
    return LG_OK;
}

}  // namespace lg
