// Checks the host side the stateless entry points share (lightglue_amd/csrc/lg_host_call.h) without a GPU: every rule below is restated from
// include/lightglue_amd.h, then asserted over a grid — the LG_FLAG_INDEXED refusal, the workspace refusals, the keypoint-count envelope, the three workspace
// layouts (piece by piece: every piece at a 256-byte aligned offset behind the one before it, and the byte totals the entry points have always returned) and
// the cut of a pair list into launches, the solvers' byte totals and envelope refusals, the "> 0 and finite" test, the carving of typed pointers and the
// panel loop of the Cholesky — and the opening of a call of the three estimators (check_estimator_call): every refusal in its order, with the exact
// message, per entry point.  Stand-alone: built and run by tests/test_host_call_cpu.py; for a sanitizer run add -fsanitize=address,undefined.
// Exit status 0 and "ok <checks>" on success, the first violated rule otherwise.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../lightglue_amd/csrc/lg_host_call.h"

namespace lg {
static int g_code = 0;
static std::string g_msg;
int set_error(int code, const std::string& msg) { g_code = code; g_msg = msg; return code; }
}  // namespace lg

using namespace lg;

namespace {

long long g_checks = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { std::printf("FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n  last error: %s\n", g_msg.c_str()); std::exit(1); } } while (0)

bool says(const char* word) { return g_msg.find(word) != std::string::npos; }
long long up(long long b) { return (b + 255) / 256 * 256; }
void* at(uintptr_t a) { return reinterpret_cast<void*>(a); }

void pair_list_rules() {
    const char* stages[3] = {"lg_engine_forward", "lg_nn_match", "lg_twoview_verify"};
    for (const char* stage : stages)
        for (uint32_t flags : {0u, (uint32_t)LG_FLAG_INDEXED, (uint32_t)(LG_FLAG_INDEXED | LG_FLAG_EXT | LG_FLAG_NN_MUTUAL)})
            for (int null0 = 0; null0 < 2; ++null0)
                for (int null1 = 0; null1 < 2; ++null1)
                    for (long long images0 : {-1LL, 0LL, 1LL, 7LL})
                        for (long long images1 : {-1LL, 0LL, 1LL, 1LL << 40}) {
                            g_msg.clear();
                            const int rc = check_pair_list(stage, flags, null0 ? nullptr : at(256), null1 ? nullptr : at(512), images0, images1);
                            const bool bad = (flags & LG_FLAG_INDEXED) && (null0 || null1 || images0 < 1 || images1 < 1);
                            CHECK(rc == (bad ? LG_ERR_INVALID : LG_OK), "%s flags %u null %d %d images %lld %lld", stage, flags, null0, null1, images0, images1);
                            if (bad) CHECK(g_msg.rfind(std::string(stage) + ": ", 0) == 0 && says("LG_FLAG_INDEXED") && says("index0, index1") && says("images0"), "%s", stage);
                        }
}

void workspace_rules() {
    for (const char* stage : {"lg_nn_match", "lg_twoview_verify", "lg_sift_filter"})
        for (long long need : {0LL, 256LL, 1000LL, 1LL << 33})
            for (long long slack : {-1LL, 0LL, 1LL, 1LL << 20})
                for (uintptr_t ptr : {(uintptr_t)0, (uintptr_t)256, (uintptr_t)(1 << 20), (uintptr_t)((1 << 20) + 64), (uintptr_t)((1 << 20) + 128), (uintptr_t)((1 << 20) + 255)})
                    for (int null_if_empty = 0; null_if_empty < 2; ++null_if_empty) {
                        const long long bytes = need + slack;
                        g_msg.clear();
                        const int rc = check_workspace(stage, "the_size_function", at(ptr), bytes, need, null_if_empty != 0);
                        const bool null_bad = !ptr && !(null_if_empty && need == 0), small = bytes < need, skew = ptr % 256 != 0;
                        CHECK(rc == (null_bad || small || skew ? LG_ERR_INVALID : LG_OK), "%s need %lld bytes %lld ptr %llu", stage, need, bytes, (unsigned long long)ptr);
                        if (rc) CHECK(g_msg.rfind(std::string(stage) + ": ", 0) == 0, "%s", stage);
                        // one reason per message, in this order
                        if (null_bad) CHECK(says("null workspace"), "null");
                        else if (small) CHECK(says(("workspace holds " + std::to_string(bytes) + " bytes, the_size_function = " + std::to_string(need)).c_str()), "small");
                        else if (skew) CHECK(says("256-byte aligned"), "skew");
                    }
}

void keypoint_rules() {
    for (int n0 : {-1, 0, 1, LG_MAX_KEYPOINTS, LG_MAX_KEYPOINTS + 1})
        for (int n1 : {-1, 0, LG_MAX_KEYPOINTS, LG_MAX_KEYPOINTS + 1}) {
            const char* why = keypoint_counts_error(n0, n1);
            const bool bad = n0 < 0 || n1 < 0 || n0 > LG_MAX_KEYPOINTS || n1 > LG_MAX_KEYPOINTS;
            CHECK((why != nullptr) == bad, "n0 %d n1 %d", n0, n1);
            if (why) CHECK(std::strstr(why, "LG_MAX_KEYPOINTS") != nullptr, "%s", why);
        }
    CHECK(!keypoint_counts_error(5) && keypoint_counts_error(-5), "one count");
}

// pieces in order: each starts where the one before it ends, rounded up to 256 bytes; the total is the end of the last
void check_pieces(const std::vector<long long>& offsets, const std::vector<long long>& sizes, long long total, const char* what) {
    long long expect = 0;
    for (size_t i = 0; i < sizes.size(); ++i) {
        CHECK(offsets[i] == expect && offsets[i] % 256 == 0, "%s piece %zu at %lld, expected %lld", what, i, offsets[i], expect);
        expect += up(sizes[i]);
    }
    CHECK(total == expect, "%s total %lld, expected %lld", what, total, expect);
}

void layout_rules() {
    const uint32_t nnf = LG_FLAG_INDEXED | LG_FLAG_NN_MUTUAL | LG_FLAG_DESC0_U8 | LG_FLAG_DESC1_F16 | LG_FLAG_ROOTSIFT0;
    struct { long long k0, k1; int n0, n1, dim; } nn[] = {{0, 0, 0, 0, 16}, {1, 1, 1, 1, 16}, {4, 4, 64, 64, 128}, {3, 5, 130, 70, 48}, {16, 16, 2048, 2048, 256},
                                                          {1000000, 1000000, 0, 0, 16}, {262143, 1, 8192, 8192, 256}};
    for (const auto& c : nn) {
        NnLayout L;
        CHECK(nn_layout(c.k0, c.k1, c.n0, c.n1, c.dim, nnf, L) == nullptr, "nn %lld %lld %d %d %d", c.k0, c.k1, c.n0, c.n1, c.dim);
        CHECK(L.rows0 == c.k0 * c.n0 && L.rows1 == c.k1 * c.n1, "nn rows");
        check_pieces({L.ws0, L.ws1, L.touched0, L.touched1}, {L.rows0 * c.dim * 4, L.rows1 * c.dim * 4, c.k0, c.k1}, L.total, "nn");
    }
    NnLayout L;
    CHECK(nn_layout(16, 16, 2048, 2048, 256, LG_FLAG_INDEXED, L) == nullptr && L.total == 67109376LL, "nn total %lld", L.total);
    CHECK(nn_layout(4, 4, 64, 64, 128, nnf, L) == nullptr && L.total == 2 * 131072 + 512, "nn total %lld", L.total);
    CHECK(nn_layout(1, 1, 64, 64, 20, 0, L) && nn_layout(1, 1, 64, 64, 272, 0, L) && nn_layout(1, 1, 64, 64, 0, 0, L), "nn dim");
    CHECK(nn_layout(1, 1, 8193, 64, 128, 0, L) && nn_layout(1, 1, 64, -1, 128, 0, L) && nn_layout(-1, 1, 64, 64, 128, 0, L), "nn counts");
    CHECK(nn_layout(1, 1, 64, 64, 128, 4096, L) && nn_layout(1, 1, 64, 64, 128, LG_FLAG_DESC0_F16 | LG_FLAG_DESC0_U8, L), "nn flags");
    CHECK(nn_layout(262145, 1, 8192, 64, 128, 0, L) != nullptr, "nn: more than 2^31 - 1 rows");

    const uint32_t H = LG_TWOVIEW_HOMOGRAPHY, F = LG_TWOVIEW_FUNDAMENTAL;
    struct { long long pairs; int n0; } tv[] = {{0, 0}, {1, 0}, {1, 1}, {7, 1100}, {120, 2048}, {100000, 8192}, {0x7FFFFFFFLL, 8192}};
    for (const auto& c : tv) {
        TvLayout T;
        CHECK(tv_layout(c.pairs, c.n0, F | LG_TWOVIEW_REFINE | LG_FLAG_INDEXED, T) == nullptr, "tv %lld %d", c.pairs, c.n0);
        check_pieces({T.head, T.corr, T.rows}, {c.pairs * 32, c.pairs * c.n0 * 16, c.pairs * c.n0 * 4}, T.total, "tv");
    }
    TvLayout T;
    CHECK(tv_layout(120, 2048, F, T) == nullptr && T.total == 4919040LL, "tv total %lld", T.total);
    CHECK(tv_layout(7, 1100, H, T) == nullptr && T.total == 256 + 123392 + 30976, "tv total %lld", T.total);
    CHECK(tv_layout(-1, 10, H, T) && tv_layout(1LL << 31, 10, H, T) && tv_layout(1, 8193, F, T) && tv_layout(1, -1, F, T), "tv envelope");
    CHECK(tv_layout(1, 10, H | F, T) && tv_layout(1, 10, LG_TWOVIEW_REFINE, T) && tv_layout(1, 10, H | 1u, T) && tv_layout(1, 10, H | LG_FLAG_NN_MUTUAL, T), "tv flags");

    struct { int images, n, h, w; } sf[] = {{1, 0, 1, 1}, {2, 64, 48, 64}, {3, 1000, 480, 640}, {65535, 1 << 24, 1, 1}, {256, 5, 1024, 1024}};
    for (const auto& c : sf) {
        SiftFilterLayout S;
        CHECK(sift_filter_layout(c.images, c.n, c.h, c.w, S), "sift %d %d %d %d", c.images, c.n, c.h, c.w);
        const long long raster = (long long)c.images * c.h * c.w * 4;
        check_pieces({S.m1, S.m2, S.flags}, {raster, raster, (long long)c.images * c.n}, S.total, "sift");
        CHECK(S.m2 == S.m1 + up(raster) && S.flags == S.m2 + up(raster), "sift: the two rasters are contiguous (one clear)");
    }
    SiftFilterLayout S;
    CHECK(sift_filter_layout(2, 64, 48, 64, S) && S.total == 49408, "sift total %lld", S.total);
    CHECK(!sift_filter_layout(0, 1, 1, 1, S) && !sift_filter_layout(65536, 1, 1, 1, S) && !sift_filter_layout(1, -1, 1, 1, S) && !sift_filter_layout(1, (1 << 24) + 1, 1, 1, S), "sift counts");
    CHECK(!sift_filter_layout(1, 1, 0, 1, S) && !sift_filter_layout(1, 1, 65536, 65536, S) && !sift_filter_layout(65535, 1, 46340, 46340, S), "sift rasters");
}

// The solvers' layouts (lg_bundle_adjust, _robust, _focal, lg_posegraph_solve, lg_positioning_solve): the byte totals the entry points returned before the
// solver steps were written once (computed from that commit's header), at (images, n, tracks) = (6, 96, 50) and (256, 16, 900), pairs = 15 and 900; and the
// envelope's refusals
void solver_layout_rules() {
    struct { long long images, n, tracks, pairs, ba, robust, focal, pg, pos; } sizes[] = {
        {6, 96, 50, 15, 26624, 26880, 31232, 6400, 35328}, {256, 16, 900, 900, 19141120, 19144960, 25981184, 4802560, 5062656}};
    BaLayout B; BaRobustLayout R; BaFocalLayout F; PgLayout G; PosLayout Q;
    for (const auto& c : sizes) {
        CHECK(ba_layout(c.images, c.n, c.tracks, 0, B) == nullptr && B.total == c.ba, "ba total %lld", B.total);
        CHECK(ba_robust_layout(c.images, c.n, c.tracks, 0, R) == nullptr && R.total == c.robust && R.tmov == c.ba, "robust total %lld", R.total);
        CHECK(ba_focal_layout(c.images, c.n, c.tracks, 0, F) == nullptr && F.total == c.focal, "focal total %lld", F.total);
        CHECK(pg_layout(c.images, c.pairs, 0, G) == nullptr && G.total == c.pg, "pg total %lld", G.total);
        CHECK(pos_layout(c.images, c.n, c.tracks, 0, Q) == nullptr && Q.total == c.pos, "pos total %lld", Q.total);
    }
    const auto says_why = [](const char* why, const char* word) { return why && std::strstr(why, word); };
    // images = 0, images = 257, tracks > images x n / 2, an undefined flag bit
    CHECK(says_why(ba_layout(0, 96, 50, 0, B), "images must lie in [1, LG_BA_MAX_IMAGES]") && says_why(ba_layout(257, 16, 900, 0, B), "images must lie in [1, LG_BA_MAX_IMAGES]"), "ba images");
    CHECK(says_why(ba_layout(6, 96, 289, 0, B), "tracks must lie in") && !ba_layout(6, 96, 288, 0, B) && says_why(ba_layout(6, 96, 50, 1u, B), "undefined flag bits"), "ba tracks, flags");
    CHECK(says_why(ba_robust_layout(0, 96, 50, 0, R), "images must lie in") && says_why(ba_robust_layout(257, 16, 900, 0, R), "images must lie in") &&
          says_why(ba_robust_layout(6, 96, 289, 0, R), "tracks must lie in") && says_why(ba_robust_layout(6, 96, 50, 1u << 31, R), "undefined flag bits"), "robust envelope");
    CHECK(says_why(ba_focal_layout(0, 96, 50, 0, F), "images must lie in") && says_why(ba_focal_layout(257, 16, 900, 0, F), "images must lie in") &&
          says_why(ba_focal_layout(6, 96, 289, 0, F), "tracks must lie in") && says_why(ba_focal_layout(6, 96, 50, 2u, F), "undefined flag bits"), "focal envelope");
    CHECK(says_why(pos_layout(0, 96, 50, 0, Q), "images must lie in [2, LG_BA_MAX_IMAGES]") && says_why(pos_layout(257, 16, 900, 0, Q), "images must lie in [2, LG_BA_MAX_IMAGES]") &&
          says_why(pos_layout(6, 96, 289, 0, Q), "tracks must lie in") && !pos_layout(6, 96, 288, 0, Q) && says_why(pos_layout(6, 96, 50, 1u, Q), "undefined flag bits"), "pos envelope");
    CHECK(says_why(pg_layout(0, 15, 0, G), "images must lie in [2, LG_BA_MAX_IMAGES]") && says_why(pg_layout(257, 900, 0, G), "images must lie in [2, LG_BA_MAX_IMAGES]") &&
          says_why(pg_layout(6, 15, 1u, G), "undefined flag bits"), "pg envelope");
    // the "> 0 (and finite)" test of the settings
    CHECK(positive(1e-300) && positive(1.7976931348623157e308) && !positive(0.0) && !positive(-1.0) && !positive(HUGE_VAL) && !positive(std::nan("")), "positive");
    CHECK(!pos_settings_error(12, 1.0, 2.0) && pos_settings_error(12, 0.0, 2.0) && pg_settings_error(6, 12, 0, -1, 1.0, HUGE_VAL, 1.0) &&
          ba_robust_settings_error(LG_BA_LOSS_HUBER, std::nan(""), 0, 4.0) && !ba_robust_settings_error(LG_BA_LOSS_SQUARED, 0.0, 0, 0.0), "settings");
    // typed pointers at a layout's offsets
    alignas(8) char ws[64];
    const Carved w(ws);
    CHECK((char*)w.ints(8) == ws + 8 && (char*)w.f64(16) == ws + 16 && (char*)w.as<long long>(24) == ws + 24, "carving");
}

// The panel loop of the blocked Cholesky: per panel of 48 columns, the panel and the row tiles from its own down to the last (with the right-hand sides' rows)
void cholesky_panel_rules() {
    struct { int dim, nrhs, panels, first; } cases[] = {{48, 1, 1, 2}, {49, 1, 2, 2}, {768, 3, 16, 17}, {1, 1, 1, 1}, {47, 1, 1, 1}, {96, 1, 2, 3}, {1792, 1, 38, 38}};
    for (const auto& c : cases) {
        int next = 0;
        for_cholesky_panels(c.dim, c.nrhs, [&](int panel, int tiles_below) {
            CHECK(panel == next && tiles_below == c.first - panel && tiles_below >= 1, "dim %d nrhs %d: panel %d with %d tiles", c.dim, c.nrhs, panel, tiles_below);
            ++next;
        });
        CHECK(next == c.panels, "dim %d: %d panels", c.dim, next);
    }
    std::vector<int> seen;
    for_cholesky_panels(49, 1, [&](int p, int below) { seen.push_back(p); seen.push_back(below); });
    CHECK(seen == std::vector<int>({0, 2, 1, 1}), "dim 49: (0, 2), (1, 1)");
    seen.clear();
    for_cholesky_panels(48, 1, [&](int p, int below) { seen.push_back(p); seen.push_back(below); });
    CHECK(seen == std::vector<int>({0, 2}), "dim 48: (0, 2)");
    seen.clear();
    for_cholesky_panels(768, 3, [&](int p, int below) { seen.push_back(p); seen.push_back(below); });
    CHECK(seen.size() == 32 && seen[0] == 0 && seen[1] == 17 && seen[30] == 15 && seen[31] == 2, "dim 768, 3 right-hand sides: (0, 17) ... (15, 2)");
}

void launch_rules() {
    for (int pairs : {0, 1, PAIRS_PER_LAUNCH - 1, PAIRS_PER_LAUNCH, PAIRS_PER_LAUNCH + 1, 3 * PAIRS_PER_LAUNCH + 5, 0x7FFFFFFF}) {
        long long next = 0, calls = 0;
        const int rc = for_pair_launches(pairs, [&](int p0, int count) -> int {
            CHECK(p0 == next && count >= 1 && count <= PAIRS_PER_LAUNCH, "launch %d + %d of %d", p0, count, pairs);
            next += count; ++calls;
            return LG_OK;
        });
        CHECK(rc == LG_OK && next == pairs && calls == ((long long)pairs + PAIRS_PER_LAUNCH - 1) / PAIRS_PER_LAUNCH, "%d pairs: %lld launches", pairs, calls);
    }
    int calls = 0;
    CHECK(for_pair_launches(3 * PAIRS_PER_LAUNCH, [&](int, int) -> int { return ++calls == 2 ? LG_ERR_HIP : LG_OK; }) == LG_ERR_HIP && calls == 2, "a failed launch ends the list");
}

// The opening of a call of the three estimators (check_estimator_call): the refusals in their order, code and exact message (the texts are those the three
// entry points have always set).  A call that violates refusal i AND every later one must be answered with refusal i, a valid call with LG_OK and the layout.
char g_store[64];                                        // something non-null for every pointer field; never read
void* const P = g_store;
template <class T> T* ptr() { return reinterpret_cast<T*>(P); }

template <class IO> void common_fields(IO& io, uint32_t flags) {
    io.pairs = 3; io.n0 = 40; io.n1 = 50; io.images0 = 2; io.images1 = 2; io.flags = flags | LG_FLAG_INDEXED; io.threshold = 2.f; io.num_hypotheses = 512;
    io.index0 = ptr<const int32_t>(); io.index1 = ptr<const int32_t>(); io.workspace = at(1 << 20);
}
// break(io, i): violate refusal i (1 = the layout's ... 7 = the workspace; 0, null io, is the caller's)
template <class IO> void break_common(IO& io, int i) {
    if (i == 1) io.pairs = -1;
    if (i == 2) io.n1 = LG_MAX_KEYPOINTS + 1;
    if (i == 3) io.num_hypotheses = 300;
    if (i == 4) io.threshold = 0.f;
    if (i == 5) io.images1 = 0;
    if (i == 7) io.workspace = nullptr;
}
lg_twoview_io valid_twoview() {
    lg_twoview_io io{};
    common_fields(io, LG_TWOVIEW_FUNDAMENTAL | LG_TWOVIEW_REFINE);
    io.kpts0 = io.kpts1 = ptr<const float>(); io.matches0 = ptr<const int64_t>(); io.models = ptr<float>(); io.inliers0 = ptr<uint8_t>();
    io.num_inliers = ptr<int32_t>(); io.status = ptr<int32_t>();
    return io;
}
lg_relpose_io valid_relpose() {
    lg_relpose_io io{};
    common_fields(io, LG_RELPOSE_REFINE);
    io.kpts0 = io.kpts1 = io.cameras0 = io.cameras1 = ptr<const float>(); io.matches0 = ptr<const int64_t>();
    io.rotations = io.translations = io.essentials = io.models = ptr<float>(); io.inliers0 = ptr<uint8_t>();
    io.num_inliers = io.num_in_front = io.status = ptr<int32_t>();
    return io;
}
lg_abspose_io valid_abspose() {
    lg_abspose_io io{};
    common_fields(io, LG_ABSPOSE_REFINE);
    io.kpts0 = io.points3d1 = io.cameras0 = ptr<const float>(); io.matches0 = ptr<const int64_t>();
    io.rotations = io.translations = ptr<float>(); io.inliers0 = ptr<uint8_t>(); io.num_inliers = io.pair_num_inliers = io.status = ptr<int32_t>();
    return io;
}

// budget_first: the pose estimators' layouts depend on the budget and refuse it themselves, before n1; the verifier refuses it behind n1
template <class IO, class Layout, class Break6>
void walk_estimator(const char* stage, const char* size_function, IO (*valid)(), long long total, bool budget_first, const char* pointers, Break6 break6) {
    const std::string s = std::string(stage) + ": ";
    const std::string expect[8] = {
        s + "null io", s + "the pair count must lie in [0, 2^31 - 1]", s + "n0, n1 must lie in [0, LG_MAX_KEYPOINTS]", s + "num_hypotheses must be a multiple of 256 in [256, 65536]",
        s + "threshold must be > 0 (and finite)", s + "LG_FLAG_INDEXED needs index0, index1 and images0, images1 >= 1", s + pointers, s + "null workspace"};
    Layout L;
    IO io = valid();
    io.workspace_bytes = total;
    g_msg.clear();
    CHECK(check_estimator_call(stage, size_function, &io, L) == LG_OK && g_msg.empty() && L.total == total, "%s: a valid call, total %lld", stage, L.total);
    CHECK(check_estimator_call(stage, size_function, static_cast<const IO*>(nullptr), L) == LG_ERR_INVALID && g_msg == expect[0], "%s: null io", stage);
    const int order[7] = {1, budget_first ? 3 : 2, budget_first ? 2 : 3, 4, 5, 6, 7};
    for (int first = 0; first < 7; ++first) {
        io = valid();
        io.workspace_bytes = total;
        for (int k = first; k < 7; ++k) { break_common(io, order[k]); if (order[k] == 6) break6(io); }
        g_msg.clear();
        const std::string& want = expect[order[first]];
        CHECK(check_estimator_call(stage, size_function, &io, L) == LG_ERR_INVALID && g_msg == want, "%s: refusal %d, expected \"%s\"", stage, order[first], want.c_str());
    }
    // the workspace's other two refusals
    io = valid();
    io.workspace_bytes = total - 1;
    CHECK(check_estimator_call(stage, size_function, &io, L) == LG_ERR_INVALID &&
          g_msg == s + "the workspace holds " + std::to_string(total - 1) + " bytes, " + size_function + " = " + std::to_string(total), "%s: small workspace", stage);
    io.workspace_bytes = total; io.workspace = at((1 << 20) + 64);
    CHECK(check_estimator_call(stage, size_function, &io, L) == LG_ERR_INVALID && g_msg == s + "the workspace must be 256-byte aligned", "%s: skewed workspace", stage);
    // the threshold's other side, and the layout's further refusals come before n1
    io = valid(); io.workspace_bytes = total; io.threshold = 4.0e18f;
    CHECK(check_estimator_call(stage, size_function, &io, L) == LG_ERR_INVALID && g_msg == expect[4], "%s: a threshold beyond 3e18", stage);
    io = valid(); io.workspace_bytes = total; io.n0 = -1; io.n1 = -1;
    CHECK(check_estimator_call(stage, size_function, &io, L) == LG_ERR_INVALID && g_msg == expect[2], "%s: n0", stage);
}

void estimator_call_rules() {
    const long long rows = 3 * 40;
    walk_estimator<lg_twoview_io, TvLayout>("lg_twoview_verify", "lg_twoview_workspace_bytes", valid_twoview, up(3 * 32) + up(rows * 16) + up(rows * 4), false,
        "null pointer among kpts0, kpts1, matches0, models_in, models, inliers0, num_inliers, status", [](lg_twoview_io& io) { io.status = nullptr; });
    walk_estimator<lg_relpose_io, RpLayout>("lg_relpose_estimate", "lg_relpose_workspace_bytes", valid_relpose,
        up(3 * 32) + up(3 * 48) + up(rows * 16) + up(rows * 4) + up(3LL * 512 * LG_RELPOSE_ROOTS * 36), true,
        "null pointer among kpts0, kpts1, matches0, cameras0, cameras1, rotations, translations, essentials, models, inliers0, num_inliers, num_in_front, status",
        [](lg_relpose_io& io) { io.cameras1 = nullptr; });
    walk_estimator<lg_abspose_io, ApLayout>("lg_abspose_estimate", "lg_abspose_workspace_bytes", valid_abspose, up(3 * 64) + up(rows * 16) + up(rows * 8) + up(rows * 4), true,
        "null pointer among kpts0, points3d1, matches0, cameras0, poses_in (LG_ABSPOSE_GIVEN_POSES), rotations, translations, num_inliers, inliers0, pair_num_inliers, status",
        [](lg_abspose_io& io) { io.points3d1 = nullptr; });
    // the refusals one entry point has alone, each at its place
    TvLayout T; RpLayout R; ApLayout A;
    lg_twoview_io tv = valid_twoview();
    tv.workspace_bytes = 1 << 20; tv.flags |= LG_TWOVIEW_HOMOGRAPHY; tv.n1 = -1;
    CHECK(check_estimator_call("lg_twoview_verify", "f", &tv, T) && g_msg == "lg_twoview_verify: exactly one of LG_TWOVIEW_HOMOGRAPHY and LG_TWOVIEW_FUNDAMENTAL must be set", "tv kinds");
    tv = valid_twoview(); tv.workspace_bytes = 1 << 20; tv.flags |= 1u << 30;
    CHECK(check_estimator_call("lg_twoview_verify", "f", &tv, T) && g_msg == "lg_twoview_verify: undefined flag bits (the verifier reads LG_FLAG_INDEXED and the LG_TWOVIEW_* bits)", "tv bits");
    tv = valid_twoview(); tv.workspace_bytes = 1 << 20; tv.flags |= LG_TWOVIEW_GIVEN_MODELS;
    CHECK(check_estimator_call("lg_twoview_verify", "f", &tv, T) && g_msg == "lg_twoview_verify: null pointer among kpts0, kpts1, matches0, models_in, models, inliers0, num_inliers, status", "tv models_in");
    tv = valid_twoview(); tv.workspace_bytes = 1 << 20; tv.n1 = -1; tv.num_hypotheses = 0;          // the verifier's budget is refused behind n1 ...
    CHECK(check_estimator_call("lg_twoview_verify", "f", &tv, T) && g_msg == "lg_twoview_verify: n0, n1 must lie in [0, LG_MAX_KEYPOINTS]", "tv: n1 before the budget");
    lg_relpose_io rp = valid_relpose();
    rp.workspace_bytes = 1 << 30; rp.n1 = -1; rp.num_hypotheses = 0;                                 // ... the pose estimators' with the layout, before it
    CHECK(check_estimator_call("lg_relpose_estimate", "f", &rp, R) && g_msg == "lg_relpose_estimate: num_hypotheses must be a multiple of 256 in [256, 65536]", "rp: the budget before n1");
    rp = valid_relpose(); rp.workspace_bytes = 1 << 30; rp.flags |= LG_TWOVIEW_HOMOGRAPHY;
    CHECK(check_estimator_call("lg_relpose_estimate", "f", &rp, R) && g_msg == "lg_relpose_estimate: undefined flag bits (the pose estimator reads LG_FLAG_INDEXED and LG_RELPOSE_REFINE)", "rp bits");
    lg_abspose_io ap = valid_abspose();
    ap.workspace_bytes = 1 << 20; ap.n1 = -1; ap.num_hypotheses = 65536 + 256;
    CHECK(check_estimator_call("lg_abspose_estimate", "f", &ap, A) && g_msg == "lg_abspose_estimate: num_hypotheses must be a multiple of 256 in [256, 65536]", "ap: the budget before n1");
    ap = valid_abspose(); ap.workspace_bytes = 1 << 20; ap.flags |= 1u << 30;
    CHECK(check_estimator_call("lg_abspose_estimate", "f", &ap, A) && g_msg == "lg_abspose_estimate: undefined flag bits (the absolute-pose estimator reads LG_FLAG_INDEXED and the LG_ABSPOSE_* bits)", "ap bits");
    ap = valid_abspose(); ap.workspace_bytes = 1 << 20; ap.flags |= LG_ABSPOSE_GROUPED; ap.pairs = LG_MAX_ROWS / 40 + 1;
    CHECK(check_estimator_call("lg_abspose_estimate", "f", &ap, A) && g_msg == "lg_abspose_estimate: with LG_ABSPOSE_GROUPED pairs x n0 must not exceed LG_MAX_ROWS", "ap grouped rows");
    ap = valid_abspose(); ap.workspace_bytes = 1 << 20; ap.flags |= LG_ABSPOSE_GIVEN_POSES | LG_ABSPOSE_GROUPED;
    CHECK(check_estimator_call("lg_abspose_estimate", "f", &ap, A) && g_msg == "lg_abspose_estimate: null pointer among kpts0, points3d1, matches0, cameras0, poses_in (LG_ABSPOSE_GIVEN_POSES), "
          "rotations, translations, num_inliers, inliers0, pair_num_inliers, status", "ap poses_in");
    ap.poses_in = ptr<const float>();
    CHECK(check_estimator_call("lg_abspose_estimate", "f", &ap, A) && g_msg == "lg_abspose_estimate: null pointer: LG_ABSPOSE_GROUPED needs group_offsets and group_pairs", "ap groups");
    ap.group_offsets = ap.group_pairs = ptr<const int32_t>(); ap.groups = 4; ap.workspace = nullptr;
    CHECK(check_estimator_call("lg_abspose_estimate", "f", &ap, A) && g_msg == "lg_abspose_estimate: with LG_ABSPOSE_GROUPED groups must lie in [1, pairs]", "ap group count");
    ap.groups = 3;
    CHECK(check_estimator_call("lg_abspose_estimate", "f", &ap, A) && g_msg == "lg_abspose_estimate: null workspace", "ap: the workspace last");
}

}  // namespace

int main() {
    estimator_call_rules();
    pair_list_rules();
    workspace_rules();
    keypoint_rules();
    layout_rules();
    solver_layout_rules();
    cholesky_panel_rules();
    launch_rules();
    std::printf("ok %lld\n", g_checks);
    return 0;
}
