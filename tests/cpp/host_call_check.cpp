// Checks the host side the stateless entry points share (lightglue_amd/csrc/lg_host_call.h) without a GPU: every rule below is restated from
// include/lightglue_amd.h, then asserted over a grid — the LG_FLAG_INDEXED refusal, the workspace refusals, the keypoint-count envelope, the three workspace
// layouts (piece by piece: every piece at a 256-byte aligned offset behind the one before it, and the byte totals the entry points have always returned) and
// the cut of a pair list into launches.  Stand-alone: built and run by tests/test_host_call_cpu.py; for a sanitizer run add -fsanitize=address,undefined.
// Exit status 0 and "ok <checks>" on success, the first violated rule otherwise.
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

}  // namespace

int main() {
    pair_list_rules();
    workspace_rules();
    keypoint_rules();
    layout_rules();
    launch_rules();
    std::printf("ok %lld\n", g_checks);
    return 0;
}
