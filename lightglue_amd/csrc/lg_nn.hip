// lightglue_amd — the weight-free matcher: (mutual) nearest neighbour over feature stores, with Lowe's ratio test and a distance threshold (lg_nn_match; the
// definition is in include/lightglue_amd.h).  No engine, no weights, and the similarity matrix is never written to memory.  Three kinds of launch per call:
//   nn_mark / nn_prep   every descriptor row of the images the pair list touches -> one L2-normalised fp32 row in the caller's workspace (widened from its
//                       storage format, RootSIFT first where the side asks for it): once per store row, however many pairs read it;
//   nn_kernel           one direction of every pair: a workgroup keeps NN_ROWS rows of side A as the MFMA A operand in registers, streams the rows of side B
//                       through LDS in tiles of NN_TILE, and keeps (best, its index, second best) per row in registers.  Launched twice, sides swapped: both
//                       passes multiply the same fp32 operands in the same k order, so sim[i][j] is the same fp32 number in both and nothing depends on an order;
//   nn_outputs          mutual check, scores, the sorted match list and its length, the reference dtypes (int64 indices) — one workgroup per pair.
// What a pair reads is lg_common.h's: PairIndex / pair_images (the swapped direction passes the pair list swapped), live_rows, and compact_slot for the match list.
// The refusals, the workspace layout (NnLayout) and the cut of the pair list into launches are lg_host_call.h's.
#include <string>

#include "lg_host_call.h"
#include "lg_side.h"
#include "../../include/lightglue_amd.h"

namespace lg {

constexpr int NN_WAVES = 8, NN_THREADS = NN_WAVES * 64;
constexpr int NN_ROWS = LG_NN_ROWS_PER_WORKGROUP;      // 16 rows per wave
constexpr int NN_TILE = LG_NN_TILE;                    // side-B rows per LDS tile: four 16-column MFMA tiles with independent accumulators
static_assert(NN_ROWS == NN_WAVES * 16 && NN_TILE == 64, "the kernel below is written for 8 waves of 16 rows and 4 column tiles");

// ------------------------------------------------------------------ which images does the pair list read
struct NnMarkArgs { const int* index; int pairs, images; unsigned char* touched; };
__global__ __launch_bounds__(256) void nn_mark_kernel(NnMarkArgs a) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.pairs) return;
    const int k = a.index[p];
    if ((unsigned)k < (unsigned)a.images) a.touched[k] = 1;       // (every writer stores the same byte)
}

// ------------------------------------------------------------------ prep: one wave per store row, 4 rows per workgroup
// dst row = x / max(|x|_2, 1e-12) in fp32, x the widened (and RootSIFT'd) row; lane l holds x[4l .. 4l + 3].  Inside every block of 16 values the row is stored
// TRANSPOSED as 4 x 4 (value 4a + b at 4b + a): the 16 bytes a lane of nn_kernel reads at slot g of block c are then the values k = 16c + g, 16c + 4 + g,
// 16c + 8 + g, 16c + 12 + g — one per MFMA — and MFMA e of the block multiplies k = 16c + 4e .. 16c + 4e + 3: the contraction runs over k ascending.
struct NnPrepArgs { const void* src; int kind, rootsift; const int* num; const unsigned char* touched; long long rows; int n, dim; float* dst; };
__global__ __launch_bounds__(256) void nn_prep_kernel(NnPrepArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + wave;
    if (r >= a.rows) return;                       // uniform per wave, like the two tests below
    const long long k = r / a.n;
    const int i = (int)(r - k * a.n);
    if (a.touched && !a.touched[k]) return;
    if (i >= live_rows(a.num, (int)k, a.n)) return; // rows beyond num_keypoints are never read: whatever they hold stays out of the workspace
    const bool own = lane * 4 < a.dim;
    f32x4 x = own ? load_desc4(a.src, a.kind, r * a.dim + lane * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.rootsift) x = rootsift_row(x, lane, a.dim);
    const float sq = fmaf(x[3], x[3], fmaf(x[2], x[2], fmaf(x[1], x[1], x[0] * x[0])));
    const float nrm = fmaxf(sqrtf(wave_sum(own ? sq : 0.f)), 1e-12f);
    if (!own) return;
    float* d = a.dst + r * a.dim + (lane >> 2) * 16 + (lane & 3);
#pragma unroll
    for (int b = 0; b < 4; ++b) d[4 * b] = x[b] / nrm;
}

// ------------------------------------------------------------------ one direction of every pair
struct NnArgs {
    const float* rowsA; const float* rowsB;      // normalised rows [imagesA][nA][dim], [imagesB][nB][dim] (nn_prep_kernel's layout)
    const int* numA; const int* numB;            // live rows per image or nullptr
    PairIndex px;                                // index0 / images0 belong to side A of THIS launch (the second one passes the pair list swapped)
    int nA, nB, dim, pair0;
    float ratio2, dist2;                         // squared thresholds, <= 0: off
    int* raw; float* sim;                        // [pairs][nA]: nearest neighbour after the tests (-1: none / rejected) and its similarity
};

struct NnBest { float s1, s2; int j1; };
// fold candidate b into a: larger similarity first, on equal similarities the lower index.  Symmetric: both lanes of an exchange end with the same triple.
__device__ __forceinline__ void nn_merge(NnBest& a, const NnBest& b) {
    const bool b_wins = b.s1 > a.s1 || (b.s1 == a.s1 && b.j1 < a.j1);
    const float second = b_wins ? fmaxf(a.s1, b.s2) : fmaxf(a.s2, b.s1);
    if (b_wins) { a.s1 = b.s1; a.j1 = b.j1; }
    a.s2 = second;
}

template <int CMAX>       // 16-value blocks of a row the A registers can hold: dim <= 16 * CMAX
__global__ __launch_bounds__(NN_THREADS) void nn_kernel(NnArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nn_lds[];
    const int pair = a.pair0 + blockIdx.x, row0 = blockIdx.y * NN_ROWS;
    const PairImages src = pair_images(a.px, pair);
    if (!src.ok) return;                                         // everything up to the tile loop is uniform per workgroup
    const int ia = src.i0, ib = src.i1, na = live_rows(a.numA, ia, a.nA), nb = live_rows(a.numB, ib, a.nB);
    if (row0 >= na) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, g = lane >> 4;
    const int nch = a.dim >> 4, slots = a.dim >> 2;              // 16-value blocks / 16-byte slots of a row
    const int ldb = a.dim * 4 + 16;                              // LDS row pitch in bytes: an ODD number of 16-byte slots, so the 16 rows a 16-lane group of
                                                                 // ds_read_b128 touches at one slot lie in 16 different bank groups (dim % 16 == 0)
    // the A operand of this wave for its whole life: row (wave, col), slot g of every block
    f32x4 A[CMAX];
    {
        const int arow = row0 + wave * 16 + col;
        const float* ap = a.rowsA + ((long long)ia * a.nA + min(arow, na - 1)) * a.dim + g * 4;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) A[c] = c < nch && arow < na ? *reinterpret_cast<const f32x4*>(ap + c * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // C layout: acc[t][r] of this lane is sim[row 4g + r of the wave][column 16t + col of the tile]
    float s1[4], s2[4];       // per row: the best similarity so far, the second best, and the best's column
    int j1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { s1[r] = s2[r] = -INFINITY; j1[r] = INT_MAX; }
    const float* bsrc = a.rowsB + (long long)ib * a.nB * a.dim;
    for (int j0 = 0; j0 < nb; j0 += NN_TILE) {
        if (j0) __syncthreads();                                 // every wave has read the previous tile
        for (int s = tid; s < NN_TILE * slots; s += NN_THREADS) {
            const int r = s / slots, q = s - r * slots, j = j0 + r;
            const f32x4 v = j < nb ? *reinterpret_cast<const f32x4*>(bsrc + (long long)j * a.dim + q * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(nn_lds + r * ldb + q * 16) = v;
        }
        __syncthreads();
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            if (c >= nch) continue;       // (uniform.  Not `break`: hipcc then gives up unrolling and A[] lives in scratch)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(nn_lds + (t * 16 + col) * ldb + c * 64 + g * 16);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[c][0], b[0], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[c][1], b[1], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[c][2], b[2], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[c][3], b[3], acc[t], 0, 0, 0);
            }
        }
        // columns arrive in ascending order per lane, so `>` alone keeps the lowest index among equal values; a NaN never wins a comparison
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = j0 + t * 16 + col;
            if (j < nb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[t][r];
                    const bool first = v > s1[r];
                    s2[r] = first ? s1[r] : v > s2[r] ? v : s2[r];
                    j1[r] = first ? j : j1[r];
                    s1[r] = first ? v : s1[r];
                }
            }
        }
    }
    // the 16 lanes that share g hold the 16 column classes of the same four rows
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        NnBest b{s1[r], s2[r], j1[r]};
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) nn_merge(b, NnBest{__shfl_xor(b.s1, o, 64), __shfl_xor(b.s2, o, 64), __shfl_xor(b.j1, o, 64)});
        const int i = row0 + wave * 16 + 4 * g + r;
        if (col == r && i < na) {                                // lane col = r writes row 4g + r
            const bool found = b.j1 < nb;
            const float d1 = fmaxf(2.f * (1.f - b.s1), 0.f), d2 = fmaxf(2.f * (1.f - b.s2), 0.f);     // no second neighbour: s2 = -inf, d2 = +inf, the ratio test passes
            const bool keep = found && (a.ratio2 <= 0.f || d1 <= a.ratio2 * d2) && (a.dist2 <= 0.f || d1 <= a.dist2);
            const long long at = (long long)pair * a.nA + i;
            a.raw[at] = keep ? b.j1 : -1;
            a.sim[at] = found ? b.s1 : 0.f;
        }
    }
}

// ------------------------------------------------------------------ outputs: one workgroup per pair
struct NnOutArgs {
    PairIndex px; const int* num0; const int* num1;
    int n0, n1, pair0, mutual, list_rows;
    const int* raw0; const int* raw1;            // [pairs][n0], [pairs][n1] (nn_kernel)
    long long* m0; long long* m1; float* sc0; float* sc1;      // sc0 / sc1 arrive holding nn_kernel's similarities
    long long* mlist; float* mscores; int* n_matches; int* status;
    int* stop; long long* stop64; float* prune0; float* prune1;     // optional: zeros
};
// rows [0, n) of one side: the match (mutual: only if the other side's nearest neighbour points back), its score (s1 + 1) / 2, -1 / 0 for every other row
__device__ __forceinline__ void nn_side_row(int i, int live, bool mutual, const int* raw, const int* raw_other, long long* m, float* sc, float* prune,
                                            int& match, float& score) {
    match = -1; score = 0.f;
    if (i < live) {
        const int j = raw[i];
        if (j >= 0 && (!mutual || raw_other[j] == i)) { match = j; score = (sc[i] + 1.f) * 0.5f; }
    }
    m[i] = match; sc[i] = score;
    if (prune) prune[i] = 0.f;
}
__global__ __launch_bounds__(256) void nn_outputs_kernel(NnOutArgs a) {
    const int pair = a.pair0 + blockIdx.x, tid = threadIdx.x;
    const PairImages src = pair_images(a.px, pair);
    const bool ok = src.ok;
    int live0 = ok ? live_rows(a.num0, src.i0, a.n0) : 0, live1 = ok ? live_rows(a.num1, src.i1, a.n1) : 0;
    if (live0 == 0 || live1 == 0) live0 = live1 = 0;             // an empty side: nn_kernel's rows of this pair are not read
    const long long at0 = (long long)pair * a.n0, at1 = (long long)pair * a.n1;
    const int* raw0 = a.raw0 + at0; const int* raw1 = a.raw1 + at1;
    const bool mutual = a.mutual != 0;
    for (int j = tid; j < a.n1; j += 256) {
        int match; float score;
        nn_side_row(j, live1, mutual, raw1, raw0, a.m1 + at1, a.sc1 + at1, a.prune1 ? a.prune1 + at1 : nullptr, match, score);
    }
    // side 0, 256 rows at a time, with the running compaction of the matched rows in ascending order (ref :593-602)
    long long* mlist = a.mlist + (long long)pair * a.list_rows * 2;
    float* mscores = a.mscores + (long long)pair * a.list_rows;
    __shared__ int wsum[4];
    int base = 0;
    for (int r0 = 0; r0 < a.n0; r0 += 256) {
        const int i = r0 + tid;
        int match = -1; float score = 0.f;
        if (i < a.n0) nn_side_row(i, live0, mutual, raw0, raw1, a.m0 + at0, a.sc0 + at0, a.prune0 ? a.prune0 + at0 : nullptr, match, score);
        const int k = compact_slot(match >= 0, base, wsum);
        if (match >= 0 && k < a.list_rows) { mlist[2 * k] = i; mlist[2 * k + 1] = match; mscores[k] = score; }
    }
    if (tid == 0) {
        a.n_matches[pair] = min(base, a.list_rows);
        a.status[pair] = ok ? LG_OK : LG_ERR_INDEX;
        if (a.stop) a.stop[pair] = 0;
        if (a.stop64) a.stop64[pair] = 0;
    }
}

// ------------------------------------------------------------------ host side
template <int CMAX>
static hipError_t nn_launch(const NnArgs& a, int pairs, hipStream_t s) {
    const dim3 grid(pairs, (a.nA + NN_ROWS - 1) / NN_ROWS);
    return launch_with_lds(nn_kernel<CMAX>, grid, dim3(NN_THREADS), NN_TILE * (a.dim * 4 + 16), s, a);
}

}  // namespace lg

using namespace lg;

extern "C" {

int64_t lg_nn_workspace_bytes(int64_t images0, int64_t images1, int32_t n0, int32_t n1, int32_t dim, uint32_t flags) {
    NnLayout L;
    return nn_layout(images0, images1, n0, n1, dim, flags, L) ? -1 : L.total;
}

int lg_nn_match(const lg_nn_io* io, void* hip_stream) {
    if (!io) return set_error(LG_ERR_INVALID, "lg_nn_match: null io");
    const bool indexed = io->flags & LG_FLAG_INDEXED;
    const int P = io->pairs;
    if (P < 0) return set_error(LG_ERR_INVALID, "lg_nn_match: negative pair count");
    const long long images0 = indexed ? io->images0 : P, images1 = indexed ? io->images1 : P;
    NnLayout L;
    if (const char* why = nn_layout(images0, images1, io->n0, io->n1, io->dim, io->flags, L)) return set_error(LG_ERR_INVALID, std::string("lg_nn_match: ") + why);
    if (!(io->ratio_threshold <= 1.f)) return set_error(LG_ERR_INVALID, "lg_nn_match: ratio_threshold must lie in (0, 1] (<= 0: off)");
    if (io->distance_threshold != io->distance_threshold) return set_error(LG_ERR_INVALID, "lg_nn_match: distance_threshold is NaN");
    if (P == 0) return LG_OK;
    const int n0 = io->n0, n1 = io->n1, dim = io->dim;
    const bool mutual = io->flags & LG_FLAG_NN_MUTUAL;
    if (const int rc = check_pair_list("lg_nn_match", io->flags, io->index0, io->index1, images0, images1)) return rc;
    if ((L.rows0 && !io->desc0) || (L.rows1 && !io->desc1)) return set_error(LG_ERR_INVALID, "lg_nn_match: null descriptor pointer");
    if (!io->n_matches || !io->status || (n0 && (!io->raw0 || !io->matches0 || !io->scores0)) || (n1 && (!io->raw1 || !io->matches1 || !io->scores1)))
        return set_error(LG_ERR_INVALID, "lg_nn_match: null output pointer");
    const int list_need = mutual ? (n0 < n1 ? n0 : n1) : n0;
    if (io->list_rows < list_need) return set_error(LG_ERR_INVALID, "lg_nn_match: list_rows must be >= min(n0, n1) (mutual) or >= n0");
    if (io->list_rows && (!io->matches || !io->match_scores)) return set_error(LG_ERR_INVALID, "lg_nn_match: null match list pointer");
    if ((reinterpret_cast<uintptr_t>(io->desc0) & 15) || (reinterpret_cast<uintptr_t>(io->desc1) & 15))
        return set_error(LG_ERR_INVALID, "lg_nn_match: descriptor pointers must be 16-byte aligned");
    if (const int rc = check_workspace("lg_nn_match", "lg_nn_workspace_bytes", io->workspace, io->workspace_bytes, L.total, true)) return rc;

    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    char* ws = static_cast<char*>(io->workspace);
    const SideFormat f0 = side_format(io->flags | LG_FLAG_EXT, 0), f1 = side_format(io->flags | LG_FLAG_EXT, 1);
    // both sides read the same store in the same way (a pair list over one store): its rows are prepared once
    const bool shared = io->desc0 == io->desc1 && images0 == images1 && n0 == n1 && io->num0 == io->num1 && f0.kind == f1.kind && f0.rootsift == f1.rootsift;
    float* rows0 = reinterpret_cast<float*>(ws + L.ws0);
    float* rows1 = shared ? rows0 : reinterpret_cast<float*>(ws + L.ws1);
    unsigned char* touched0 = indexed ? reinterpret_cast<unsigned char*>(ws + L.touched0) : nullptr;
    unsigned char* touched1 = !indexed ? nullptr : shared ? touched0 : reinterpret_cast<unsigned char*>(ws + L.touched1);
    if (indexed) {
        HIPCHK(hipMemsetAsync(touched0, 0, (size_t)(L.total - L.touched0), s));
        const dim3 grid((P + 255) / 256);
        hipLaunchKernelGGL(nn_mark_kernel, grid, dim3(256), 0, s, NnMarkArgs{io->index0, P, (int)images0, touched0});
        hipLaunchKernelGGL(nn_mark_kernel, grid, dim3(256), 0, s, NnMarkArgs{io->index1, P, (int)images1, touched1});
    }
    if (L.rows0)
        hipLaunchKernelGGL(nn_prep_kernel, dim3((unsigned)((L.rows0 + 3) / 4)), dim3(256), 0, s,
                           NnPrepArgs{io->desc0, f0.kind, f0.rootsift ? 1 : 0, io->num0, touched0, L.rows0, n0, dim, rows0});
    if (L.rows1 && !shared)
        hipLaunchKernelGGL(nn_prep_kernel, dim3((unsigned)((L.rows1 + 3) / 4)), dim3(256), 0, s,
                           NnPrepArgs{io->desc1, f1.kind, f1.rootsift ? 1 : 0, io->num1, touched1, L.rows1, n1, dim, rows1});
    HIPCHK(hipGetLastError());

    const float ratio2 = io->ratio_threshold > 0.f ? io->ratio_threshold * io->ratio_threshold : 0.f;
    const float dist2 = io->distance_threshold > 0.f ? io->distance_threshold * io->distance_threshold : 0.f;
    const PairIndex px01 = indexed ? PairIndex{io->index0, io->index1, (int)images0, (int)images1} : PairIndex{};
    const PairIndex px10{px01.index1, px01.index0, px01.images1, px01.images0};
    return for_pair_launches(P, [&](int p0, int count) -> int {
        const NnArgs dir[2] = {{rows0, rows1, io->num0, io->num1, px01, n0, n1, dim, p0, ratio2, dist2, io->raw0, io->scores0},
                               {rows1, rows0, io->num1, io->num0, px10, n1, n0, dim, p0, ratio2, dist2, io->raw1, io->scores1}};
        for (const NnArgs& a : dir) {
            if (a.nA == 0 || a.nB == 0) continue;     // nn_outputs_kernel reads nothing of an empty side
            HIPCHK(dim <= 64 ? nn_launch<4>(a, count, s) : dim <= 128 ? nn_launch<8>(a, count, s) : nn_launch<16>(a, count, s));
        }
        const NnOutArgs o{px01, io->num0, io->num1, n0, n1, p0, mutual ? 1 : 0, io->list_rows, io->raw0, io->raw1,
                          reinterpret_cast<long long*>(io->matches0), reinterpret_cast<long long*>(io->matches1), io->scores0, io->scores1,
                          reinterpret_cast<long long*>(io->matches), io->match_scores, io->n_matches, io->status,
                          io->stop, reinterpret_cast<long long*>(io->stop_i64), io->prune0, io->prune1};
        hipLaunchKernelGGL(nn_outputs_kernel, dim3(count), dim3(256), 0, s, o);
        HIPCHK(hipGetLastError());
        return LG_OK;
    });
}

}  // extern "C"
