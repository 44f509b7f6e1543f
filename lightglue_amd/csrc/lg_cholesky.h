// lightglue_amd — THE dense blocked Cholesky of the bundle adjuster and of the pose-graph solver (include/lightglue_amd.h, lg_bundle_adjust: "Cholesky"):
// left-looking, 48 columns per panel, two launches per panel, the right-hand sides carried as extra rows of the matrix, a flag on a failed pivot, and the
// substitution L^T x = z for every right-hand side.  Parameters: the matrix, dim, the number of right-hand-side rows (1 in lg_bundle.hip; 3 and 1 in
// lg_posegraph.hip) and the pivot floor (0 in lg_bundle.hip, 1e-10 in lg_posegraph.hip).  Device code, to be called by ALL 256 threads of a workgroup; the caller's kernels name the
// launch (which panel, which tile) and test their own "converged" record first.  The matrix is S [dim + nrhs][dim] row-major, only its lower triangle is
// read; rows dim .. dim + nrhs - 1 hold the right-hand sides and come out as z = L^-1 rhs.  The order of every sum is the header's.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace lg {

constexpr int CH_THREADS = 256, CH_NB = 48, CH_KT = 32, CH_PARTS = 5;

struct CholeskyDiagLds { double Bs[CH_NB][CH_KT + 1], Dm[CH_NB][CH_NB + 1], od[CH_NB]; };
struct CholeskyRowsLds { double As[CH_NB][CH_KT + 1], Bs[CH_NB][CH_KT + 1], Lp[CH_NB][CH_NB + 1], Gm[CH_NB][CH_NB + 1]; };
struct CholeskySolveLds { double part[CH_PARTS][CH_NB], Lp[CH_NB][CH_NB + 1]; };

// a. ONE workgroup: the panel's diagonal block D = S_pp - L_p L_p^T over all earlier columns, factored in LDS and written over S_pp.  A pivot that is not
// finite or not above floor x (the entry's value in S) sets *fail and is replaced by 1
__device__ __forceinline__ void cholesky_diag(double* S, int dim, int panel, double floor, int* fail, CholeskyDiagLds& m) {
    const int t = threadIdx.x, tr = t >> 4, tc = t & 15;
    const int C0 = panel * CH_NB, nb = min(CH_NB, dim - C0);
    double acc[3][3];
#pragma unroll
    for (int ii = 0; ii < 3; ++ii)
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) acc[ii][jj] = 0.0;
    for (int k0 = 0; k0 < C0; k0 += CH_KT) {
        const int kt = min(CH_KT, C0 - k0);
        __syncthreads();
        for (int q = t; q < CH_NB * CH_KT; q += CH_THREADS) {
            const int row = q / CH_KT, kk = q - row * CH_KT;
            m.Bs[row][kk] = (row < nb && kk < kt) ? S[(long long)(C0 + row) * dim + k0 + kk] : 0.0;
        }
        __syncthreads();
        for (int kk = 0; kk < kt; ++kk) {
            double bv[3], dv[3];
#pragma unroll
            for (int ii = 0; ii < 3; ++ii) { dv[ii] = m.Bs[tr + 16 * ii][kk]; bv[ii] = m.Bs[tc + 16 * ii][kk]; }
#pragma unroll
            for (int ii = 0; ii < 3; ++ii)
#pragma unroll
                for (int jj = 0; jj < 3; ++jj) acc[ii][jj] += dv[ii] * bv[jj];
        }
    }
#pragma unroll
    for (int ii = 0; ii < 3; ++ii)
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) {
            const int row = tr + 16 * ii, col = tc + 16 * jj;
            m.Dm[row][col] = (row < nb && col <= row) ? S[(long long)(C0 + row) * dim + C0 + col] - acc[ii][jj] : 0.0;
        }
    if (t < CH_NB) m.od[t] = t < nb ? S[(long long)(C0 + t) * dim + C0 + t] : 1.0;
    __syncthreads();
    for (int kk = 0; kk < nb; ++kk) {                                   // right-looking inside the block
        double d = m.Dm[kk][kk];
        const bool good = isfinite(d) && d > floor * m.od[kk];
        if (!good) d = 1.0;
        const double l = sqrt(d);
        __syncthreads();
        if (t == 0) { m.Dm[kk][kk] = l; if (!good) atomicOr(fail, 1); }
        if (t > kk && t < nb) m.Dm[t][kk] = m.Dm[t][kk] / l;
        __syncthreads();
        for (int q = t; q < CH_NB * CH_NB; q += CH_THREADS) {
            const int row = q / CH_NB, col = q - row * CH_NB;
            if (col > kk && col <= row && row < nb) m.Dm[row][col] = m.Dm[row][col] - m.Dm[row][kk] * m.Dm[col][kk];
        }
        __syncthreads();
    }
    for (int q = t; q < CH_NB * CH_NB; q += CH_THREADS) {
        const int row = q / CH_NB, col = q - row * CH_NB;
        if (row < nb && col <= row) S[(long long)(C0 + row) * dim + C0 + col] = m.Dm[row][col];
    }
}

// b. workgroup `tile` (>= panel) of the rows [48 tile, 48 tile + 48) below the panel's diagonal block, right-hand-side rows included: G = S_ip - L_i L_p^T,
// then L_i = G L_pp^-T.  It writes its own rows' panel columns, which no other workgroup of the launch reads
__device__ __forceinline__ void cholesky_rows(double* S, int dim, int nrhs, int panel, int tile, CholeskyRowsLds& m) {
    const int t = threadIdx.x, tr = t >> 4, tc = t & 15;
    const int C0 = panel * CH_NB, nb = min(CH_NB, dim - C0);
    const int R0 = tile * CH_NB, nr = min(CH_NB, dim + nrhs - R0);
    if (R0 + nr <= C0 + nb) return;                                     // uniform over the workgroup: nothing below the block
    double acc[3][3];
#pragma unroll
    for (int ii = 0; ii < 3; ++ii)
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) acc[ii][jj] = 0.0;
    for (int k0 = 0; k0 < C0; k0 += CH_KT) {
        const int kt = min(CH_KT, C0 - k0);
        __syncthreads();
        for (int q = t; q < CH_NB * CH_KT; q += CH_THREADS) {
            const int row = q / CH_KT, kk = q - row * CH_KT;
            m.As[row][kk] = (row < nr && R0 + row >= C0 + nb && kk < kt) ? S[(long long)(R0 + row) * dim + k0 + kk] : 0.0;
            m.Bs[row][kk] = (row < nb && kk < kt) ? S[(long long)(C0 + row) * dim + k0 + kk] : 0.0;
        }
        __syncthreads();
        for (int kk = 0; kk < kt; ++kk) {
            double av[3], bv[3];
#pragma unroll
            for (int ii = 0; ii < 3; ++ii) { av[ii] = m.As[tr + 16 * ii][kk]; bv[ii] = m.Bs[tc + 16 * ii][kk]; }
#pragma unroll
            for (int ii = 0; ii < 3; ++ii)
#pragma unroll
                for (int jj = 0; jj < 3; ++jj) acc[ii][jj] += av[ii] * bv[jj];
        }
    }
#pragma unroll
    for (int ii = 0; ii < 3; ++ii)
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) {
            const int row = tr + 16 * ii, col = tc + 16 * jj;
            m.Gm[row][col] = (row < nr && col < nb && R0 + row >= C0 + nb) ? S[(long long)(R0 + row) * dim + C0 + col] - acc[ii][jj] : 0.0;
            m.Lp[row][col] = (row < nb && col <= row) ? S[(long long)(C0 + row) * dim + C0 + col] : 0.0;
        }
    __syncthreads();
    if (t < nr && R0 + t >= C0 + nb) {                                  // one lane per row, columns in ascending order
        for (int col = 0; col < nb; ++col) {
            double v = m.Gm[t][col];
            for (int kk = 0; kk < col; ++kk) v = v - m.Gm[t][kk] * m.Lp[col][kk];
            v = v / m.Lp[col][col];
            m.Gm[t][col] = v;
            S[(long long)(R0 + t) * dim + C0 + col] = v;
        }
    }
}

// c. ONE workgroup: L^T x = z backwards for each of the nrhs right-hand sides, x of right-hand side r left in sd[r dim .. r dim + dim) (LDS of the caller).
// Per panel the rows below are summed in CH_PARTS interleaved partial sums (row i goes to partial (i - first row below) mod 5), added in order 0 .. 4.
// Ends with a barrier: every thread may read sd afterwards
__device__ __forceinline__ void cholesky_backsolve(const double* S, int dim, int nrhs, double* sd, CholeskySolveLds& m) {
    const int t = threadIdx.x;
    const int panels = (dim + CH_NB - 1) / CH_NB;
    for (int panel = panels - 1; panel >= 0; --panel) {
        const int C0 = panel * CH_NB, nb = min(CH_NB, dim - C0), below = C0 + nb;
        for (int q = t; q < CH_NB * CH_NB; q += CH_THREADS) {
            const int row = q / CH_NB, col = q - row * CH_NB;
            m.Lp[row][col] = (row < nb && col <= row) ? S[(long long)(C0 + row) * dim + C0 + col] : 0.0;
        }
        for (int r = 0; r < nrhs; ++r) {
            double* x = sd + r * dim;
            const double* z = S + (long long)(dim + r) * dim;
            if (t < CH_PARTS * CH_NB) {
                const int col = t % CH_NB, part_id = t / CH_NB;
                double sum = 0.0;
                if (col < nb) for (int i = below + part_id; i < dim; i += CH_PARTS) sum += S[(long long)i * dim + C0 + col] * x[i];
                m.part[part_id][col] = sum;
            }
            __syncthreads();
            if (t == 0)
                for (int col = nb - 1; col >= 0; --col) {
                    double v = z[C0 + col] - ((((m.part[0][col] + m.part[1][col]) + m.part[2][col]) + m.part[3][col]) + m.part[4][col]);
                    for (int i = col + 1; i < nb; ++i) v = v - m.Lp[i][col] * x[C0 + i];
                    x[C0 + col] = v / m.Lp[col][col];
                }
            __syncthreads();
        }
    }
}

}  // namespace lg
