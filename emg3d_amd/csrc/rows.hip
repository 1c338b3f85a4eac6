// Device-resident row store: n_rows x n_cols doubles, row-major, in one block of HBM of its own, and the dense products over them --
// emg3d_rows_* of include/emg3d_hip.h.  gfx950 only.
//
//   k_rows_park           one chunk of rows from a handle's row buffer into their store rows (emg3d_mg_sens_rows_park)
//   k_sens_rows_fill      (csrc/gradient.hpp) both parts of a chunk's rows from the fields into their store rows, no row buffer
//                         (emg3d_mg_sens_rows_fill)
//   k_rows_gram           G = R diag(cm) R^T: per (K-slab, pair of row blocks) one workgroup on v_mfma_f64_16x16x4_f64, slab partials
//   k_rows_gram_reduce    the slab partials summed in ascending slab order, the lower triangle mirrored
//   k_rows_matvec(_reduce) R v: per (row, slab) a fixed tree, the slab partials summed in ascending order
//   k_rows_rmatvec        cm (.) R^T y: one thread per column, rows ascending, no contraction
//   k_rows_project        Y = M R into another store: per (panel of columns, block of output rows) one workgroup on the f64 MFMA, one
//                         accumulation chain over the source's rows per element, each element written once
//   k_rows_colsumsq       sum_i s[i] R[i][j]^2: one thread per column, rows ascending, no contraction
//   k_rows_smooth_*       the smoothing model covariance: tridiagonal line solves over every row, in place (rows_cov.hpp)
//
// No floating-point atomics anywhere: every result is a fixed expression of the store, of n_cols and of the operands.
#include "../../include/emg3d_hip.h"

#include <algorithm>
#include <new>
#include <vector>

#include "gradient.hpp"
#include "rows.hpp"
#include "rows_cov.hpp"

struct emg3d_rows {
    int device = 0;
    i64 n_rows = 0, n_cols = 0;
    double* R = nullptr;            // the block
    size_t nbytes = 0;              // its size (256-byte aligned)
    hipStream_t stream = nullptr;   // the store's own products run here; every entry point ends with a synchronise
    int32_t* d_dest = nullptr;      // park: destination rows of a chunk's pairs; fill: two tables (real parts, then imaginary parts)
    double* chain[3] = {nullptr, nullptr, nullptr};     // chain factors of emg3d_rows_set_chain (one block)
    i64 chain_n = 0;
    size_t chain_bytes = 0;
    char* ws = nullptr;             // workspace of the products (operands, slab partials, results): one block that grows to the largest
    size_t ws_bytes = 0;            // call so far -- a hipMalloc / hipFree pair per call costs more than the kernels
};

namespace {

constexpr int PARK_PAIRS_MAX = 64 * 64;         // pairs of one emg3d_mg_sens_rows call

size_t aligned(size_t nb) { return (nb + 255) & ~(size_t)255; }

// optional device memory: a failing hipMalloc is the caller's business
void* quiet_alloc(size_t nb) {
    void* p = nullptr;
    hipError_t st = hipMalloc(&p, nb);
    if (st != hipSuccess) {         // blocks parked in the handles' pool count as free (emg3d_hip_mem_info)
        (void)hipGetLastError();
        if (emg3d_hip_release_cached() > 0) st = hipMalloc(&p, nb);
    }
    if (st != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
// The pieces of one call, carved from the store's workspace in the order they are asked for; `sizes`: their doubles.  nullptr for
// all: the workspace did not fit (the store stays usable).
template <int N>
bool carve(emg3d_rows* r, const size_t (&sizes)[N], double* (&out)[N]) {
    size_t need = 0;
    for (int i = 0; i < N; ++i) need += aligned(std::max<size_t>(sizes[i], 1) * sizeof(double));
    if (r->ws_bytes < need) {
        if (r->ws) { (void)hipStreamSynchronize(r->stream); (void)hipFree(r->ws); r->ws = nullptr; r->ws_bytes = 0; }
        r->ws = (char*)quiet_alloc(need);
        if (!r->ws) return false;
        r->ws_bytes = need;
    }
    size_t off = 0;
    for (int i = 0; i < N; ++i) { out[i] = (double*)(r->ws + off); off += aligned(std::max<size_t>(sizes[i], 1) * sizeof(double)); }
    return true;
}

#define ROWS_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { (void)hipGetLastError(); return (int)_e; } } while (0)

int to_device(emg3d_rows* r, void* dst, const void* src, size_t nb) {
    ROWS_TRY(hipMemcpyAsync(dst, src, nb, hipMemcpyHostToDevice, r->stream));
    ROWS_TRY(hipStreamSynchronize(r->stream));
    return 0;
}
int to_host(emg3d_rows* r, void* dst, const void* src, size_t nb) {
    ROWS_TRY(hipMemcpyAsync(dst, src, nb, hipMemcpyDeviceToHost, r->stream));
    ROWS_TRY(hipStreamSynchronize(r->stream));
    return 0;
}
int launched() {
    const hipError_t st = hipGetLastError();
    return st == hipSuccess ? 0 : (int)st;
}

typedef double d4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------- park
// grid (cells / 256, pairs).  The operations and their order are those of optimize.SurveyJacobian.sensitivity_rows on the host (chain
// factor times value, then (p0 + p1) + p2), without contraction: a parked row equals the row it returns, bit for bit.
__global__ void __launch_bounds__(256) k_rows_park(double* __restrict__ R, i64 n_cols, const double* __restrict__ src, int ndir, int npart,
                                                   i64 ncells, const int32_t* __restrict__ dest, const double* c0, const double* c1,
                                                   const double* c2, int sum3) {
#pragma clang fp contract(off)
    const i64 cell = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 p = blockIdx.y;
    const i64 d = dest[p];
    if (d < 0 || cell >= ncells) return;
    const double* s = src + p * ndir * npart * ncells + cell;
    double* out = R + d * n_cols + cell;
    const i64 plane = (i64)npart * ncells;
    if (sum3) {
        double v0 = s[0], v1 = s[plane], v2 = s[2 * plane];
        if (c0) { v0 = c0[cell] * v0; v1 = c1[cell] * v1; v2 = c2[cell] * v2; }
        out[0] = (v0 + v1) + v2;
    } else {
        const double* c[3] = {c0, c1, c2};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (q >= ndir) break;
            double v = s[q * plane];
            if (c[q]) v = c[q][cell] * v;
            out[q * ncells] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- gram
// grid (nslab, jobs of this batch), 512 threads = 8 waves.  Per step of 16 columns the workgroup stages its two row blocks as
// [k][row] tiles in LDS -- global reads run along the rows (16 lanes per row, 128 contiguous bytes), cm multiplies the B
// operand only, rows past n_rows and columns past the slab are staged as zeros --, the next step's values already in flight in
// registers; then every wave runs its tile pairs: lane l takes A[i = l & 15][k = l >> 4] = As[k][16 ta + i] and
// B[k = l >> 4][j = l & 15] = Bs[k][16 tb + j], one f64 each, and D[i][j] += sum_k A[i][k] B[k][j].  The f64 result map is its own:
// register r of lane l is D[i = (l >> 4) + 4 r][j = l & 15], i.e. element l + 64 r of the row-major 16 x 16 tile.
// part = [job in batch][t][slab][256].
//
// gram_job: one job on one slab.  DIAG: the 36 tile pairs ta >= tb of one block, 5 per wave (waves 4 .. 7 repeat pair 0 as their fifth and drop
// it); otherwise the 64 pairs of two blocks, 8 per wave.  Nothing in the loop is conditional: the loads of a step are issued
// together from clamped addresses and zeroed by a select, and a tile past the last row multiplies zeros and is dropped at the end.
template <bool DIAG, bool CM>
__device__ __forceinline__ void gram_job(const double* __restrict__ R, const double* __restrict__ cm, double* __restrict__ out, i64 n_rows,
                                         i64 n_cols, i64 c0, i64 c1, i64 ra0, i64 rb0, i64 nslab, double* As, double* Bs) {
    constexpr int NT = DIAG ? 5 : 8;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int oa[NT], ob[NT];
    bool live[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        int ta, tb;
        if (!rows_job_tile(DIAG, wave + ROWS_WAVES * i, ta, tb)) { ta = tb = 0; live[i] = false; }
        else live[i] = ra0 + ta * ROWS_TILE < n_rows && rb0 + tb * ROWS_TILE < n_rows;          // (not wholly past the last row)
        oa[i] = ta * ROWS_TILE; ob[i] = tb * ROWS_TILE;
    }
    d4 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = (d4){0.0, 0.0, 0.0, 0.0};

    // staging: element e = tid + 512 i of the 128 x 16 block, row e >> 4 = sr + 32 i, k = e & 15
    const int sk = tid & 15, sr = tid >> 4;
    // fetch: the raw values of a step into registers (nothing waits for them); stage: zeros and cm applied, into LDS -- a step later,
    // after the MFMAs that hide the loads' latency
    double va[4], vb[4], vw = 1.0;
    auto fetch = [&](i64 c) {
        const i64 col = c + sk;
        const i64 cc = col < c1 ? col : c1 - 1;
        if (CM) vw = cm[cc];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const i64 ga = ra0 + sr + 32 * i, gb = rb0 + sr + 32 * i;
            va[i] = R[(ga < n_rows ? ga : n_rows - 1) * n_cols + cc];
            if (!DIAG) vb[i] = R[(gb < n_rows ? gb : n_rows - 1) * n_cols + cc];
        }
    };
    auto stage = [&](i64 c) {
        const bool in = c + sk < c1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double b = DIAG ? va[i] : vb[i];
            As[sk * ROWS_LD + sr + 32 * i] = (in && ra0 + sr + 32 * i < n_rows) ? va[i] : 0.0;
            Bs[sk * ROWS_LD + sr + 32 * i] = (in && rb0 + sr + 32 * i < n_rows) ? (CM ? vw * b : b) : 0.0;
        }
    };
    fetch(c0);
    const int fk = lane >> 4, fi = lane & 15;
    for (i64 c = c0; c < c1; c += ROWS_KSTEP) {
        __syncthreads();            // the previous step's operand reads are done
        stage(c);
        __syncthreads();
        if (c + ROWS_KSTEP < c1) fetch(c + ROWS_KSTEP);
#pragma unroll
        for (int kk = 0; kk < ROWS_KSTEP / 4; ++kk) {
            const int k = (4 * kk + fk) * ROWS_LD + fi;
            double fa[NT], fb[NT];          // all operands of this k first, then the MFMAs back to back
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                fa[i] = As[k + oa[i]];
                fb[i] = (DIAG || i == 0) ? Bs[k + ob[i]] : fb[0];           // (two blocks: tile pair t = wave + 8 i has tb = wave for every i)
            }
#pragma unroll
            for (int i = 0; i < NT; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[i], acc[i], 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        if (!live[i]) continue;
        double* o = out + (i64)(wave + ROWS_WAVES * i) * nslab * 256 + lane;
        o[0] = acc[i][0]; o[64] = acc[i][1]; o[128] = acc[i][2]; o[192] = acc[i][3];
    }
}

__global__ void __launch_bounds__(64 * ROWS_WAVES, 4) k_rows_gram(const double* __restrict__ R, const double* __restrict__ cm,
                                                                double* __restrict__ part, i64 n_rows, i64 n_cols, i64 slab, i64 nslab,
                                                                i64 job0) {
    __shared__ double As[ROWS_KSTEP * ROWS_LD];
    __shared__ double Bs[ROWS_KSTEP * ROWS_LD];
    const i64 s = blockIdx.x;
    i64 ba, bb;
    rows_job_blocks(job0 + blockIdx.y, ba, bb);
    const i64 c0 = s * slab, c1 = c0 + slab < n_cols ? c0 + slab : n_cols;
    const i64 ra0 = ba * ROWS_BLOCK, rb0 = bb * ROWS_BLOCK;
    double* out = part + ((i64)blockIdx.y * 64 * nslab + s) * 256;          // tile pair t of this job and slab: + t * nslab * 256
    if (ba == bb) {
        if (cm) gram_job<true, true>(R, cm, out, n_rows, n_cols, c0, c1, ra0, rb0, nslab, As, Bs);
        else gram_job<true, false>(R, cm, out, n_rows, n_cols, c0, c1, ra0, rb0, nslab, As, Bs);
    } else {
        if (cm) gram_job<false, true>(R, cm, out, n_rows, n_cols, c0, c1, ra0, rb0, nslab, As, Bs);
        else gram_job<false, false>(R, cm, out, n_rows, n_cols, c0, c1, ra0, rb0, nslab, As, Bs);
    }
}

// grid (64 tile pairs, jobs of this batch), 256 threads = the elements of a tile.  Element (gi, gj), gi >= gj, is the sum of its slab
// partials in ascending slab order, written to G[gi][gj] and G[gj][gi]: G == G^T exactly; a diagonal tile's upper half is dropped
// (cm sits on one operand, so its rounding is not the lower half's).
__global__ void __launch_bounds__(256) k_rows_gram_reduce(double* __restrict__ G, const double* __restrict__ part, i64 n_rows, i64 nslab,
                                                          i64 job0) {
    i64 ba, bb;
    rows_job_blocks(job0 + blockIdx.y, ba, bb);
    int ta, tb;
    if (!rows_job_tile(ba == bb, (int)blockIdx.x, ta, tb)) return;
    const int e = threadIdx.x;
    const i64 gi = ba * ROWS_BLOCK + ta * ROWS_TILE + (e >> 4), gj = bb * ROWS_BLOCK + tb * ROWS_TILE + (e & 15);
    if (gi >= n_rows || gj >= n_rows || gi < gj) return;
    const double* p = part + ((i64)blockIdx.y * 64 + blockIdx.x) * nslab * 256 + e;
    double sum = p[0];
    for (i64 s = 1; s < nslab; ++s) sum += p[s * 256];
    G[gi * n_rows + gj] = sum;
    G[gj * n_rows + gi] = sum;
}

// ---------------------------------------------------------------------------------------------------------------- matvec
// grid (n_rows * nslab), 256 threads: block = (row, slab); thread t sums columns c0 + t, c0 + t + 256, ... of the slab in ascending
// order, the 256 sums meet in a fixed tree.  part = [row][slab].
__global__ void __launch_bounds__(256) k_rows_matvec(const double* __restrict__ R, const double* __restrict__ v, double* __restrict__ part,
                                                     i64 n_cols, i64 slab, i64 nslab) {
    __shared__ double red[256];
    const i64 row = (i64)blockIdx.x / nslab, s = (i64)blockIdx.x % nslab;
    const i64 c0 = s * slab, c1 = c0 + slab < n_cols ? c0 + slab : n_cols;
    const double* r = R + row * n_cols;
    double acc = 0.0;
    for (i64 c = c0 + threadIdx.x; c < c1; c += 256) acc = __builtin_fma(r[c], v[c], acc);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
__global__ void __launch_bounds__(256) k_rows_matvec_reduce(double* __restrict__ out, const double* __restrict__ part, i64 n_rows, i64 nslab) {
    const i64 row = (i64)blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const double* p = part + row * nslab;
    double sum = p[0];
    for (i64 s = 1; s < nslab; ++s) sum += p[s];
    out[row] = sum;
}

// ---------------------------------------------------------------------------------------------------------------- rmatvec
// one thread per column: acc = acc + y[rho] * R[rho][j], rows ascending, then cm[j] * acc; products and sums rounded apart
__global__ void __launch_bounds__(256) k_rows_rmatvec(const double* __restrict__ R, const double* __restrict__ y, const double* __restrict__ cm,
                                                      double* __restrict__ out, i64 n_rows, i64 n_cols) {
#pragma clang fp contract(off)
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_cols) return;
    double acc = 0.0;
    for (i64 r = 0; r < n_rows; ++r) acc = acc + y[r] * R[r * n_cols + j];
    out[j] = cm ? cm[j] * acc : acc;
}

// ---------------------------------------------------------------------------------------------------------------- project
// Y[m x n_cols] = M[m x n_rows] R[n_rows x n_cols], the contraction over the ROWS of the store: every column is on its own, there is
// no split over k, no partial and no second pass.  grid (panels), 256 threads = 4 waves; one launch per block of output rows
// (row0), NT the row tiles per wave (rows.hpp).  Mt is M transposed, [n_rows][m]: the slice of a step is then read along the output
// rows, as the slice of R is read along its columns -- 64 contiguous doubles per wave both -- and both are written to LDS as they
// are read: As[k][i], Bs[k][j].  Lane l takes A[i = l & 15][k = l >> 4] = As[4 kk + k][16 t + i] and B[k = l >> 4][j = l & 15] =
// Bs[4 kk + k][16 c + j]; result register r of lane l is D[(l >> 4) + 4 r][l & 15] (the f64 map), so that 16 lanes write 128
// contiguous bytes of one row of Y.  Element (i, j) is ONE chain over k = 0 .. n_rows - 1 in groups of four, ascending, padded
// with zeros to a multiple of 16.  Nothing in the loop is conditional: every load of a step comes from a clamped address and is
// selected to zero where it lies past n_rows, m or n_cols (so that a NaN next door never enters a product); the next step's loads
// (clamped too: the step after the last reads the last row again and drops it) are issued before the MFMAs and staged after them.
// NT = 8 asks for two workgroups per compute unit: its 128 accumulator registers and the operands then share the 256 a lane may
// have (no scratch; without the bound the compiler takes 318 and one workgroup).
template <int NT>
__global__ void __launch_bounds__(PROJ_THREADS, NT == 8 ? 2 : 1) k_rows_project(const double* __restrict__ R, const double* __restrict__ Mt,
                                                               double* __restrict__ Y, i64 n_rows, i64 m, i64 n_cols, i64 row0) {
    constexpr int BR = 32 * NT, LDA = BR + PROJ_PAD, LDB = PROJ_COLS + PROJ_PAD;
    constexpr int NA = PROJ_KSTEP * BR / PROJ_THREADS, KA = PROJ_THREADS / BR;      // values of M per thread and step; k between them
    constexpr int NB = PROJ_KSTEP * PROJ_COLS / PROJ_THREADS, KB = PROJ_THREADS / PROJ_COLS;
    __shared__ double As[PROJ_KSTEP * LDA];
    __shared__ double Bs[PROJ_KSTEP * LDB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const i64 col0 = (i64)blockIdx.x * PROJ_COLS;
    const int ra = (wave & 1) * (16 * NT), cb = (wave >> 1) * 32;
    d4 acc[NT][2];
#pragma unroll
    for (int t = 0; t < NT; ++t) { acc[t][0] = (d4){0.0, 0.0, 0.0, 0.0}; acc[t][1] = (d4){0.0, 0.0, 0.0, 0.0}; }

    // staging: element e = tid + 256 q of the 16 x 64 slice of R is (k = e / 64, j = e % 64), of the 16 x BR slice of Mt (k = e / BR, i = e % BR)
    const int bj = tid & (PROJ_COLS - 1), bk = tid / PROJ_COLS;
    const int ai = tid & (BR - 1), ak = tid / BR;
    const bool cin = col0 + bj < n_cols, iin = row0 + ai < m;
    const double* rp = R + (cin ? col0 + bj : n_cols - 1);
    const double* mp = Mt + (iin ? row0 + ai : m - 1);
    const i64 klast = n_rows - 1;
    double va[NA], vb[NB];
    auto fetch = [&](i64 k0) {
#pragma unroll
        for (int q = 0; q < NB; ++q) { const i64 k = k0 + bk + KB * q; vb[q] = rp[(k < klast ? k : klast) * n_cols]; }
#pragma unroll
        for (int q = 0; q < NA; ++q) { const i64 k = k0 + ak + KA * q; va[q] = mp[(k < klast ? k : klast) * m]; }
    };
    auto stage = [&](i64 k0) {
#pragma unroll
        for (int q = 0; q < NB; ++q) Bs[(bk + KB * q) * LDB + bj] = (cin & (k0 + bk + KB * q < n_rows)) ? vb[q] : 0.0;
#pragma unroll
        for (int q = 0; q < NA; ++q) As[(ak + KA * q) * LDA + ai] = (iin & (k0 + ak + KA * q < n_rows)) ? va[q] : 0.0;
    };
    fetch(0);
    const int fk = lane >> 4, fi = lane & 15;
    for (i64 k0 = 0; k0 < n_rows; k0 += PROJ_KSTEP) {
        __syncthreads();            // the previous step's operand reads are done
        stage(k0);
        __syncthreads();
        fetch(k0 + PROJ_KSTEP);
        __builtin_amdgcn_sched_barrier(0);          // (the loads are issued here, ahead of the MFMAs that hide their latency, not after them)
#pragma unroll
        for (int kk = 0; kk < PROJ_KSTEP / 4; ++kk) {
            const int k = 4 * kk + fk;
            double fa[NT], fb[2];           // all operands of this k first, then the MFMAs back to back
            fb[0] = Bs[k * LDB + cb + fi];
            fb[1] = Bs[k * LDB + cb + 16 + fi];
#pragma unroll
            for (int t = 0; t < NT; ++t) fa[t] = As[k * LDA + ra + 16 * t + fi];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                acc[t][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[t], fb[0], acc[t][0], 0, 0, 0);
                acc[t][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[t], fb[1], acc[t][1], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const i64 col = col0 + cb + 16 * c + fi;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const i64 row = row0 + ra + 16 * t + fk + 4 * r;
                if (row < m && col < n_cols) Y[row * n_cols + col] = acc[t][c][r];
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------- colsumsq
// one thread per column: acc = acc + s[i] * (R[i][j] * R[i][j]) (S) or acc + R[i][j] * R[i][j], rows ascending, every operation
// rounded once; the loads of COLSUM_U rows are issued before the chain that consumes them
constexpr int COLSUM_U = 8;
template <bool S>
__global__ void __launch_bounds__(256) k_rows_colsumsq(const double* __restrict__ R, const double* __restrict__ s, double* __restrict__ out,
                                                       i64 n_rows, i64 n_cols) {
#pragma clang fp contract(off)
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_cols) return;
    const double* p = R + j;
    double acc = 0.0;
    i64 r = 0;
    for (; r + COLSUM_U <= n_rows; r += COLSUM_U) {
        double v[COLSUM_U];
#pragma unroll
        for (int k = 0; k < COLSUM_U; ++k) v[k] = p[(r + k) * n_cols];
#pragma unroll
        for (int k = 0; k < COLSUM_U; ++k) {
            const double q = v[k] * v[k];
            acc = S ? acc + s[r + k] * q : acc + q;
        }
    }
    for (; r < n_rows; ++r) {
        const double v = p[r * n_cols];
        const double q = v * v;
        acc = S ? acc + s[r] * q : acc + q;
    }
    out[j] = acc;
}

}  // namespace

// ====================================================================================================== C ABI
int emg3d_rows_gram_plan(int64_t n_rows, int64_t n_cols, int64_t* out) {
    if (n_rows < 1 || n_cols < 1 || !out) return -2;
    const RowsGramPlan p = rows_gram_plan(n_rows, n_cols);
    out[0] = ROWS_BLOCK; out[1] = ROWS_KSTEP; out[2] = p.slab; out[3] = p.nslab; out[4] = p.nblk; out[5] = p.njobs;
    out[6] = p.njobs * p.nslab; out[7] = p.lds_bytes;
    return 0;
}

int emg3d_rows_gram_job(int64_t n_rows, int64_t job, int64_t* out) {
    if (n_rows < 1 || job < 0 || !out) return -2;
    const RowsGramPlan p = rows_gram_plan(n_rows, 1);
    if (job >= p.njobs) return -2;
    i64 ba, bb;
    rows_job_blocks(job, ba, bb);
    out[0] = ba * ROWS_BLOCK; out[1] = std::min<i64>(n_rows, (ba + 1) * ROWS_BLOCK);
    out[2] = bb * ROWS_BLOCK; out[3] = std::min<i64>(n_rows, (bb + 1) * ROWS_BLOCK);
    return 0;
}

int emg3d_rows_gram_batch(int64_t n_rows, int64_t n_cols, int64_t* out) {
    if (n_rows < 1 || n_cols < 1 || !out) return -2;
    const RowsGramBatch b = rows_gram_batch(n_rows, n_cols);
    out[0] = b.batch; out[1] = b.launches; out[2] = b.per_job; out[3] = ROWS_GRAM_SCRATCH;
    return 0;
}

int emg3d_rows_create(int device, int64_t n_rows, int64_t n_cols, emg3d_rows_t** out) {
    if (!out || n_rows < 1 || n_cols < 1) return -2;
    *out = nullptr;
    if (n_cols > (((int64_t)1 << 59) / n_rows)) return (int)hipErrorOutOfMemory;        // (n_rows * n_cols * 8 must fit an int64)
    const size_t nb = aligned((size_t)n_rows * (size_t)n_cols * sizeof(double));
    int64_t fr = 0, tot = 0;
    const int st = emg3d_hip_mem_info(device, &fr, &tot);
    if (st) return st;
    if ((int64_t)nb > fr + emg3d_hip_cached_bytes_on(device)) return (int)hipErrorOutOfMemory;     // (no allocation attempted)
    ROWS_TRY(hipSetDevice(device));
    emg3d_rows* r = new (std::nothrow) emg3d_rows();
    if (!r) return -3;
    r->device = device; r->n_rows = n_rows; r->n_cols = n_cols;
    r->R = (double*)quiet_alloc(nb);
    r->d_dest = r->R ? (int32_t*)quiet_alloc(aligned(2 * PARK_PAIRS_MAX * sizeof(int32_t))) : nullptr;
    if (!r->d_dest || hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        emg3d_rows_destroy(r);
        return (int)hipErrorOutOfMemory;
    }
    r->nbytes = nb;
    *out = r;
    return 0;
}

void emg3d_rows_destroy(emg3d_rows_t* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->stream) { (void)hipStreamSynchronize(r->stream); (void)hipStreamDestroy(r->stream); }
    if (r->R) (void)hipFree(r->R);
    if (r->d_dest) (void)hipFree(r->d_dest);
    if (r->chain[0]) (void)hipFree(r->chain[0]);
    if (r->ws) (void)hipFree(r->ws);
    (void)hipGetLastError();
    delete r;
}

int64_t emg3d_rows_bytes(const emg3d_rows_t* r) { return r ? (int64_t)(r->nbytes + r->chain_bytes + r->ws_bytes) : -2; }

int emg3d_rows_set(emg3d_rows_t* r, int64_t i, const double* host) {
    if (!r || !host || i < 0 || i >= r->n_rows) return -2;
    ROWS_TRY(hipSetDevice(r->device));
    return to_device(r, r->R + i * r->n_cols, host, (size_t)r->n_cols * sizeof(double));
}

int emg3d_rows_get(emg3d_rows_t* r, int64_t i, double* host) {
    if (!r || !host || i < 0 || i >= r->n_rows) return -2;
    ROWS_TRY(hipSetDevice(r->device));
    return to_host(r, host, r->R + i * r->n_cols, (size_t)r->n_cols * sizeof(double));
}

int emg3d_rows_set_chain(emg3d_rows_t* r, int64_t n, const double* cx, const double* cy, const double* cz) {
    if (!r || n < 0 || (n > 0 && (!cx || !cy || !cz))) return -2;
    ROWS_TRY(hipSetDevice(r->device));
    if (n != r->chain_n) {
        if (r->chain[0]) { ROWS_TRY(hipStreamSynchronize(r->stream)); (void)hipFree(r->chain[0]); }
        r->chain[0] = r->chain[1] = r->chain[2] = nullptr;
        r->chain_n = 0; r->chain_bytes = 0;
        if (n == 0) return 0;
        const size_t nb = aligned(3 * (size_t)n * sizeof(double));
        r->chain[0] = (double*)quiet_alloc(nb);
        if (!r->chain[0]) return (int)hipErrorOutOfMemory;
        r->chain[1] = r->chain[0] + n; r->chain[2] = r->chain[0] + 2 * n;
        r->chain_n = n; r->chain_bytes = nb;
    }
    const double* src[3] = {cx, cy, cz};
    for (int q = 0; q < 3 && n > 0; ++q) {
        const int st = to_device(r, r->chain[q], src[q], (size_t)n * sizeof(double));
        if (st) return st;
    }
    return 0;
}

int rows_park(emg3d_rows* r, hipStream_t stream, int device, const double* src, i64 pairs, int ndir, int npart, i64 ncells,
              const int32_t* dest, int chain, int sum3) {
    if (!r || !src || !dest || pairs < 1 || pairs > PARK_PAIRS_MAX || (ndir != 1 && ndir != 3) || npart < 1 || npart > 2 || ncells < 1)
        return -2;
    if (device != r->device || (sum3 && ndir != 3) || r->n_cols != (sum3 ? 1 : ndir) * ncells) return -2;
    if (chain && r->chain_n != ncells) return -2;
    bool any = false;
    for (i64 p = 0; p < pairs; ++p) {
        if (dest[p] >= r->n_rows) return -2;
        any = any || dest[p] >= 0;
    }
    if (!any) return 0;
    ROWS_TRY(hipStreamSynchronize(r->stream));          // (the store's own products are done with the rows about to change)
    ROWS_TRY(hipMemcpyAsync(r->d_dest, dest, (size_t)pairs * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    const double* c[3] = {chain ? r->chain[0] : nullptr, chain ? r->chain[1] : nullptr, chain ? r->chain[2] : nullptr};
    hipLaunchKernelGGL(k_rows_park, dim3((unsigned)((ncells + 255) / 256), (unsigned)pairs), dim3(256), 0, stream, r->R, r->n_cols, src,
                       ndir, npart, ncells, (const int32_t*)r->d_dest, c[0], c[1], c[2], sum3);
    return launched();
}

int rows_fill_check(const emg3d_rows* r, int device, i64 pairs, int ndir, int npart, i64 ncells, const int32_t* dest_re,
                    const int32_t* dest_im, int chain, int sum3) {
    if (!r || !dest_re || pairs < 1 || pairs > PARK_PAIRS_MAX || (ndir != 1 && ndir != 3) || npart < 1 || npart > 2 || ncells < 1)
        return -2;
    if (dest_im && npart != 2) return -2;
    if (device != r->device || (sum3 && ndir != 3) || r->n_cols != (sum3 ? 1 : ndir) * ncells) return -2;
    if (chain && r->chain_n != ncells) return -2;
    std::vector<int32_t> named;
    named.reserve((size_t)(2 * pairs));
    for (const int32_t* dest : {dest_re, dest_im})
        for (i64 p = 0; dest && p < pairs; ++p) {
            if (dest[p] >= r->n_rows) return -2;
            if (dest[p] >= 0) named.push_back(dest[p]);
        }
    if (named.empty()) return -2;
    std::sort(named.begin(), named.end());
    return std::adjacent_find(named.begin(), named.end()) == named.end() ? 0 : -2;
}

template <class T>
int rows_fill(emg3d_rows* r, hipStream_t stream, int device, const RowsFillFields<T>& f, int split, const int32_t* dest_re,
              const int32_t* dest_im, int chain, int sum3) {
    if (!f.fwd || !f.adj || f.nsys < 1 || f.nsys > 64) return -2;
    const unsigned long long clip = f.nsys < 64 ? (1ull << f.nsys) - 1ull : ~0ull;
    const i64 pairs = (i64)__builtin_popcountll(f.use_fwd & clip) * (i64)__builtin_popcountll(f.use_adj & clip);
    const i64 ncells = f.nC[0] * f.nC[1] * f.nC[2];
    const int st = rows_fill_check(r, device, pairs, split ? 3 : 1, (int)(sizeof(T) / sizeof(double)), ncells, dest_re, dest_im, chain, sum3);
    if (st) return st;
    ROWS_TRY(hipStreamSynchronize(r->stream));          // (the store's own products are done with the rows about to change)
    ROWS_TRY(hipMemcpyAsync(r->d_dest, dest_re, (size_t)pairs * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    if (dest_im)
        ROWS_TRY(hipMemcpyAsync(r->d_dest + PARK_PAIRS_MAX, dest_im, (size_t)pairs * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    RowsFillArgs a;
    a.R = r->R; a.n_cols = r->n_cols;
    a.dest_re = r->d_dest; a.dest_im = dest_im ? r->d_dest + PARK_PAIRS_MAX : nullptr;
    for (int q = 0; q < 3; ++q) a.c[q] = chain ? r->chain[q] : nullptr;
    a.sum3 = sum3;
    const dim3 grid((unsigned)((ncells + 255) / 256));
    if (split)
        hipLaunchKernelGGL((k_sens_rows_fill<T, true>), grid, dim3(256), 0, stream, f.nC[0], f.nC[1], f.nC[2], f.fl, f.fwd, f.adj, f.nE,
                           f.nsys, f.use_fwd, f.use_adj, f.sr, f.si, f.h[0], f.h[1], f.h[2], a);
    else
        hipLaunchKernelGGL((k_sens_rows_fill<T, false>), grid, dim3(256), 0, stream, f.nC[0], f.nC[1], f.nC[2], f.fl, f.fwd, f.adj, f.nE,
                           f.nsys, f.use_fwd, f.use_adj, f.sr, f.si, f.h[0], f.h[1], f.h[2], a);
    return launched();
}
template int rows_fill<double>(emg3d_rows*, hipStream_t, int, const RowsFillFields<double>&, int, const int32_t*, const int32_t*, int, int);
template int rows_fill<c128>(emg3d_rows*, hipStream_t, int, const RowsFillFields<c128>&, int, const int32_t*, const int32_t*, int, int);

int emg3d_rows_gram(emg3d_rows_t* r, const double* cm, double* G) {
    if (!r || !G) return -2;
    ROWS_TRY(hipSetDevice(r->device));
    const RowsGramPlan p = rows_gram_plan(r->n_rows, r->n_cols);
    const RowsGramBatch gb = rows_gram_batch(r->n_rows, r->n_cols);
    const size_t per_job = (size_t)gb.per_job;
    const i64 batch = gb.batch;
    double* w[3];       // slab partials, G, cm
    if (!carve(r, {per_job / sizeof(double) * (size_t)batch, (size_t)r->n_rows * (size_t)r->n_rows, cm ? (size_t)r->n_cols : 1}, w))
        return (int)hipErrorOutOfMemory;
    double *part = w[0], *dG = w[1], *dcm = w[2];
    if (cm) { const int st = to_device(r, dcm, cm, (size_t)r->n_cols * sizeof(double)); if (st) return st; }
    for (i64 job0 = 0; job0 < p.njobs; job0 += batch) {
        const unsigned nj = (unsigned)std::min<i64>(batch, p.njobs - job0);
        hipLaunchKernelGGL(k_rows_gram, dim3((unsigned)p.nslab, nj), dim3(64 * ROWS_WAVES), 0, r->stream, (const double*)r->R,
                           cm ? (const double*)dcm : nullptr, part, r->n_rows, r->n_cols, p.slab, p.nslab, job0);
        hipLaunchKernelGGL(k_rows_gram_reduce, dim3(64, nj), dim3(256), 0, r->stream, dG, (const double*)part, r->n_rows,
                           p.nslab, job0);
    }
    const int st = launched();
    if (st) { (void)hipStreamSynchronize(r->stream); return st; }
    return to_host(r, G, dG, (size_t)r->n_rows * (size_t)r->n_rows * sizeof(double));
}

int emg3d_rows_matvec(emg3d_rows_t* r, const double* v, double* out) {
    if (!r || !v || !out) return -2;
    ROWS_TRY(hipSetDevice(r->device));
    const RowsGramPlan p = rows_gram_plan(r->n_rows, r->n_cols);
    if (r->n_rows * p.nslab > 0x7fffffff) return -2;
    double* w[3];       // v, slab partials, result
    if (!carve(r, {(size_t)r->n_cols, (size_t)(r->n_rows * p.nslab), (size_t)r->n_rows}, w)) return (int)hipErrorOutOfMemory;
    double *dv = w[0], *part = w[1], *dout = w[2];
    int st = to_device(r, dv, v, (size_t)r->n_cols * sizeof(double));
    if (st) return st;
    hipLaunchKernelGGL(k_rows_matvec, dim3((unsigned)(r->n_rows * p.nslab)), dim3(256), 0, r->stream, (const double*)r->R,
                       (const double*)dv, part, r->n_cols, p.slab, p.nslab);
    hipLaunchKernelGGL(k_rows_matvec_reduce, dim3((unsigned)((r->n_rows + 255) / 256)), dim3(256), 0, r->stream, dout,
                       (const double*)part, r->n_rows, p.nslab);
    st = launched();
    if (st) { (void)hipStreamSynchronize(r->stream); return st; }
    return to_host(r, out, dout, (size_t)r->n_rows * sizeof(double));
}

int emg3d_rows_rmatvec(emg3d_rows_t* r, const double* y, const double* cm, double* out) {
    if (!r || !y || !out) return -2;
    ROWS_TRY(hipSetDevice(r->device));
    if ((r->n_cols + 255) / 256 > 0x7fffffff) return -2;
    double* w[3];       // y, cm, result
    if (!carve(r, {(size_t)r->n_rows, cm ? (size_t)r->n_cols : 1, (size_t)r->n_cols}, w)) return (int)hipErrorOutOfMemory;
    double *dy = w[0], *dcm = w[1], *dout = w[2];
    int st = to_device(r, dy, y, (size_t)r->n_rows * sizeof(double));
    if (!st && cm) st = to_device(r, dcm, cm, (size_t)r->n_cols * sizeof(double));
    if (st) return st;
    hipLaunchKernelGGL(k_rows_rmatvec, dim3((unsigned)((r->n_cols + 255) / 256)), dim3(256), 0, r->stream, (const double*)r->R,
                       (const double*)dy, cm ? (const double*)dcm : nullptr, dout, r->n_rows, r->n_cols);
    st = launched();
    if (st) { (void)hipStreamSynchronize(r->stream); return st; }
    return to_host(r, out, dout, (size_t)r->n_cols * sizeof(double));
}

int emg3d_rows_project_plan(int64_t n_rows, int64_t m, int64_t n_cols, int64_t* out) {
    if (n_rows < 1 || m < 1 || n_cols < 1 || !out) return -2;
    const RowsProjectPlan p = rows_project_plan(n_rows, m, n_cols);
    out[0] = PROJ_BLOCK; out[1] = PROJ_COLS; out[2] = PROJ_KSTEP; out[3] = p.passes; out[4] = p.wg; out[5] = p.lds_bytes;
    out[6] = p.panels; out[7] = p.last_rows;
    return 0;
}

int emg3d_rows_project(emg3d_rows_t* r, const double* M, int64_t m, emg3d_rows_t* dst) {
    if (!r || !M || !dst || m < 1 || dst == r || dst->device != r->device || dst->n_rows != m || dst->n_cols != r->n_cols) return -2;
    if (dst->R == r->R || m > (((int64_t)1 << 59) / r->n_rows)) return -2;
    const RowsProjectPlan p = rows_project_plan(r->n_rows, m, r->n_cols);
    if (p.panels > (i64)0x7fffffff) return -2;
    ROWS_TRY(hipSetDevice(r->device));
    const size_t nm = (size_t)m * (size_t)r->n_rows;
    double* w[1];       // M transposed
    if (!carve(r, {nm}, w)) return (int)hipErrorOutOfMemory;
    double* mt = new (std::nothrow) double[nm];
    if (!mt) return -3;
    for (i64 i = 0; i < m; ++i)
        for (i64 k = 0; k < r->n_rows; ++k) mt[k * m + i] = M[i * r->n_rows + k];
    int st = to_device(r, w[0], mt, nm * sizeof(double));       // (synchronised: mt may go)
    delete[] mt;
    if (st) return st;
    for (i64 b = 0; b < p.passes; ++b) {
        const i64 row0 = b * PROJ_BLOCK;
        const i64 cover = b + 1 < p.passes ? PROJ_BLOCK : p.last_rows;
        const dim3 grid((unsigned)p.panels), block(PROJ_THREADS);
        if (cover == 32)
            hipLaunchKernelGGL(k_rows_project<1>, grid, block, 0, r->stream, (const double*)r->R, (const double*)w[0], dst->R, r->n_rows, m, r->n_cols, row0);
        else if (cover == 64)
            hipLaunchKernelGGL(k_rows_project<2>, grid, block, 0, r->stream, (const double*)r->R, (const double*)w[0], dst->R, r->n_rows, m, r->n_cols, row0);
        else if (cover == 128)
            hipLaunchKernelGGL(k_rows_project<4>, grid, block, 0, r->stream, (const double*)r->R, (const double*)w[0], dst->R, r->n_rows, m, r->n_cols, row0);
        else
            hipLaunchKernelGGL(k_rows_project<8>, grid, block, 0, r->stream, (const double*)r->R, (const double*)w[0], dst->R, r->n_rows, m, r->n_cols, row0);
    }
    st = launched();
    if (st) { (void)hipStreamSynchronize(r->stream); return st; }
    ROWS_TRY(hipStreamSynchronize(r->stream));
    return 0;
}

int emg3d_rows_colsumsq(emg3d_rows_t* r, const double* s, double* out) {
    if (!r || !out) return -2;
    ROWS_TRY(hipSetDevice(r->device));
    if ((r->n_cols + 255) / 256 > 0x7fffffff) return -2;
    double* w[2];       // s, result
    if (!carve(r, {s ? (size_t)r->n_rows : 1, (size_t)r->n_cols}, w)) return (int)hipErrorOutOfMemory;
    double *ds = w[0], *dout = w[1];
    int st = s ? to_device(r, ds, s, (size_t)r->n_rows * sizeof(double)) : 0;
    if (st) return st;
    const dim3 grid((unsigned)((r->n_cols + 255) / 256));
    if (s) hipLaunchKernelGGL(k_rows_colsumsq<true>, grid, dim3(256), 0, r->stream, (const double*)r->R, (const double*)ds, dout, r->n_rows, r->n_cols);
    else hipLaunchKernelGGL(k_rows_colsumsq<false>, grid, dim3(256), 0, r->stream, (const double*)r->R, (const double*)nullptr, dout, r->n_rows, r->n_cols);
    st = launched();
    if (st) { (void)hipStreamSynchronize(r->stream); return st; }
    return to_host(r, out, dout, (size_t)r->n_cols * sizeof(double));
}

// ====================================================================================================== smoothing covariance
int emg3d_rows_smooth_plan(int64_t nx, int64_t ny, int64_t nz, int axis, int64_t* out) {
    if (nx < 1 || ny < 1 || nz < 1 || axis < 0 || axis > 2 || !out) return -2;
    const RowsSmoothPlan p = rows_smooth_plan(nx, ny, nz, axis);
    out[0] = p.path; out[1] = p.lines; out[2] = p.lds_bytes; out[3] = p.wg; out[4] = SMOOTH_LINES_MIN; out[5] = p.nl;
    return 0;
}

namespace {
// the factors of an axis come as three arrays or as none
bool smooth_factors_ok(const double* const (&h)[3][3]) {
    for (int ax = 0; ax < 3; ++ax)
        if ((h[ax][0] != nullptr) != (h[ax][1] != nullptr) || (h[ax][0] != nullptr) != (h[ax][2] != nullptr)) return false;
    return true;
}
}  // namespace

int emg3d_smooth3d(int device, int64_t n_arrays, int64_t nx, int64_t ny, int64_t nz, const double* scale, const double* lo_x,
                   const double* cp_x, const double* inv_x, const double* lo_y, const double* cp_y, const double* inv_y,
                   const double* lo_z, const double* cp_z, const double* inv_z, int passes, int scale_after, double* data) {
    const double* const h[3][3] = {{lo_x, cp_x, inv_x}, {lo_y, cp_y, inv_y}, {lo_z, cp_z, inv_z}};
    if (n_arrays < 1 || nx < 1 || ny < 1 || nz < 1 || passes < 1 || !data || !smooth_factors_ok(h)) return -2;
    if (ny > (((int64_t)1 << 59) / nx) || nz > (((int64_t)1 << 59) / (nx * ny)) || n_arrays > (((int64_t)1 << 59) / (nx * ny * nz))) return -2;
    HIP_TRY(hipSetDevice(device));
    const i64 dims[3] = {nx, ny, nz};
    const size_t cells = (size_t)(nx * ny * nz), total = cells * (size_t)n_arrays;
    double *d_data = nullptr, *d_w = nullptr, *d_f = nullptr;
    DEV_ALLOC(d_data, total * sizeof(double));
    DEV_ALLOC(d_w, (scale ? cells : 1) * sizeof(double));
    DEV_ALLOC(d_f, (size_t)3 * (size_t)(nx + ny + nz) * sizeof(double));
    HIP_TRY(hipMemcpy(d_data, data, total * sizeof(double), hipMemcpyHostToDevice));
    if (scale) HIP_TRY(hipMemcpy(d_w, scale, cells * sizeof(double), hipMemcpyHostToDevice));
    SmoothFactors f;
    double* next = d_f;
    for (int ax = 0; ax < 3; ++ax)
        for (int q = 0; q < 3 && h[ax][0]; ++q) {
            HIP_TRY(hipMemcpy(next, h[ax][q], (size_t)dims[ax] * sizeof(double), hipMemcpyHostToDevice));
            f.p[ax][q] = next;
            next += dims[ax];
        }
    const int st = smooth_run(nullptr, d_data, n_arrays, nx, ny, nz, 1, scale ? d_w : nullptr, f, passes, scale_after);
    HIP_TRY(hipDeviceSynchronize());
    if (st) return st;
    HIP_TRY(hipMemcpy(data, d_data, total * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

namespace {
// L^T (scale_after == 0) or L (1) on every row of a store, in place: the body of emg3d_rows_smooth and emg3d_rows_smooth_l
int rows_smooth(emg3d_rows* r, i64 nx, i64 ny, i64 nz, int planes, const double* scale, const double* const (&h)[3][3], int passes,
                int scale_after) {
    if (!r || nx < 1 || ny < 1 || nz < 1 || planes < 1 || passes < 1 || !smooth_factors_ok(h)) return -2;
    // (no product before it is known to fit: nx ny nz <= n_cols, and planes divides n_cols)
    if (nx > r->n_cols || ny > r->n_cols / nx || nz > r->n_cols / (nx * ny)) return -2;
    if (r->n_cols % planes != 0 || nx * ny * nz != r->n_cols / planes) return -2;
    if (r->n_rows > (((int64_t)1 << 59) / planes)) return -2;           // (the number of arrays, n_rows * planes)
    ROWS_TRY(hipSetDevice(r->device));
    const i64 dims[3] = {nx, ny, nz};
    size_t sizes[10] = {scale ? (size_t)r->n_cols : 1};
    for (int ax = 0; ax < 3; ++ax)
        for (int q = 0; q < 3; ++q) sizes[1 + 3 * ax + q] = h[ax][0] ? (size_t)dims[ax] : 1;
    double* w[10];      // scale, then lo, cp, inv per axis
    if (!carve(r, sizes, w)) return (int)hipErrorOutOfMemory;
    if (scale) { const int st = to_device(r, w[0], scale, (size_t)r->n_cols * sizeof(double)); if (st) return st; }
    SmoothFactors f;
    for (int ax = 0; ax < 3; ++ax)
        for (int q = 0; q < 3 && h[ax][0]; ++q) {
            const int st = to_device(r, w[1 + 3 * ax + q], h[ax][q], (size_t)dims[ax] * sizeof(double));
            if (st) return st;
            f.p[ax][q] = w[1 + 3 * ax + q];
        }
    const int st = smooth_run(r->stream, r->R, r->n_rows * planes, nx, ny, nz, planes, scale ? w[0] : nullptr, f, passes, scale_after);
    if (st) { (void)hipStreamSynchronize(r->stream); return st; }
    ROWS_TRY(hipStreamSynchronize(r->stream));
    return 0;
}
}  // namespace

int emg3d_rows_smooth(emg3d_rows_t* r, int64_t nx, int64_t ny, int64_t nz, int planes, const double* scale, const double* lo_x,
                      const double* cp_x, const double* inv_x, const double* lo_y, const double* cp_y, const double* inv_y,
                      const double* lo_z, const double* cp_z, const double* inv_z, int passes) {
    const double* const h[3][3] = {{lo_x, cp_x, inv_x}, {lo_y, cp_y, inv_y}, {lo_z, cp_z, inv_z}};
    return rows_smooth(r, nx, ny, nz, planes, scale, h, passes, 0);
}

int emg3d_rows_smooth_l(emg3d_rows_t* r, int64_t nx, int64_t ny, int64_t nz, int planes, const double* scale, const double* lo_x,
                        const double* cp_x, const double* inv_x, const double* lo_y, const double* cp_y, const double* inv_y,
                        const double* lo_z, const double* cp_z, const double* inv_z, int passes) {
    const double* const h[3][3] = {{lo_x, cp_x, inv_x}, {lo_y, cp_y, inv_y}, {lo_z, cp_z, inv_z}};
    return rows_smooth(r, nx, ny, nz, planes, scale, h, passes, 1);
}

int emg3d_rows_clone(emg3d_rows_t* r, emg3d_rows_t** out) {
    if (!r || !out) return -2;
    const int st = emg3d_rows_create(r->device, r->n_rows, r->n_cols, out);     // (the same memory check, the same answers)
    if (st) return st;
    emg3d_rows* c = *out;
    const hipError_t cp = hipMemcpyAsync(c->R, r->R, (size_t)r->n_rows * (size_t)r->n_cols * sizeof(double), hipMemcpyDeviceToDevice, r->stream);
    const hipError_t sy = cp == hipSuccess ? hipStreamSynchronize(r->stream) : cp;
    if (sy != hipSuccess) {
        (void)hipGetLastError();
        emg3d_rows_destroy(c);
        *out = nullptr;
        return (int)sy;
    }
    return 0;
}
