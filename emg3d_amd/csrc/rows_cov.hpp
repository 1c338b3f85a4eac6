// Smoothing model covariance of a row store (csrc/rows.hip includes this): tridiagonal line solves along x, y and z over
// n_arrays 3-D arrays of nx x ny x nz doubles (x fastest), in place -- emg3d_smooth3d, emg3d_rows_smooth.  gfx950 only.
//
//   k_rows_smooth_lines   y- and z-lines: one thread per line, adjacent threads adjacent in x; the line sits in LDS as [i][thread]
//   k_rows_smooth_xtile   x-lines: a tile of lines loaded along x into LDS rows of odd length, one thread walks each row
//   k_rows_smooth_hbm     any axis, any length: one thread per line, in place through HBM (the forward sweep overwrites, the backward
//                         sweep reads again)
//   k_rows_smooth_scale   a = w * a where no axis is active
//
// One line a[0 .. n-1] with the factors lo, cp, inv of its axis (maps.SmoothingCovariance computes them on the host):
//   a[0] = a[0] * inv[0];   a[i] = (a[i] - lo[i] * a[i-1]) * inv[i], i = 1 .. n-1;   a[i] = a[i] - cp[i] * a[i+1], i = n-2 .. 0
// -- sequential Thomas, every operation rounded once (no contraction): the result equals that loop in numpy bit for bit, whichever
// kernel ran it.  `passes` solves in a row are done while the line is on chip; the scale w multiplies on the way in (w_pre, the
// first active axis of L^T) or on the way out (w_post, the last active axis of L), so that per axis every element is read once and
// written once.
#pragma once
#include "common.hpp"

// ---- geometry (host arithmetic; exported as emg3d_rows_smooth_plan) ------------------------------------------------------------------
constexpr i64 SMOOTH_LDS_MAX = 160 * 1024;      // LDS bytes of a workgroup
constexpr int SMOOTH_LINES = 64;                // lines (= threads) of a workgroup ...
constexpr int SMOOTH_LINES_MIN = 32;            // ... or, where 64 lines do not fit the LDS, this many: 256 contiguous bytes per step
constexpr int SMOOTH_HBM_LINES = 64;            // lines of a workgroup of k_rows_smooth_hbm

struct RowsSmoothPlan {
    int path = 0;               // 0: the line is resident in LDS, 1: through HBM
    i64 n = 0;                  // length of a line
    i64 nl = 0;                 // lines of one array
    i64 lines = 0;              // lines per workgroup
    i64 ld = 0;                 // path 0: LDS doubles per line (x: n | 1, the padded row; y, z: n)
    i64 lds_bytes = 0;
    i64 wg = 0;                 // workgroups per array (a workgroup never spans two arrays: the plan does not depend on their number)
};
inline RowsSmoothPlan rows_smooth_plan(i64 nx, i64 ny, i64 nz, int axis) {
    RowsSmoothPlan p;
    p.n = axis == 0 ? nx : axis == 1 ? ny : nz;
    p.nl = axis == 0 ? ny * nz : axis == 1 ? nx * nz : nx * ny;
    p.ld = axis == 0 ? (p.n | 1) : p.n;
    const i64 per_line = p.ld * (i64)sizeof(double);
    if (per_line * SMOOTH_LINES <= SMOOTH_LDS_MAX) p.lines = SMOOTH_LINES;
    else if (per_line * SMOOTH_LINES_MIN <= SMOOTH_LDS_MAX) p.lines = SMOOTH_LINES_MIN;
    else { p.path = 1; p.lines = SMOOTH_HBM_LINES; }
    p.lds_bytes = p.path ? 0 : per_line * p.lines;
    p.wg = (p.nl + p.lines - 1) / p.lines;
    return p;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------
struct SmoothArgs {
    double* data;                       // n_arrays arrays of `cells` doubles, back to back
    const double *lo, *cp, *inv;        // the factors of this axis, n doubles each
    const double *w_pre, *w_post;       // wplanes * cells doubles each, or nullptr: array q takes plane q % wplanes
    i64 cells, wplanes;
    i64 n, stride;                      // a line: n elements, `stride` doubles apart
    i64 ninner, os;                     // line l of an array starts at (l / ninner) * os + l % ninner
    i64 nl, wg;                         // lines and workgroups per array
    int passes;
};

extern __shared__ __attribute__((aligned(16))) char smooth_lds[];

// `passes` solves of the line z[0], z[LD], .., z[(n - 1) LD] in LDS.  Per chunk of SMOOTH_U steps the line's values and the factors
// are loaded first -- none depends on the recurrence --, then the subtract-multiply chain runs on registers.
constexpr int SMOOTH_U = 8;
template <int LD>
__device__ __forceinline__ void smooth_line(double* z, int n, const double* __restrict__ lo, const double* __restrict__ cp,
                                            const double* __restrict__ inv, int passes) {
#pragma clang fp contract(off)
    for (int p = 0; p < passes; ++p) {
        double prev = z[0] * inv[0];
        z[0] = prev;
        int i = 1;
        for (; i + SMOOTH_U <= n; i += SMOOTH_U) {
            double v[SMOOTH_U], l[SMOOTH_U], d[SMOOTH_U];
#pragma unroll
            for (int k = 0; k < SMOOTH_U; ++k) { v[k] = z[(i + k) * LD]; l[k] = lo[i + k]; d[k] = inv[i + k]; }
#pragma unroll
            for (int k = 0; k < SMOOTH_U; ++k) { prev = (v[k] - l[k] * prev) * d[k]; z[(i + k) * LD] = prev; }
        }
        for (; i < n; ++i) { prev = (z[i * LD] - lo[i] * prev) * inv[i]; z[i * LD] = prev; }
        i = n - 2;
        for (; i - (SMOOTH_U - 1) >= 0; i -= SMOOTH_U) {
            double v[SMOOTH_U], c[SMOOTH_U];
#pragma unroll
            for (int k = 0; k < SMOOTH_U; ++k) { v[k] = z[(i - k) * LD]; c[k] = cp[i - k]; }
#pragma unroll
            for (int k = 0; k < SMOOTH_U; ++k) { prev = v[k] - c[k] * prev; z[(i - k) * LD] = prev; }
        }
        for (; i >= 0; --i) { prev = z[i * LD] - cp[i] * prev; z[i * LD] = prev; }
    }
}

// grid (wg * n_arrays), LPW threads, n * LPW * 8 bytes of dynamic LDS.  Thread t owns column t of the [i][t] image: no barrier.
template <int LPW>
__global__ void __launch_bounds__(LPW) k_rows_smooth_lines(SmoothArgs a) {
#pragma clang fp contract(off)
    const i64 arr = (i64)(blockIdx.x / (unsigned)a.wg);
    const i64 l = (i64)(blockIdx.x % (unsigned)a.wg) * LPW + threadIdx.x;
    if (l >= a.nl) return;
    i64 inner, outer;
    unlin2(l, a.ninner, inner, outer);
    const i64 c0 = outer * a.os + inner;
    double* g = a.data + arr * a.cells + c0;
    const i64 wo = (arr % a.wplanes) * a.cells + c0;
    double* z = (double*)smooth_lds + threadIdx.x;
    const int n = (int)a.n;
    const i64 st = a.stride;
    if (a.w_pre) {
        const double* w = a.w_pre + wo;
#pragma unroll 16
        for (int i = 0; i < n; ++i) z[i * LPW] = w[i * st] * g[i * st];
    } else {
#pragma unroll 32
        for (int i = 0; i < n; ++i) z[i * LPW] = g[i * st];
    }
    smooth_line<LPW>(z, n, a.lo, a.cp, a.inv, a.passes);
    if (a.w_post) {
        const double* w = a.w_post + wo;
#pragma unroll 8
        for (int i = 0; i < n; ++i) g[i * st] = w[i * st] * z[i * LPW];
    } else {
#pragma unroll 8
        for (int i = 0; i < n; ++i) g[i * st] = z[i * LPW];
    }
}

// grid (wg * n_arrays), LT threads, LT * (n | 1) * 8 bytes of dynamic LDS.  The LT lines of a tile are one contiguous piece of the
// array: element e of it is read by thread e % LT (coalesced) into row e / n of the LDS image; the odd row length puts the rows of
// the 32 lanes of a half wave on 32 different banks when every thread walks its own row.
template <int LT>
__global__ void __launch_bounds__(LT) k_rows_smooth_xtile(SmoothArgs a) {
#pragma clang fp contract(off)
    const i64 arr = (i64)(blockIdx.x / (unsigned)a.wg);
    const i64 l0 = (i64)(blockIdx.x % (unsigned)a.wg) * LT;
    const unsigned n = (unsigned)a.n, ld = n | 1u;
    const unsigned nlt = (unsigned)(a.nl - l0 < LT ? a.nl - l0 : LT);
    const unsigned cnt = nlt * n;
    const i64 c0 = l0 * a.n;
    double* g = a.data + arr * a.cells + c0;
    const i64 wo = (arr % a.wplanes) * a.cells + c0;
    double* z = (double*)smooth_lds;
    if (a.w_pre) {
        const double* w = a.w_pre + wo;
#pragma unroll 8
        for (unsigned e = threadIdx.x; e < cnt; e += LT) { const unsigned r = e / n; z[r * ld + (e - r * n)] = w[e] * g[e]; }
    } else {
#pragma unroll 16
        for (unsigned e = threadIdx.x; e < cnt; e += LT) { const unsigned r = e / n; z[r * ld + (e - r * n)] = g[e]; }
    }
    __syncthreads();
    if (threadIdx.x < nlt) smooth_line<1>(z + threadIdx.x * ld, (int)n, a.lo, a.cp, a.inv, a.passes);
    __syncthreads();
    if (a.w_post) {
        const double* w = a.w_post + wo;
#pragma unroll 4
        for (unsigned e = threadIdx.x; e < cnt; e += LT) { const unsigned r = e / n; g[e] = w[e] * z[r * ld + (e - r * n)]; }
    } else {
#pragma unroll 4
        for (unsigned e = threadIdx.x; e < cnt; e += LT) { const unsigned r = e / n; g[e] = z[r * ld + (e - r * n)]; }
    }
}

// grid (wg * n_arrays), SMOOTH_HBM_LINES threads: the fallback for a line that no LDS holds.  64-bit offsets; w_pre multiplies what
// the first forward sweep reads, w_post what the last backward sweep writes (the chain goes on with the unscaled value).
__global__ void __launch_bounds__(SMOOTH_HBM_LINES) k_rows_smooth_hbm(SmoothArgs a) {
#pragma clang fp contract(off)
    const i64 arr = (i64)(blockIdx.x / (unsigned)a.wg);
    const i64 l = (i64)(blockIdx.x % (unsigned)a.wg) * SMOOTH_HBM_LINES + threadIdx.x;
    if (l >= a.nl) return;
    i64 inner, outer;
    unlin2(l, a.ninner, inner, outer);
    const i64 c0 = outer * a.os + inner;
    double* g = a.data + arr * a.cells + c0;
    const i64 wo = (arr % a.wplanes) * a.cells + c0;
    const i64 n = a.n, st = a.stride;
    const double* __restrict__ lo = a.lo;
    const double* __restrict__ cp = a.cp;
    const double* __restrict__ inv = a.inv;
    for (int p = 0; p < a.passes; ++p) {
        const double* wi = (p == 0 && a.w_pre) ? a.w_pre + wo : nullptr;
        const double* wq = (p == a.passes - 1 && a.w_post) ? a.w_post + wo : nullptr;
        double prev = (wi ? wi[0] * g[0] : g[0]) * inv[0];
        g[0] = prev;
        for (i64 i = 1; i < n; ++i) {
            const double v = wi ? wi[i * st] * g[i * st] : g[i * st];
            prev = (v - lo[i] * prev) * inv[i];
            g[i * st] = prev;
        }
        if (wq) g[(n - 1) * st] = wq[(n - 1) * st] * prev;
        for (i64 i = n - 2; i >= 0; --i) {
            prev = g[i * st] - cp[i] * prev;
            g[i * st] = wq ? wq[i * st] * prev : prev;
        }
    }
}

// grid (ceil(total / 256)), 256 threads: a = w * a, array q with plane q % wplanes of w
__global__ void __launch_bounds__(256) k_rows_smooth_scale(double* __restrict__ data, const double* __restrict__ w, i64 total, i64 wlen) {
#pragma clang fp contract(off)
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    data[e] = w[e % wlen] * data[e];
}

// ---- launches ------------------------------------------------------------------------------------------------------------------------
// L^T (scale_after == 0: w first) or L (w last) on n_arrays arrays on the device, on `stream`; w: wplanes * cells doubles (device)
// or nullptr; f.p[axis] = {lo, cp, inv} (device), all nullptr: the axis is skipped, as is one of length 1.  0, a HIP error, or -2 (a
// launch of more than 2^31 - 1 workgroups).
struct SmoothFactors {
    const double* p[3][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
};
inline int smooth_run(hipStream_t stream, double* data, i64 n_arrays, i64 nx, i64 ny, i64 nz, i64 wplanes, const double* w,
                      const SmoothFactors& f, int passes, int scale_after) {
    const i64 dims[3] = {nx, ny, nz};
    const i64 cells = nx * ny * nz;
    int active[3], na = 0;
    for (int ax = 0; ax < 3; ++ax)
        if (f.p[ax][0] && dims[ax] > 1) active[na++] = ax;
    for (int k = 0; k < na; ++k)
        if (rows_smooth_plan(nx, ny, nz, active[k]).wg > (i64)0x7fffffff / n_arrays) return -2;
    if (na == 0) {
        if (!w) return 0;
        const i64 total = n_arrays * cells, blocks = (total + 255) / 256;
        if (blocks > (i64)0x7fffffff) return -2;
        hipLaunchKernelGGL(k_rows_smooth_scale, dim3((unsigned)blocks), dim3(256), 0, stream, data, w, total, wplanes * cells);
        const hipError_t st = hipGetLastError();
        return st == hipSuccess ? 0 : (int)st;
    }
    for (int k = 0; k < na; ++k) {
        const int ax = active[k];
        const RowsSmoothPlan p = rows_smooth_plan(nx, ny, nz, ax);
        SmoothArgs a;
        a.data = data;
        a.lo = f.p[ax][0]; a.cp = f.p[ax][1]; a.inv = f.p[ax][2];
        a.w_pre = (w && !scale_after && k == 0) ? w : nullptr;
        a.w_post = (w && scale_after && k == na - 1) ? w : nullptr;
        a.cells = cells; a.wplanes = wplanes;
        a.n = p.n;
        a.stride = ax == 0 ? 1 : ax == 1 ? nx : nx * ny;
        a.ninner = ax == 0 ? 1 : ax == 1 ? nx : nx * ny;
        a.os = ax == 0 ? nx : ax == 1 ? nx * ny : 0;
        a.nl = p.nl; a.wg = p.wg;
        a.passes = passes;
        const dim3 grid((unsigned)(p.wg * n_arrays));
        const size_t lds = (size_t)p.lds_bytes;
        const void* fn = nullptr;
        if (p.path == 0) {
            if (ax == 0) fn = p.lines == SMOOTH_LINES ? (const void*)&k_rows_smooth_xtile<SMOOTH_LINES> : (const void*)&k_rows_smooth_xtile<SMOOTH_LINES_MIN>;
            else fn = p.lines == SMOOTH_LINES ? (const void*)&k_rows_smooth_lines<SMOOTH_LINES> : (const void*)&k_rows_smooth_lines<SMOOTH_LINES_MIN>;
            // (more than 64 KiB of dynamic LDS must be asked for, per device; the call is cheap beside a launch over the store)
            if (lds > (size_t)64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMOOTH_LDS_MAX) != hipSuccess) {
                const hipError_t st = hipGetLastError();
                return st == hipSuccess ? (int)hipErrorInvalidValue : (int)st;
            }
        }
        if (p.path == 1) hipLaunchKernelGGL(k_rows_smooth_hbm, grid, dim3(SMOOTH_HBM_LINES), 0, stream, a);
        else if (ax == 0 && p.lines == SMOOTH_LINES) hipLaunchKernelGGL(k_rows_smooth_xtile<SMOOTH_LINES>, grid, dim3(SMOOTH_LINES), lds, stream, a);
        else if (ax == 0) hipLaunchKernelGGL(k_rows_smooth_xtile<SMOOTH_LINES_MIN>, grid, dim3(SMOOTH_LINES_MIN), lds, stream, a);
        else if (p.lines == SMOOTH_LINES) hipLaunchKernelGGL(k_rows_smooth_lines<SMOOTH_LINES>, grid, dim3(SMOOTH_LINES), lds, stream, a);
        else hipLaunchKernelGGL(k_rows_smooth_lines<SMOOTH_LINES_MIN>, grid, dim3(SMOOTH_LINES_MIN), lds, stream, a);
        const hipError_t st = hipGetLastError();
        if (st != hipSuccess) return (int)st;
    }
    return 0;
}
