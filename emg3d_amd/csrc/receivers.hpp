// Receiver extraction on the device: fields.get_receiver_response (reference emg3d/fields.py:733-817) and
// maps.interp3d (reference emg3d/maps.py:179-276; mode='constant').
//
// The cubic branch of interp3d is SciPy in the reference (maps.py:257-272): interp1d(kind='cubic') -- the
// not-a-knot cubic spline through (points[i], i), extrapolated -- turns coordinates into fractional indices
// (O(n) host work, notaknot_index_coords below), and ndimage.map_coordinates(order=3, mode='constant', cval)
// interpolates: a separable cubic B-spline prefilter over the WHOLE array (pole sqrt(3) - 2, mirror boundary
// initialisation; k_spline_filter_axis: one recursion per line, three passes) followed by a 4 x 4 x 4 weighted
// sum per point (k_spline_eval); points outside [0, n-1] get cval.  The linear branch is
// RegularGridInterpolator(method='linear', bounds_error=False, fill_value) (k_linear_eval).
//
// With the field resident in HBM only the responses (16 bytes per receiver) cross PCIe / xGMI instead of the
// field (102 MB at 128^3): SURVEY 8f rank 3.
#pragma once
#include <cmath>
#include <vector>
#include "common.hpp"

#define EMG_RCV_BLOCK 128

// ---- host: fractional index of xi in the grid x (not-a-knot cubic spline through (x_i, i)) ------------------
inline void notaknot_index_coords(const double* x, i64 n, const double* xi, i64 m, double* out) {
    std::vector<double> h(n - 1), M(n, 0.0);
    for (i64 i = 0; i + 1 < n; ++i) h[i] = x[i + 1] - x[i];
    // dense (n x n) system of the second derivatives with partial pivoting: n is a grid dimension (<= ~1000),
    // solved once per axis and field component
    std::vector<double> A((size_t)n * n, 0.0), r(n, 0.0);
    auto a = [&](i64 i, i64 j) -> double& { return A[(size_t)i * n + j]; };
    for (i64 i = 1; i + 1 < n; ++i) {
        a(i, i - 1) = h[i - 1]; a(i, i) = 2 * (h[i - 1] + h[i]); a(i, i + 1) = h[i];
        r[i] = 6 * (1.0 / h[i] - 1.0 / h[i - 1]);          // y_i = i: (y_{i+1} - y_i) = 1
    }
    a(0, 0) = h[1]; a(0, 1) = -(h[0] + h[1]); a(0, 2) = h[0];
    a(n - 1, n - 3) = h[n - 2]; a(n - 1, n - 2) = -(h[n - 3] + h[n - 2]); a(n - 1, n - 1) = h[n - 3];
    // banded elimination with row pivoting inside a window of 3 rows (the matrix is tridiagonal plus the
    // two 3-entry end rows)
    for (i64 c = 0; c < n; ++c) {
        i64 p = c;
        const i64 rmax = std::min<i64>(n - 1, c + 2);
        for (i64 q = c + 1; q <= rmax; ++q) if (std::fabs(a(q, c)) > std::fabs(a(p, c))) p = q;
        if (p != c) {
            const i64 jmax = std::min<i64>(n - 1, c + 4);
            for (i64 j = c; j <= jmax; ++j) std::swap(a(c, j), a(p, j));
            std::swap(r[c], r[p]);
        }
        for (i64 q = c + 1; q <= rmax; ++q) {
            const double f = a(q, c) / a(c, c);
            if (f == 0.0) continue;
            const i64 jmax = std::min<i64>(n - 1, c + 4);
            for (i64 j = c; j <= jmax; ++j) a(q, j) -= f * a(c, j);
            r[q] -= f * r[c];
        }
    }
    for (i64 c = n - 1; c >= 0; --c) {
        double s = r[c];
        const i64 jmax = std::min<i64>(n - 1, c + 4);
        for (i64 j = c + 1; j <= jmax; ++j) s -= a(c, j) * M[j];
        M[c] = s / a(c, c);
    }
    for (i64 k = 0; k < m; ++k) {
        const double v = xi[k];
        i64 i = (i64)(std::lower_bound(x, x + n, v) - x) - 1;     // searchsorted(x, v) - 1
        if (i < 0) i = 0;
        if (i > n - 2) i = n - 2;
        const double t0 = v - x[i], t1 = x[i + 1] - v, hi = h[i];
        out[k] = (M[i] * t1 * t1 * t1 + M[i + 1] * t0 * t0 * t0) / (6 * hi) + ((double)i / hi - M[i] * hi / 6) * t1 +
                 ((double)(i + 1) / hi - M[i + 1] * hi / 6) * t0;
        // at the end points the interpolating spline IS its data value (SciPy's B-spline form returns exactly 0 and
        // n - 1 there); the cancelling terms above may leave +-1e-17, which would push a receiver on the first / last
        // point of the trimmed grid outside (cval = NaN)
        if (v == x[0]) out[k] = 0.0;
        if (v == x[n - 1]) out[k] = (double)(n - 1);
    }
}

// ---- device ---------------------------------------------------------------------------------------------------
// dst (n0-2, n1-2, n2-2) <- src[1:-1, 1:-1, 1:-1] of an F-ordered (n0, n1, n2) array (fields.py:799, 812)
template <class T>
__global__ void k_trim_copy(T* dst, const T* src, i64 n0, i64 n1, i64 n2) {
    const i64 m0 = n0 - 2, m1 = n1 - 2, m2 = n2 - 2;
    const i64 tot = m0 * m1 * m2;
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (i64)gridDim.x * blockDim.x) {
        const i64 i0 = idx % m0, i1 = (idx / m0) % m1, i2 = idx / (m0 * m1);
        dst[idx] = src[(i0 + 1) + n0 * ((i1 + 1) + n1 * (i2 + 1))];
    }
}

// In-place cubic B-spline prefilter along `axis` of an F-ordered (n0, n1, n2) array: thread per line.
// scipy.ndimage spline_filter1d, order 3, mirror initialisation (what map_coordinates(mode='constant') uses):
// gain, causal initialisation, causal recursion, anti-causal initialisation, anti-causal recursion.
// reflect != 0: the half-sample-symmetric ("reflect") initialisation that scipy uses for mode='nearest' / 'reflect'.
template <class T>
__global__ void k_spline_filter_axis(T* c, i64 n0, i64 n1, i64 n2, int axis, int reflect) {
    const i64 n = axis == 0 ? n0 : axis == 1 ? n1 : n2;
    const i64 nlines = (n0 * n1 * n2) / n;
    const i64 line = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (line >= nlines || n < 2) return;
    i64 base, st;
    if (axis == 0) { base = line * n0; st = 1; }
    else if (axis == 1) { const i64 i0 = line % n0, i2 = line / n0; base = i0 + n0 * n1 * i2; st = n0; }
    else { base = line; st = n0 * n1; }
    const double z = sqrt(3.0) - 2.0;
    const double gain = (1.0 - z) * (1.0 - 1.0 / z);
    T* p = c + base;
    for (i64 i = 0; i < n; ++i) p[i * st] *= gain;
    if (reflect) {
        const double zn = pow(z, (double)n);
        const T first = p[0];
        T c0 = p[0] + zn * p[(n - 1) * st];
        double zi = z;
        for (i64 i = 1; i < n; ++i) {
            c0 += zi * (p[i * st] + zn * p[(n - 1 - i) * st]);
            zi *= z;
        }
        c0 *= z / (1.0 - zn * zn);
        p[0] = c0 + first;
    } else {
        const double zn1 = pow(z, (double)(n - 1));
        T c0 = p[0] + zn1 * p[(n - 1) * st];
        double zi = z;
        for (i64 i = 1; i < n - 1; ++i) {
            c0 += zi * (p[i * st] + zn1 * p[(n - 1 - i) * st]);
            zi *= z;
        }
        p[0] = c0 / (1.0 - zn1 * zn1);
    }
    T prev = p[0];
    for (i64 i = 1; i < n; ++i) {
        T v = p[i * st];
        v += z * prev;
        p[i * st] = v;
        prev = v;
    }
    const T last = reflect ? p[(n - 1) * st] * (z / (z - 1.0))
                           : (z * p[(n - 2) * st] + p[(n - 1) * st]) * (z / (z * z - 1.0));
    p[(n - 1) * st] = last;
    T nxt = last;
    for (i64 i = n - 2; i >= 0; --i) {
        const T v = z * (nxt - p[i * st]);
        p[i * st] = v;
        nxt = v;
    }
}

__device__ __forceinline__ void bspline3_weights(double t, double w[4]) {
    w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
    const double u = 1.0 - t;
    w[2] = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0;
    w[0] = u * u * u / 6.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
}
__device__ __forceinline__ i64 mirror_index(i64 j, i64 n) {
    if (n == 1) return 0;
    const i64 s2 = 2 * n - 2;
    if (j < 0) {
        j = s2 * (i64)(-j / s2) + j;
        j = (j <= 1 - n) ? j + s2 : -j;
    } else if (j >= n) {
        j -= s2 * (i64)(j / s2);
        if (j >= n) j = s2 - j;
    }
    return j;
}
// Index into the half-sample symmetric extension (d c b a | a b c d | d c b a; scipy's NI_EXTEND_REFLECT), for ANY j:
// scipy maps the coordinate into the array first and only ever reflects indices next to it; here the stencil stays at
// the caller's coordinate, so the rule has to hold far away too (period 2 n).
__device__ __forceinline__ i64 reflect_index(i64 j, i64 n) {
    const i64 s2 = 2 * n;
    i64 m = j % s2;
    if (m < 0) m += s2;
    return m < n ? m : s2 - 1 - m;
}
template <class T> __device__ __forceinline__ T fill_of(double v);
template <> __device__ __forceinline__ double fill_of<double>(double v) { return v; }
template <> __device__ __forceinline__ c128 fill_of<c128>(double v) { return mk(v, v); }

// Cubic B-spline interpolant of `coef` at the fractional indices co(0), co(1), co(2) (k_spline_eval, k_spline_eval_grid).
// edge = 0 (mode='constant'): points outside [0, n-1] get cval, stencil indices beyond the array are mirrored;
// edge = 1 (mode='nearest', on the pre-padded array) / 2 (mode='mirror', and 'wrap' on coordinates wrapped by the caller) /
// 3 (mode='reflect'): no point is outside -- the stencil sits at the coordinate and indices beyond the array take the edge
// coefficient / are mirrored / are reflected (scipy's NI_EXTEND_NEAREST / _MIRROR / _REFLECT).
template <class T, class Co>
__device__ __forceinline__ T spline_point(const T* coef, i64 n0, i64 n1, i64 n2, Co co, double cval, int edge) {
    const i64 nn[3] = {n0, n1, n2};
    i64 idx[3][4];
    double w[3][4];
    bool outside = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double cc = co(a);
        if (edge) {
            if (!(cc == cc) || fabs(cc) > 1e15) outside = true;             // NaN (or beyond integer range)
            if (edge == 1) cc = cc < -4.0 ? -4.0 : (cc > (double)(nn[a] + 3) ? (double)(nn[a] + 3) : cc);   // far away: all four indices clamp alike
        } else if (!(cc >= 0.0 && cc <= (double)(nn[a] - 1))) outside = true;                // NaN coordinates count as outside
        const double fl = floor(cc);
        bspline3_weights(cc - fl, w[a]);
        const i64 start = (i64)fl - 1;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const i64 j = start + l;
            idx[a][l] = outside ? 0 : edge == 1 ? (j < 0 ? 0 : (j > nn[a] - 1 ? nn[a] - 1 : j))
                                    : edge == 3 ? reflect_index(j, nn[a]) : mirror_index(j, nn[a]);
        }
    }
    T val;
    if (outside) {
        val = fill_of<T>(cval);
    } else {
        // the 64 coefficients are loaded together, then summed in the fixed order (written as one loop the float64
        // instantiation issued one load per term and waited for it: 56 dependent round trips)
        T c[64];
#pragma unroll
        for (int a0 = 0; a0 < 4; ++a0)
#pragma unroll
            for (int a1 = 0; a1 < 4; ++a1)
#pragma unroll
                for (int a2 = 0; a2 < 4; ++a2)
                    c[(a0 * 4 + a1) * 4 + a2] = coef[idx[0][a0] + n0 * (idx[1][a1] + n1 * idx[2][a2])];
        __builtin_amdgcn_sched_barrier(0);
        val = Zero<T>::v();
#pragma unroll
        for (int a0 = 0; a0 < 4; ++a0)
#pragma unroll
            for (int a1 = 0; a1 < 4; ++a1)
#pragma unroll
                for (int a2 = 0; a2 < 4; ++a2)
                    val += c[(a0 * 4 + a1) * 4 + a2] * (w[0][a0] * w[1][a1] * w[2][a2]);
    }
    return val;
}

// out[r] += fac[r] * (cubic B-spline interpolant of `coef` at the fractional indices coords[a][r]); thread per point.
// fac == nullptr: out[r] = value.  edge: spline_point.
template <class T>
__global__ __launch_bounds__(EMG_RCV_BLOCK) void k_spline_eval(T* out, const T* coef, i64 n0, i64 n1, i64 n2, const double* coords, const double* fac,
                              i64 npts, double cval, int edge) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= npts) return;
    const T val = spline_point<T>(coef, n0, n1, n2, [&](int a) { return coords[a * npts + r]; }, cval, edge);
    if (fac) out[r] += fac[r] * val;
    else out[r] = val;
}

// The 2 x 2 x 2 weighted sum of trilinear interpolation in interval (i0, i1, i2) at normalised distances (t0, t1, t2)
// (k_linear_eval, k_linear_eval_grid).
template <class T>
__device__ __forceinline__ T linear_point(const T* values, i64 s0, i64 s1, i64 s2, i64 i0, i64 i1, i64 i2, double t0, double t1,
                                          double t2) {
    T val = Zero<T>::v();
    for (int a0 = 0; a0 < 2; ++a0)
        for (int a1 = 0; a1 < 2; ++a1)
            for (int a2 = 0; a2 < 2; ++a2) {
                const double w = (a0 ? t0 : 1 - t0) * (a1 ? t1 : 1 - t1) * (a2 ? t2 : 1 - t2);
                val += values[(i0 + a0) * s0 + (i1 + a1) * s1 + (i2 + a2) * s2] * w;
            }
    return val;
}

// Trilinear interpolation, thread per point: ii / tt = interval index and normalised distance per axis (host:
// searchsorted - 1 clipped, as RegularGridInterpolator), inside[r] = 0: the point gets `fill`.
// The array is addressed with explicit offset / strides, so the trimmed view [1:-1]^3 needs no copy.
template <class T>
__global__ void k_linear_eval(T* out, const T* values, i64 s0, i64 s1, i64 s2, const int* ii, const double* tt,
                              const int* inside, const double* fac, i64 npts, double fill) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= npts) return;
    T val;
    if (!inside[r]) {
        val = Zero<T>::v();
        add_real(val, fill);            // fill_value is a real scalar (complex values: fill + 0j)
    } else {
        val = linear_point<T>(values, s0, s1, s2, ii[r], ii[npts + r], ii[2 * npts + r], tt[r], tt[npts + r], tt[2 * npts + r]);
    }
    if (fac) out[r] += fac[r] * val;
    else out[r] = val;
}

// ---- host driver ----------------------------------------------------------------------------------------------
// One field component on the device: F-ordered (n[0], n[1], n[2]) array and the grid vector of every axis.
template <class T>
struct RcvComp {
    const T* dev = nullptr;
    i64 n[3] = {0, 0, 0};
    std::vector<double> pts[3];
};

// interp3d(points, values, xi, method, fill_value, 'constant', cval) of a device-resident array (maps.py:179-276):
// out_dev[r] (+)= fac[r] * value.  `off`/(s0,s1,s2): the view of `values` that `pts` describe (the receivers pass the
// [1:-1]^3 view: off = 1 + n0 + n0 n1).  scratch: >= prod(n) entries for the spline coefficients (cubic only).
template <class T>
int interp3d_device(hipStream_t st, const T* values, const i64 n[3], i64 off, i64 s0, i64 s1, i64 s2,
                    const std::vector<double> pts[3], i64 npts, const double* xi /* [3][npts] */, int method,
                    bool has_fill, double fill, double cval, const double* fac_host, T* scratch, T* out_dev) {
    for (int a = 0; a < 3; ++a) if ((i64)pts[a].size() != n[a] || n[a] < 1) return -2;
    // method: 0 linear, 1 cubic, 2 / 3 / 4 cubic with `xi` already in INDEX coordinates of `values` (the caller has applied the
    // not-a-knot index spline and a boundary mode of scipy.ndimage.map_coordinates: emg3d_amd/maps.py); 3: the arithmetic of
    // mode='nearest' on the pre-padded array ("reflect" prefilter initialisation, indices clamped, nothing is outside)
    for (int a = 0; a < 3; ++a) if (n[a] < 4 && method < 2) method = 0;             // maps.py:238-240
    if (method >= 2) for (int a = 0; a < 3; ++a) if (n[a] < 4) return -2;
    const unsigned blocks = (unsigned)((npts + EMG_RCV_BLOCK - 1) / EMG_RCV_BLOCK);
    double* dfac = nullptr;
    DevBlock tmpb;
    const size_t nb = (size_t)npts * (3 * sizeof(double) + sizeof(double) + 3 * sizeof(int) + sizeof(int)) + 256;
    HIP_TRY(tmpb.alloc(nb));
    char* tmp = tmpb.get<char>();
    double* dco = (double*)tmp;                         // coords / tt
    dfac = dco + 3 * npts;
    int* dii = (int*)(dfac + npts);
    int* dins = dii + 3 * npts;
    if (fac_host) HIP_TRY(hipMemcpyAsync(dfac, fac_host, (size_t)npts * sizeof(double), hipMemcpyHostToDevice, st));
    int rc = 0;
    if (method >= 1) {
        std::vector<double> co((size_t)3 * npts);
        for (int a = 0; a < 3; ++a) {
            if (method >= 2) std::copy(xi + a * npts, xi + (a + 1) * npts, co.data() + a * npts);
            else notaknot_index_coords(pts[a].data(), n[a], xi + a * npts, npts, co.data() + a * npts);
        }
        HIP_TRY(hipMemcpyAsync(dco, co.data(), co.size() * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));                 // `co` is a temporary
        // spline coefficients of the view: copy it out contiguously, filter the three axes in place
        const i64 tot = n[0] * n[1] * n[2];
        {
            // generic strided copy through k_trim_copy when the view is the [1:-1]^3 interior, else plain copy
            if (off == 0) HIP_TRY(hipMemcpyAsync(scratch, values, (size_t)tot * sizeof(T), hipMemcpyDeviceToDevice, st));
            else hipLaunchKernelGGL(k_trim_copy<T>, dim3((unsigned)std::min<i64>((tot + 255) / 256, 8192)), dim3(256), 0, st,
                                    scratch, values, n[0] + 2, n[1] + 2, n[2] + 2);
        }
        for (int a = 0; a < 3; ++a) {
            const i64 nl = tot / n[a];
            hipLaunchKernelGGL(k_spline_filter_axis<T>, dim3((unsigned)((nl + 63) / 64)), dim3(64), 0, st, scratch, n[0], n[1], n[2], a,
                               (method == 3 || method == 4) ? 1 : 0);
        }
        hipLaunchKernelGGL(k_spline_eval<T>, dim3(blocks), dim3(EMG_RCV_BLOCK), 0, st, out_dev, (const T*)scratch, n[0], n[1], n[2],
                           (const double*)dco, fac_host ? (const double*)dfac : nullptr, npts, cval, method == 3 ? 1 : method == 2 ? 2 : method == 4 ? 3 : 0);
    } else {
        std::vector<int> ii((size_t)3 * npts), ins((size_t)npts, 1);
        std::vector<double> tt((size_t)3 * npts);
        for (int a = 0; a < 3; ++a) {
            const double* g = pts[a].data();
            for (i64 r = 0; r < npts; ++r) {
                const double v = xi[a * npts + r];
                if (!(v >= g[0] && v <= g[n[a] - 1])) ins[r] = has_fill ? 0 : ins[r];
                i64 i = (i64)(std::lower_bound(g, g + n[a], v) - g) - 1;
                if (i < 0) i = 0;
                if (i > n[a] - 2) i = n[a] - 2;
                if (n[a] == 1) {
                    // an axis with ONE point (a 3-cell grid dimension, trimmed): RegularGridInterpolator's interval has no
                    // length, its normalised distance is 0 and both corners are that point (the stride is zeroed below)
                    ii[a * npts + r] = 0;
                    tt[a * npts + r] = 0.0;
                    continue;
                }
                ii[a * npts + r] = (int)i;
                tt[a * npts + r] = (v - g[i]) / (g[i + 1] - g[i]);
            }
        }
        HIP_TRY(hipMemcpyAsync(dco, tt.data(), tt.size() * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dii, ii.data(), ii.size() * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dins, ins.data(), ins.size() * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (n[0] == 1) s0 = 0;
        if (n[1] == 1) s1 = 0;
        if (n[2] == 1) s2 = 0;
        hipLaunchKernelGGL(k_linear_eval<T>, dim3(blocks), dim3(EMG_RCV_BLOCK), 0, st, out_dev, values + off, s0, s1, s2,
                           (const int*)dii, (const double*)dco, (const int*)dins, fac_host ? (const double*)dfac : nullptr, npts, fill);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { fprintf(stderr, "[emg3d_hip] interp3d: %s\n", hipGetErrorString(e)); rc = (int)e; }
    return rc;
}

// fields.get_receiver_response (fields.py:733-817) of three device-resident components: resp_host[n] =
// sum_c fac[c][r] * interp3d(points_c[1:-1], comp_c[1:-1,1:-1,1:-1], xyz, 'cubic', 0.0, 'constant', nan); a component
// whose factors are all <= 1e-10 in magnitude is skipped (fields.py:810).  method 0: trilinear interpolation on the same trimmed
// points, NaN outside (the receiver operator whose transpose receiver_adjoint_device applies); scratch is not used then.
template <class T>
int receiver_response_device(hipStream_t st, const RcvComp<T> comp[3], i64 npts, const double* xyz, const double* fac,
                             T* scratch, T* resp_host, int method = 1) {
    if (npts < 1) return -2;
    T* dresp = nullptr;
    DEV_ALLOC(dresp, (size_t)npts * sizeof(T));
    HIP_TRY(hipMemsetAsync(dresp, 0, (size_t)npts * sizeof(T), st));
    int rc = 0;
    for (int c = 0; c < 3 && rc == 0; ++c) {
        bool active = false;
        for (i64 r = 0; r < npts; ++r) if (std::fabs(fac[c * npts + r]) > 1e-10) { active = true; break; }
        if (!active) continue;
        const RcvComp<T>& C = comp[c];
        i64 m[3];
        std::vector<double> p[3];
        for (int a = 0; a < 3; ++a) {
            m[a] = C.n[a] - 2;
            if (m[a] < 1) { rc = -2; break; }
            p[a].assign(C.pts[a].begin() + 1, C.pts[a].end() - 1);
        }
        if (rc) break;
        const i64 off = 1 + C.n[0] + C.n[0] * C.n[1];
        rc = interp3d_device<T>(st, C.dev, m, off, 1, C.n[0], C.n[0] * C.n[1], p, npts, xyz, method, true, method ? 0.0 : NAN, NAN,
                                fac + c * npts, scratch, dresp);
    }
    if (rc == 0) {
        hipError_t e = hipMemcpyAsync(resp_host, dresp, (size_t)npts * sizeof(T), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = (int)e;
    }
        return rc;
}

// ---- transpose of the receiver operators ------------------------------------------------------------------------------------
// s[edge] (+)= sum over the receivers r that touch the edge of weight * w[r]: thread per TOUCHED edge, contributions in the fixed
// order of the host's table (receiver, then corner) -- deterministic although receivers share edges, no atomics.
template <class T>
__global__ void k_receiver_adjoint(T* s, const i64* edges, const int* ptr, const int* rcv, const double* wgt, const T* w, i64 nedges) {
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nedges) return;
    T acc = Zero<T>::v();
    for (int q = ptr[k]; q < ptr[k + 1]; ++q) acc += w[rcv[q]] * wgt[q];
    s[edges[k]] += acc;
}

// Transpose of k_spline_eval: coef[idx] = sum of w[r] * (fac[r] w0 w1 w2) over the (receiver, stencil point) pairs that read the
// coefficient idx -- thread per TOUCHED coefficient of the zeroed trimmed array, summed in the order of the host's table
// (receiver, then stencil order; stencil indices that the mirror extension folds onto one coefficient add up).
template <class T>
__global__ void k_spline_eval_adjoint(T* coef, const i64* idx, const int* ptr, const int* rcv, const double* wgt, const T* w, i64 ntouched) {
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ntouched) return;
    T acc = Zero<T>::v();
    for (int q = ptr[k]; q < ptr[k + 1]; ++q) acc += w[rcv[q]] * wgt[q];
    coef[idx[k]] = acc;
}

// First and last entry of every line along `axis` of an F-ordered (n0, n1, n2) array times f; thread per line.  The prefilter
// F of k_spline_filter_axis (mirror initialisation) is the inverse of tridiag(1/6, 4/6, 1/6) with the end rows (4/6, 2/6): not
// symmetric, but F^T = D F D^-1 with D = diag(1/2, 1, ..., 1, 1/2) -- the transposed filter is this kernel with f = 2, the
// forward filter, this kernel with f = 1/2 (both scalings are exact).  Lines with n < 2 are left alone, as the filter leaves them.
template <class T>
__global__ void k_line_ends_scale(T* c, i64 n0, i64 n1, i64 n2, int axis, double f) {
    const i64 n = axis == 0 ? n0 : axis == 1 ? n1 : n2;
    const i64 nlines = (n0 * n1 * n2) / n;
    const i64 line = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (line >= nlines || n < 2) return;
    i64 base, st;
    if (axis == 0) { base = line * n0; st = 1; }
    else if (axis == 1) { const i64 i0 = line % n0, i2 = line / n0; base = i0 + n0 * n1 * i2; st = n0; }
    else { base = line; st = n0 * n1; }
    c[base] *= f;
    c[base + (n - 1) * st] *= f;
}

// Transpose of k_trim_copy through a field layout: s[off + (i0+1) st0 + (i1+1) st1 + (i2+1) st2] += coef[i0, i1, i2] for the
// F-ordered (m0, m1, m2) array coef; thread per trimmed element, i0 fastest.
template <class T>
__global__ void k_trim_add(T* s, const T* coef, i64 m0, i64 m1, i64 m2, i64 off, i64 st0, i64 st1, i64 st2) {
    const i64 tot = m0 * m1 * m2;
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (i64)gridDim.x * blockDim.x) {
        i64 i0, i1, i2;
        unlin3(idx, m0, m1, m2, i0, i1, i2);
        s[off + (i0 + 1) * st0 + (i1 + 1) * st1 + (i2 + 1) * st2] += coef[idx];
    }
}

// host twins of bspline3_weights / mirror_index (the tables of k_spline_eval_adjoint are built on the host)
inline void bspline3_weights_host(double t, double w[4]) {
    w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
    const double u = 1.0 - t;
    w[2] = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0;
    w[0] = u * u * u / 6.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
}
inline i64 mirror_index_host(i64 j, i64 n) {
    if (n == 1) return 0;
    const i64 s2 = 2 * n - 2;
    if (j < 0) {
        j = s2 * (i64)(-j / s2) + j;
        j = (j <= 1 - n) ? j + s2 : -j;
    } else if (j >= n) {
        j -= s2 * (i64)(j / s2);
        if (j >= n) j = s2 - j;
    }
    return j;
}

// One contribution of a receiver to an entry of the target array.
struct AdjEntry { i64 idx; int r; double w; };

// The 8 trilinear weights per receiver of component c (as interp3d_device, method 0, on the trimmed points) for every receiver
// with skip[r] == 0, appended to `ent` with target indices through the layout tl.
template <class T>
void linear_adjoint_entries(const RcvComp<T>& C, const FieldLayout& tl, int c, i64 npts, const double* xyz, const double* fac,
                            const std::vector<char>& skip, std::vector<AdjEntry>& ent) {
    for (i64 r = 0; r < npts; ++r) {
        if (skip[r]) continue;
        i64 ii[3];
        double tt[3];
        for (int a = 0; a < 3; ++a) {           // as interp3d_device, method 0
            const double* g = C.pts[a].data() + 1;
            const i64 m = C.n[a] - 2;
            const double v = xyz[a * npts + r];
            i64 i = (i64)(std::lower_bound(g, g + m, v) - g) - 1;
            if (i < 0) i = 0;
            if (i > m - 2) i = m - 2;
            if (m == 1) { ii[a] = 1; tt[a] = 0.0; continue; }
            ii[a] = i + 1;
            tt[a] = (v - g[i]) / (g[i + 1] - g[i]);
        }
        for (int a0 = 0; a0 < 2; ++a0)
            for (int a1 = 0; a1 < 2; ++a1)
                for (int a2 = 0; a2 < 2; ++a2) {
                    const double wg = (a0 ? tt[0] : 1 - tt[0]) * (a1 ? tt[1] : 1 - tt[1]) * (a2 ? tt[2] : 1 - tt[2]);
                    // (an axis with one trimmed point: both corners are that point, weights 1 and 0)
                    const i64 i0 = ii[0] + (C.n[0] == 3 ? 0 : a0), i1 = ii[1] + (C.n[1] == 3 ? 0 : a1),
                              i2 = ii[2] + (C.n[2] == 3 ? 0 : a2);
                    ent.push_back({tl.off[c] + i0 * tl.st[c][0] + i1 * tl.st[c][1] + i2 * tl.st[c][2], (int)r,
                                   fac[c * npts + r] * wg});
                }
    }
}

// CSR by target index of `ent` (stable: the entries of one index keep their order) on the device; the host arrays stay alive with
// the table (the uploads are asynchronous).
struct AdjCsr {
    DevBlock blk;
    std::vector<i64> edges;
    std::vector<int> ptr, rcv;
    std::vector<double> wgt;
    i64* dedges = nullptr;
    double* dwgt = nullptr;
    int* dptr = nullptr;
    int* drcv = nullptr;
    i64 ne = 0;
};

inline int csr_adjoint_build(hipStream_t st, std::vector<AdjEntry>& ent, AdjCsr& t) {
    t.ne = 0;
    if (ent.empty()) return 0;
    std::stable_sort(ent.begin(), ent.end(), [](const AdjEntry& a, const AdjEntry& b) { return a.idx < b.idx; });
    t.rcv.resize(ent.size());
    t.wgt.resize(ent.size());
    for (size_t q = 0; q < ent.size(); ++q) {
        if (q == 0 || ent[q].idx != ent[q - 1].idx) { t.edges.push_back(ent[q].idx); t.ptr.push_back((int)q); }
        t.rcv[q] = ent[q].r; t.wgt[q] = ent[q].w;
    }
    t.ptr.push_back((int)ent.size());
    const size_t ne = t.edges.size(), nq = ent.size();
    HIP_TRY(t.blk.alloc(ne * 8 + nq * 8 + (ne + 1 + nq) * 4 + 64));
    t.dedges = t.blk.get<i64>();
    t.dwgt = (double*)(t.dedges + ne);
    t.dptr = (int*)(t.dwgt + nq);
    t.drcv = t.dptr + ne + 1;
    HIP_TRY(hipMemcpyAsync(t.dedges, t.edges.data(), ne * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(t.dwgt, t.wgt.data(), nq * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(t.dptr, t.ptr.data(), (ne + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(t.drcv, t.rcv.data(), nq * 4, hipMemcpyHostToDevice, st));
    t.ne = (i64)ne;
    return 0;
}

// One thread per touched index of the table: ASSIGN ? k_spline_eval_adjoint (dst[idx] = sum) : k_receiver_adjoint (dst[idx] += sum),
// with the device-resident data vector w.  Does not synchronise.
template <class T, bool ASSIGN>
void csr_adjoint_apply(hipStream_t st, const AdjCsr& t, const T* dw, T* dst) {
    if (!t.ne) return;
    const dim3 grid((unsigned)((t.ne + EMG_RCV_BLOCK - 1) / EMG_RCV_BLOCK));
    if (ASSIGN)
        hipLaunchKernelGGL(k_spline_eval_adjoint<T>, grid, dim3(EMG_RCV_BLOCK), 0, st, dst, (const i64*)t.dedges, (const int*)t.dptr,
                           (const int*)t.drcv, (const double*)t.dwgt, dw, t.ne);
    else
        hipLaunchKernelGGL(k_receiver_adjoint<T>, grid, dim3(EMG_RCV_BLOCK), 0, st, dst, (const i64*)t.dedges, (const int*)t.dptr,
                           (const int*)t.drcv, (const double*)t.dwgt, dw, t.ne);
}

// The transpose P^T of a receiver operator as device tables -- everything that depends on the grid and the receivers only, built
// ONCE (build) and then applied to any number of data vectors (apply: kernels only, no host work).
//   method 0: P the operator of receiver_response_device(method 0) on the components comp (only n / pts are used; electric edges or
//   magnetic faces), fl the layout of the target.  Host: 8 weights per receiver and active component, O(npts log npts); CSR by edge.
//   A receiver outside the trimmed points of an active component (its datum is NaN) contributes nothing.
//   method 1: P the operator of receiver_response_device(method 1): per active component
//       P = R Eval(xi) F_2 F_1 F_0 Trim,       P^T w = Trim^T F_0^T F_1^T F_2^T Eval^T R^T w
//   with the 64 weights fac w0 w1 w2 per receiver gathered into the zeroed coefficient array `coef` (k_spline_eval_adjoint), the
//   transposed prefilter per axis (k_line_ends_scale, k_spline_filter_axis, k_line_ends_scale) and k_trim_add into the target.  The
//   rules of the forward operator: a component with fewer than four trimmed points along an axis is linear with fill value 0 (a
//   receiver outside ITS points adds nothing for that component); a receiver whose index coordinates leave [0, n - 1] on an axis of
//   a cubic component has a NaN datum and contributes nothing at all.
template <class T>
struct RcvAdjPlan {
    AdjCsr lin;              // the linear components, straight into the target
    AdjCsr cub[3];           // per cubic component: coefficient -> contributions
    i64 m[3][3];
    FieldLayout fl;

    int build(hipStream_t st, int method, const RcvComp<T> comp[3], const FieldLayout& tl, i64 npts, const double* xyz, const double* fac) {
        if (npts < 1) return -2;
        fl = tl;
        bool active[3], cubic[3];
        std::vector<double> co[3];
        std::vector<char> dead((size_t)npts, 0);
        for (int c = 0; c < 3; ++c) {
            active[c] = false; cubic[c] = false;
            for (i64 r = 0; r < npts; ++r) if (std::fabs(fac[c * npts + r]) > 1e-10) { active[c] = true; break; }
            if (!active[c]) continue;
            cubic[c] = method != 0;
            for (int a = 0; a < 3; ++a) {
                if (comp[c].n[a] < 3) return -2;
                m[c][a] = comp[c].n[a] - 2;
                if (m[c][a] < 4) cubic[c] = false;              // maps.py:238-240
            }
            if (!method) {          // linear receivers: outside ANY active component's points -> NaN datum
                for (int a = 0; a < 3; ++a) {
                    const double* g = comp[c].pts[a].data() + 1;
                    for (i64 r = 0; r < npts; ++r) if (!(xyz[a * npts + r] >= g[0] && xyz[a * npts + r] <= g[m[c][a] - 1])) dead[r] = 1;
                }
                continue;
            }
            if (!cubic[c]) continue;
            co[c].resize((size_t)3 * npts);
            for (int a = 0; a < 3; ++a) {
                notaknot_index_coords(comp[c].pts[a].data() + 1, m[c][a], xyz + a * npts, npts, co[c].data() + a * npts);
                for (i64 r = 0; r < npts; ++r) {
                    const double cc = co[c][a * npts + r];
                    if (!(cc >= 0.0 && cc <= (double)(m[c][a] - 1))) dead[r] = 1;
                }
            }
        }
        std::vector<AdjEntry> ent;
        for (int c = 0; c < 3; ++c) {
            if (!active[c] || cubic[c]) continue;
            std::vector<char> skip(dead);
            if (method)             // the linear fallback of a cubic operator: fill value 0 outside ITS points
                for (int a = 0; a < 3; ++a) {
                    const double* g = comp[c].pts[a].data() + 1;
                    for (i64 r = 0; r < npts; ++r) if (!(xyz[a * npts + r] >= g[0] && xyz[a * npts + r] <= g[m[c][a] - 1])) skip[r] = 1;
                }
            linear_adjoint_entries<T>(comp[c], fl, c, npts, xyz, fac, skip, ent);
        }
        int rc = csr_adjoint_build(st, ent, lin);
        for (int c = 0; c < 3 && rc == 0; ++c) {
            if (!active[c] || !cubic[c]) continue;
            const i64 m0 = m[c][0], m1 = m[c][1];
            ent.clear();
            for (i64 r = 0; r < npts; ++r) {
                if (dead[r]) continue;
                i64 idx[3][4];
                double wt[3][4];
                for (int a = 0; a < 3; ++a) {           // as spline_point, edge 0
                    const double cc = co[c][a * npts + r];
                    const double flr = std::floor(cc);
                    bspline3_weights_host(cc - flr, wt[a]);
                    const i64 start = (i64)flr - 1;
                    for (int l = 0; l < 4; ++l) idx[a][l] = mirror_index_host(start + l, m[c][a]);
                }
                for (int a0 = 0; a0 < 4; ++a0)
                    for (int a1 = 0; a1 < 4; ++a1)
                        for (int a2 = 0; a2 < 4; ++a2)
                            ent.push_back({idx[0][a0] + m0 * (idx[1][a1] + m1 * idx[2][a2]), (int)r,
                                           fac[c * npts + r] * (wt[0][a0] * wt[1][a1] * wt[2][a2])});
            }
            rc = csr_adjoint_build(st, ent, cub[c]);
        }
        return rc;
    }

    // s += P^T w for the device-resident data vector dw (npts values); coef: scratch, >= the largest trimmed component (cubic only)
    void apply(hipStream_t st, const T* dw, T* coef, T* s) const {
        csr_adjoint_apply<T, false>(st, lin, dw, s);
        for (int c = 0; c < 3; ++c) {
            if (!cub[c].ne) continue;
            const i64 m0 = m[c][0], m1 = m[c][1], m2 = m[c][2], tot = m0 * m1 * m2;
            hipMemsetAsync(coef, 0, (size_t)tot * sizeof(T), st);
            csr_adjoint_apply<T, true>(st, cub[c], dw, coef);
            for (int a = 2; a >= 0; --a) {
                const i64 nl = tot / m[c][a];
                const dim3 grid((unsigned)((nl + 63) / 64));
                hipLaunchKernelGGL(k_line_ends_scale<T>, grid, dim3(64), 0, st, coef, m0, m1, m2, a, 2.0);
                hipLaunchKernelGGL(k_spline_filter_axis<T>, grid, dim3(64), 0, st, coef, m0, m1, m2, a, 0);
                hipLaunchKernelGGL(k_line_ends_scale<T>, grid, dim3(64), 0, st, coef, m0, m1, m2, a, 0.5);
            }
            hipLaunchKernelGGL(k_trim_add<T>, dim3((unsigned)std::min<i64>((tot + 255) / 256, 8192)), dim3(256), 0, st, s, (const T*)coef,
                               m0, m1, m2, fl.off[c], fl.st[c][0], fl.st[c][1], fl.st[c][2]);
        }
    }
};

inline int rcv_adjoint_sync(hipStream_t st, const char* what) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);             // (the host tables and the device blocks go out of scope)
    if (e != hipSuccess) { fprintf(stderr, "[emg3d_hip] %s: %s\n", what, hipGetErrorString(e)); return (int)e; }
    return 0;
}

// s (+)= P^T w for ONE host data vector: the plan, built and applied once (method 0 / 1 as RcvAdjPlan).  Synchronises the stream.
template <class T>
int receiver_adjoint_any_device(hipStream_t st, int method, const RcvComp<T> comp[3], const FieldLayout& fl, i64 npts, const double* xyz,
                                const double* fac, const T* w_host, T* coef, T* s) {
    if (npts < 1) return -2;
    T* dw = nullptr;
    DEV_ALLOC(dw, (size_t)npts * sizeof(T));            // (before the plan: no early return while its uploads are in flight)
    RcvAdjPlan<T> plan;
    int rc = plan.build(st, method, comp, fl, npts, xyz, fac);
    if (rc == 0 && hipMemcpyAsync(dw, w_host, (size_t)npts * sizeof(T), hipMemcpyHostToDevice, st) != hipSuccess)
        rc = (int)hipGetLastError();
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    plan.apply(st, dw, coef, s);
    return rcv_adjoint_sync(st, method ? "cubic receiver adjoint" : "receiver adjoint");
}

template <class T>
int receiver_adjoint_device(hipStream_t st, const RcvComp<T> comp[3], const FieldLayout& fl, i64 npts, const double* xyz,
                            const double* fac, const T* w_host, T* s) {
    return receiver_adjoint_any_device<T>(st, 0, comp, fl, npts, xyz, fac, w_host, (T*)nullptr, s);
}

template <class T>
int receiver_adjoint_cubic_device(hipStream_t st, const RcvComp<T> comp[3], const FieldLayout& fl, i64 npts, const double* xyz,
                                  const double* fac, const T* w_host, T* coef, T* s) {
    return receiver_adjoint_any_device<T>(st, 1, comp, fl, npts, xyz, fac, w_host, coef, s);
}
