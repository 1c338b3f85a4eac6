// Regridding on the device: maps.volume_average / maps.grid2grid (reference emg3d/maps.py:34-178, 453-576).
//
// Volume averaging (grid2grid(method='volume'), Model.interpolate2grid).  Per axis, the union of the old and the new edges
// cuts the new grid into segments; segment s has length w[s], lies in old cell in[s] and new cell out[s] (O(n) host work,
// volume_average_weights_host).  New cell (ox, oy, oz) is the sum over the tensor product of its segments of
// (w_z w_y) w_x v[in_x, in_y, in_z], divided by its volume.  The segments come out sorted by new cell, so every new cell owns
// a contiguous range of them per axis (CSR offsets `ptr`): k_volume_average is a gather, one thread per new cell, x fastest
// (the writes coalesce; no atomics, the result does not depend on the schedule).  Each thread sums in the reference's order
// (z segments outermost, then y, then x, onto the value already there) and divides as NumPy does, so the result is the
// reference's bit for bit.  Bytes: the old array once (neighbouring threads read neighbouring old cells) plus the new array
// read and written.
//
// Tensor-product interpolation (grid2grid(method='linear' / 'cubic')): the targets of grid2grid are the tensor product of
// three coordinate vectors; the per-axis work (interval index and distance, not-a-knot index coordinates) is O(mx + my + mz)
// on the host and k_linear_eval_grid / k_spline_eval_grid evaluate the per-point kernels' arithmetic (linear_point,
// spline_point) at point (i, j, k) from the per-axis vectors -- bit for bit interp3d on the materialised points.
#pragma once
#include <algorithm>
#include <vector>
#include "common.hpp"
#include "receivers.hpp"

#define EMG_RGD_BLOCK 256
#define EMG_RGD_XSEG 8         // x segments per new cell kept in registers (more: the plain loop)

// ---- host: segments of one axis --------------------------------------------------------------------------------
// x1 (n1 edges, old grid), x2 (n2 edges, new grid), both ascending, n1, n2 >= 2.  Writes at most n1 + n2 - 1 segments
// (w, in, out) and ptr[0 .. n2-1] (new cell o owns segments [ptr[o], ptr[o+1])); returns the number of segments.
inline i64 volume_average_weights_host(const double* x1, i64 n1, const double* x2, i64 n2, double* w, i64* in, i64* out,
                                       i64* ptr) {
    std::vector<double> u(x1, x1 + n1);
    u.insert(u.end(), x2, x2 + n2);
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    // index of the cell of `e` (ascending, n edges) that holds c: the last edge <= c, clipped to the first / last cell
    auto cell = [](const double* e, i64 n, double c) {
        const i64 k = (i64)(std::upper_bound(e, e + n, c) - e) - 1;
        return k < 0 ? (i64)0 : (k > n - 2 ? n - 2 : k);
    };
    for (i64 o = 0; o < n2; ++o) ptr[o] = 0;
    i64 ns = 0;
    for (size_t i = 0; i + 1 < u.size(); ++i) {
        const double a = u[i], b = u[i + 1];
        const double c = 0.5 * (a + b);
        if (!(x2[0] <= c && c <= x2[n2 - 1])) continue;
        w[ns] = b - a;
        in[ns] = cell(x1, n1, c);
        out[ns] = cell(x2, n2, c);
        ++ptr[out[ns] + 1];
        ++ns;
    }
    for (i64 o = 1; o < n2; ++o) ptr[o] += ptr[o - 1];
    return ns;
}

// ---- device ----------------------------------------------------------------------------------------------------
struct VolAvgAxes {
    const i64* ptr[3];          // per axis: segment offsets of the new cells (m + 1)
    const i64* in[3];           // per axis: old cell of each segment
    const double* w[3];         // per axis: segment length
};

// new_values[o] = (new_values[o] + sum_segments (w_z w_y) w_x v[in]) / vol[o]; one thread per new cell, x fastest.
template <class T> __device__ __forceinline__ T div_vol(T a, double v);
template <> __device__ __forceinline__ double div_vol<double>(double a, double v) { return a / v; }
// NumPy divides complex128 by float64 as complex by (v + 0j): Smith's formula with ratio 0, i.e. a * (1 / v)
template <> __device__ __forceinline__ c128 div_vol<c128>(c128 a, double v) {
#pragma clang fp contract(off)
    const double s = 1.0 / v;
    return mk(a.re * s, a.im * s);
}

// acc += wt * v, unfused (the pragma must cover the complex parts too: operator* / += of common.hpp carry the default)
__device__ __forceinline__ void add_weighted(double& acc, double wt, double v) {
#pragma clang fp contract(off)
    acc += wt * v;
}
__device__ __forceinline__ void add_weighted(c128& acc, double wt, c128 v) {
#pragma clang fp contract(off)
    acc.re += wt * v.re;
    acc.im += wt * v.im;
}

template <class T>
__global__ __launch_bounds__(EMG_RGD_BLOCK) void k_volume_average(T* out, const T* v, const double* vol, i64 nx, i64 ny,
                                                                  i64 mx, i64 my, i64 ntot, VolAvgAxes ax) {
#pragma clang fp contract(off)      // NumPy's loops do not fuse; keeps the result bit-identical to the reference's
    const i64 o = (i64)blockIdx.x * EMG_RGD_BLOCK + threadIdx.x;
    if (o >= ntot) return;
    const i64 ox = o % mx, oyz = o / mx;
    const i64 oy = oyz % my, oz = oyz / my;
    const i64 x0 = ax.ptr[0][ox], x1 = ax.ptr[0][ox + 1];
    const i64 y0 = ax.ptr[1][oy], y1 = ax.ptr[1][oy + 1];
    const i64 z0 = ax.ptr[2][oz], z1 = ax.ptr[2][oz + 1];
    const i64 nxy = nx * ny;
    T acc = out[o];
    if (x1 - x0 <= EMG_RGD_XSEG) {
        // the thread's x segments in registers, the loads of a row issued together (one dependent round trip per row
        // instead of one per segment: 512^3 -> 256^3 float64 1.23 -> 0.79 ms), then summed in the same order
        const int cx = (int)(x1 - x0);
        double wx[EMG_RGD_XSEG];
        i64 ix[EMG_RGD_XSEG];
#pragma unroll
        for (int k = 0; k < EMG_RGD_XSEG; ++k) {
            wx[k] = k < cx ? ax.w[0][x0 + k] : 0.0;
            ix[k] = k < cx ? ax.in[0][x0 + k] : 0;
        }
        for (i64 sz = z0; sz < z1; ++sz) {
            const double wz = ax.w[2][sz];
            const i64 bz = ax.in[2][sz] * nxy;
            for (i64 sy = y0; sy < y1; ++sy) {
                const double wzy = wz * ax.w[1][sy];
                const T* row = v + bz + ax.in[1][sy] * nx;
                T r[EMG_RGD_XSEG];
#pragma unroll
                for (int k = 0; k < EMG_RGD_XSEG; ++k) if (k < cx) r[k] = row[ix[k]];
#pragma unroll
                for (int k = 0; k < EMG_RGD_XSEG; ++k) if (k < cx) add_weighted(acc, wzy * wx[k], r[k]);
            }
        }
    } else {
        for (i64 sz = z0; sz < z1; ++sz) {
            const double wz = ax.w[2][sz];
            const i64 bz = ax.in[2][sz] * nxy;
            for (i64 sy = y0; sy < y1; ++sy) {
                const double wzy = wz * ax.w[1][sy];
                const T* row = v + bz + ax.in[1][sy] * nx;
                for (i64 sx = x0; sx < x1; ++sx) add_weighted(acc, wzy * ax.w[0][sx], row[ax.in[0][sx]]);
            }
        }
    }
    out[o] = div_vol<T>(acc, vol[o]);
}

// ---- the transpose of volume averaging (maps.volume_average_adjoint, emg3d_mg_grad_acc(3)_get_model) ------------------------
// With A[o, i] = (sum of the segment weights (w_z w_y) w_x of new cell o that lie in old cell i) / vol[o] -- what
// k_volume_average applies to a zero new array --, out = Q (.) A^T (F (.) y): y, F, vol on the NEW grid (m cells), out and Q on
// the OLD grid (n cells).  The segments of an axis come out in ascending coordinate order, so they are sorted by old cell too:
// old cell i owns the contiguous range [iptr[i], iptr[i+1]) (old_cell_offsets_host).  Two launches: k_regrid_scale streams
// t[o] = (F[o] y[o]) / vol[o] into scratch (a term of the sum then costs one load, not three), k_volume_average_adjoint is a
// gather, one thread per OLD cell, x fastest (the writes coalesce; no atomics, the result does not depend on the schedule):
// out[i] = Q[i] * sum_sz sum_sy sum_sx ((w_z w_y) w_x) t[o], z outermost, segments ascending, from 0, nothing fused.  An old cell
// without a segment (the old grid reaches beyond the new one) gets an exact 0.  Bytes: y, F read once, t written and read once
// (neighbouring threads read neighbouring new cells), Q read and out written once.  double only: gradients are real.
struct VolAvgAdjAxes {
    const i64* iptr[3];         // per axis: segment offsets of the OLD cells (n + 1)
    const i64* out[3];          // per axis: new cell of each segment
    const double* w[3];         // per axis: segment length
};

// x1 cells n, ns segments with old cells in[] (ascending): iptr[0 .. n], old cell i owns segments [iptr[i], iptr[i+1])
inline void old_cell_offsets_host(const i64* in, i64 ns, i64 n, i64* iptr) {
    for (i64 i = 0; i <= n; ++i) iptr[i] = 0;
    for (i64 s = 0; s < ns; ++s) ++iptr[in[s] + 1];
    for (i64 i = 0; i < n; ++i) iptr[i + 1] += iptr[i];
}

// t[o] = (F[o] y[o]) / vol[o]; F == nullptr: F = 1; vol == nullptr: vol = (h0 h1) h2, the product of meshes.cell_volumes
__global__ __launch_bounds__(EMG_RGD_BLOCK) void k_regrid_scale(double* t, const double* y, const double* F, const double* vol,
                                                                const double* h0, const double* h1, const double* h2, i64 mx,
                                                                i64 my, i64 mtot) {
#pragma clang fp contract(off)
    const i64 o = (i64)blockIdx.x * EMG_RGD_BLOCK + threadIdx.x;
    if (o >= mtot) return;
    double v;
    if (vol) v = vol[o];
    else {
        const i64 ox = o % mx, oyz = o / mx;
        v = (h0[ox] * h1[oyz % my]) * h2[oyz / my];
    }
    const double fy = F ? F[o] * y[o] : y[o];
    t[o] = fy / v;
}

__global__ __launch_bounds__(EMG_RGD_BLOCK) void k_volume_average_adjoint(double* out, const double* t, const double* Q, i64 nx,
                                                                          i64 ny, i64 mx, i64 my, i64 ntot, VolAvgAdjAxes ax) {
#pragma clang fp contract(off)      // the arithmetic is part of the contract: the NumPy restatement does not fuse either
    const i64 i = (i64)blockIdx.x * EMG_RGD_BLOCK + threadIdx.x;
    if (i >= ntot) return;
    const i64 ix = i % nx, iyz = i / nx;
    const i64 iy = iyz % ny, iz = iyz / ny;
    const i64 x0 = ax.iptr[0][ix], x1 = ax.iptr[0][ix + 1];
    const i64 y0 = ax.iptr[1][iy], y1 = ax.iptr[1][iy + 1];
    const i64 z0 = ax.iptr[2][iz], z1 = ax.iptr[2][iz + 1];
    const i64 mxy = mx * my;
    double acc = 0.0;
    if (x1 - x0 <= EMG_RGD_XSEG) {
        // the thread's x segments in registers, the loads of a row issued together, then summed in the same order
        const int cx = (int)(x1 - x0);
        double wx[EMG_RGD_XSEG];
        i64 ox[EMG_RGD_XSEG];
#pragma unroll
        for (int k = 0; k < EMG_RGD_XSEG; ++k) {
            wx[k] = k < cx ? ax.w[0][x0 + k] : 0.0;
            ox[k] = k < cx ? ax.out[0][x0 + k] : 0;
        }
        for (i64 sz = z0; sz < z1; ++sz) {
            const double wz = ax.w[2][sz];
            const i64 bz = ax.out[2][sz] * mxy;
            for (i64 sy = y0; sy < y1; ++sy) {
                const double wzy = wz * ax.w[1][sy];
                const double* row = t + bz + ax.out[1][sy] * mx;
                double r[EMG_RGD_XSEG];
#pragma unroll
                for (int k = 0; k < EMG_RGD_XSEG; ++k) if (k < cx) r[k] = row[ox[k]];
#pragma unroll
                for (int k = 0; k < EMG_RGD_XSEG; ++k) if (k < cx) add_weighted(acc, wzy * wx[k], r[k]);
            }
        }
    } else {
        for (i64 sz = z0; sz < z1; ++sz) {
            const double wz = ax.w[2][sz];
            const i64 bz = ax.out[2][sz] * mxy;
            for (i64 sy = y0; sy < y1; ++sy) {
                const double wzy = wz * ax.w[1][sy];
                const double* row = t + bz + ax.out[1][sy] * mx;
                for (i64 sx = x0; sx < x1; ++sx) add_weighted(acc, wzy * ax.w[0][sx], row[ax.out[0][sx]]);
            }
        }
    }
    out[i] = Q ? Q[i] * acc : acc;
}

// the two launches on `stream`: out (n cells) = Q (.) A^T (F (.) y), t = scratch of m cells
inline void volume_average_adjoint_launch(hipStream_t stream, double* out, double* t, const double* y, const double* F,
                                          const double* Q, const double* vol, const double* h0, const double* h1, const double* h2,
                                          const i64 n[3], const i64 m[3], const VolAvgAdjAxes& ax) {
    const i64 ntot = n[0] * n[1] * n[2], mtot = m[0] * m[1] * m[2];
    hipLaunchKernelGGL(k_regrid_scale, dim3((unsigned)((mtot + EMG_RGD_BLOCK - 1) / EMG_RGD_BLOCK)), dim3(EMG_RGD_BLOCK), 0, stream,
                       t, y, F, vol, h0, h1, h2, m[0], m[1], mtot);
    hipLaunchKernelGGL(k_volume_average_adjoint, dim3((unsigned)((ntot + EMG_RGD_BLOCK - 1) / EMG_RGD_BLOCK)), dim3(EMG_RGD_BLOCK), 0,
                       stream, out, (const double*)t, Q, n[0], n[1], m[0], m[1], ntot, ax);
}

// Tensor-product targets: point r = i + mx (j + my k) at (cx[i], cy[j], cz[k]) (index coordinates of `coef`).
template <class T>
__global__ __launch_bounds__(EMG_RCV_BLOCK) void k_spline_eval_grid(T* out, const T* coef, i64 n0, i64 n1, i64 n2, const double* cx,
                                                                    const double* cy, const double* cz, i64 mx, i64 my, i64 npts,
                                                                    double cval, int edge) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= npts) return;
    const i64 i = r % mx, jk = r / mx;
    const i64 j = jk % my, k = jk / my;
    out[r] = spline_point<T>(coef, n0, n1, n2, [&](int a) { return a == 0 ? cx[i] : a == 1 ? cy[j] : cz[k]; }, cval, edge);
}

// Tensor-product targets of k_linear_eval: per axis a, ii[a] / tt[a] / ins[a] (offsets 0, mx, mx + my) of each coordinate.
template <class T>
__global__ __launch_bounds__(EMG_RCV_BLOCK) void k_linear_eval_grid(T* out, const T* values, i64 s0, i64 s1, i64 s2, const int* ii,
                                                                    const double* tt, const int* ins, i64 mx, i64 my, i64 npts,
                                                                    double fill) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= npts) return;
    const i64 i = r % mx, jk = r / mx;
    const i64 j = mx + jk % my, k = mx + my + jk / my;
    T val;
    if (!(ins[i] && ins[j] && ins[k])) {
        val = Zero<T>::v();
        add_real(val, fill);            // fill_value is a real scalar (complex values: fill + 0j)
    } else {
        val = linear_point<T>(values, s0, s1, s2, ii[i], ii[j], ii[k], tt[i], tt[j], tt[k]);
    }
    out[r] = val;
}

// ---- host drivers ------------------------------------------------------------------------------------------------
// volume_average(edges, values, new_edges, new_values, new_vol) of host arrays (F-ordered; new_values in and out).
template <class T>
int volume_average_host(const i64 n[3], const double* const edges[3], const T* values, const i64 m[3],
                        const double* const new_edges[3], T* new_values, const double* new_vol) {
    for (int a = 0; a < 3; ++a) if (n[a] < 1 || m[a] < 1) return -2;
    std::vector<double> w[3];
    std::vector<i64> in[3], out[3], ptr[3];
    i64 ns[3];
    for (int a = 0; a < 3; ++a) {
        const i64 cap = n[a] + m[a] + 1;
        w[a].resize(cap); in[a].resize(cap); out[a].resize(cap); ptr[a].resize(m[a] + 1);
        ns[a] = volume_average_weights_host(edges[a], n[a] + 1, new_edges[a], m[a] + 1, w[a].data(), in[a].data(),
                                            out[a].data(), ptr[a].data());
    }
    const i64 tot = n[0] * n[1] * n[2], mtot = m[0] * m[1] * m[2];
    // one block: [values | new_values | new_vol | per axis: ptr, in, w] (every part a multiple of 8 bytes)
    size_t nb = (size_t)tot * sizeof(T) + (size_t)mtot * (sizeof(T) + sizeof(double));
    for (int a = 0; a < 3; ++a) nb += (size_t)(m[a] + 1) * sizeof(i64) + (size_t)ns[a] * (sizeof(i64) + sizeof(double));
    DevBlock blk;
    HIP_TRY(blk.alloc(nb));
    char* p = blk.get<char>();
    T* dv = (T*)p;              p += (size_t)tot * sizeof(T);
    T* dout = (T*)p;            p += (size_t)mtot * sizeof(T);
    double* dvol = (double*)p;  p += (size_t)mtot * sizeof(double);
    VolAvgAxes ax;
    for (int a = 0; a < 3; ++a) {
        i64* dp = (i64*)p;      p += (size_t)(m[a] + 1) * sizeof(i64);
        i64* di = (i64*)p;      p += (size_t)ns[a] * sizeof(i64);
        double* dw = (double*)p; p += (size_t)ns[a] * sizeof(double);
        HIP_TRY(hipMemcpy(dp, ptr[a].data(), (size_t)(m[a] + 1) * sizeof(i64), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(di, in[a].data(), (size_t)ns[a] * sizeof(i64), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dw, w[a].data(), (size_t)ns[a] * sizeof(double), hipMemcpyHostToDevice));
        ax.ptr[a] = dp; ax.in[a] = di; ax.w[a] = dw;
    }
    HIP_TRY(hipMemcpy(dv, values, (size_t)tot * sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dout, new_values, (size_t)mtot * sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dvol, new_vol, (size_t)mtot * sizeof(double), hipMemcpyHostToDevice));
    const i64 nblk = (mtot + EMG_RGD_BLOCK - 1) / EMG_RGD_BLOCK;
    hipLaunchKernelGGL(k_volume_average<T>, dim3((unsigned)nblk), dim3(EMG_RGD_BLOCK), 0, nullptr, dout, (const T*)dv,
                       (const double*)dvol, n[0], n[1], m[0], m[1], mtot, ax);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(new_values, dout, (size_t)mtot * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

// The segments of the three axes with both sets of offsets: new-cell (ptr, k_volume_average) and old-cell (iptr, the adjoint).
struct VolAvgTables {
    std::vector<double> w[3];
    std::vector<i64> in[3], out[3], ptr[3], iptr[3];
    i64 ns[3];
    void build(const i64 n[3], const double* const edges[3], const i64 m[3], const double* const new_edges[3]) {
        for (int a = 0; a < 3; ++a) {
            const i64 cap = n[a] + m[a] + 1;
            w[a].resize(cap); in[a].resize(cap); out[a].resize(cap); ptr[a].resize(m[a] + 1); iptr[a].resize(n[a] + 1);
            ns[a] = volume_average_weights_host(edges[a], n[a] + 1, new_edges[a], m[a] + 1, w[a].data(), in[a].data(),
                                                out[a].data(), ptr[a].data());
            old_cell_offsets_host(in[a].data(), ns[a], n[a], iptr[a].data());
        }
    }
};

// out = A^T y of host arrays (F-ordered): y and new_vol on the new grid (m cells), out on the old grid (n cells).
inline int volume_average_adjoint_host(const i64 n[3], const double* const edges[3], const i64 m[3],
                                       const double* const new_edges[3], const double* y, const double* new_vol, double* out) {
    for (int a = 0; a < 3; ++a) if (n[a] < 1 || m[a] < 1) return -2;
    VolAvgTables tb;
    tb.build(n, edges, m, new_edges);
    const i64 tot = n[0] * n[1] * n[2], mtot = m[0] * m[1] * m[2];
    // one block: [y | new_vol | t | out | per axis: iptr, out, w] (every part a multiple of 8 bytes)
    size_t nb = (size_t)(3 * mtot + tot) * sizeof(double);
    for (int a = 0; a < 3; ++a) nb += (size_t)(n[a] + 1) * sizeof(i64) + (size_t)tb.ns[a] * (sizeof(i64) + sizeof(double));
    DevBlock blk;
    HIP_TRY(blk.alloc(nb));
    char* p = blk.get<char>();
    double* dy = (double*)p;    p += (size_t)mtot * sizeof(double);
    double* dvol = (double*)p;  p += (size_t)mtot * sizeof(double);
    double* dt = (double*)p;    p += (size_t)mtot * sizeof(double);
    double* dout = (double*)p;  p += (size_t)tot * sizeof(double);
    VolAvgAdjAxes ax;
    for (int a = 0; a < 3; ++a) {
        i64* dp = (i64*)p;      p += (size_t)(n[a] + 1) * sizeof(i64);
        i64* dn = (i64*)p;      p += (size_t)tb.ns[a] * sizeof(i64);
        double* dw = (double*)p; p += (size_t)tb.ns[a] * sizeof(double);
        HIP_TRY(hipMemcpy(dp, tb.iptr[a].data(), (size_t)(n[a] + 1) * sizeof(i64), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dn, tb.out[a].data(), (size_t)tb.ns[a] * sizeof(i64), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dw, tb.w[a].data(), (size_t)tb.ns[a] * sizeof(double), hipMemcpyHostToDevice));
        ax.iptr[a] = dp; ax.out[a] = dn; ax.w[a] = dw;
    }
    HIP_TRY(hipMemcpy(dy, y, (size_t)mtot * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dvol, new_vol, (size_t)mtot * sizeof(double), hipMemcpyHostToDevice));
    volume_average_adjoint_launch(nullptr, dout, dt, dy, nullptr, nullptr, dvol, nullptr, nullptr, nullptr, n, m, ax);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout, (size_t)tot * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// interp3d on tensor-product targets: values F-ordered (n0, n1, n2) on the host, targets xi[a] (m[a] coordinates per axis),
// out F-ordered (m0, m1, m2) on the host.  method / has_fill / fill / cval as in interp3d_device.
template <class T>
int interp3d_grid_host(const i64 n[3], const double* const pts[3], const T* values, const i64 m[3], const double* const xi[3],
                       int method, bool has_fill, double fill, double cval, T* out) {
    for (int a = 0; a < 3; ++a) if (n[a] < 1 || m[a] < 1) return -2;
    for (int a = 0; a < 3; ++a) if (n[a] < 4 && method < 2) method = 0;             // maps.py:238-240
    if (method >= 2) for (int a = 0; a < 3; ++a) if (n[a] < 4) return -2;
    const i64 tot = n[0] * n[1] * n[2], npts = m[0] * m[1] * m[2], msum = m[0] + m[1] + m[2];
    T *dv = nullptr, *dout = nullptr;
    DEV_ALLOC(dv, (size_t)tot * sizeof(T));
    DEV_ALLOC(dout, (size_t)npts * sizeof(T));
    double* dco = nullptr;                                  // per-axis index coordinates (cubic) / distances (linear)
    DEV_ALLOC(dco, (size_t)msum * sizeof(double));
    int *dii = nullptr, *dins = nullptr;                    // per-axis interval index / inside flag (linear)
    DEV_ALLOC(dii, (size_t)msum * sizeof(int));
    DEV_ALLOC(dins, (size_t)msum * sizeof(int));
    HIP_TRY(hipMemcpy(dv, values, (size_t)tot * sizeof(T), hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)((npts + EMG_RCV_BLOCK - 1) / EMG_RCV_BLOCK);
    if (method >= 1) {
        std::vector<double> co((size_t)msum);
        double* c = co.data();
        for (int a = 0; a < 3; ++a) {
            if (method >= 2) std::copy(xi[a], xi[a] + m[a], c);
            else notaknot_index_coords(pts[a], n[a], xi[a], m[a], c);
            c += m[a];
        }
        HIP_TRY(hipMemcpy(dco, co.data(), co.size() * sizeof(double), hipMemcpyHostToDevice));
        // spline coefficients: filter the three axes of the uploaded copy in place
        for (int a = 0; a < 3; ++a) {
            const i64 nl = tot / n[a];
            hipLaunchKernelGGL(k_spline_filter_axis<T>, dim3((unsigned)((nl + 63) / 64)), dim3(64), 0, nullptr, dv, n[0], n[1], n[2],
                               a, (method == 3 || method == 4) ? 1 : 0);
        }
        hipLaunchKernelGGL(k_spline_eval_grid<T>, dim3(blocks), dim3(EMG_RCV_BLOCK), 0, nullptr, dout, (const T*)dv, n[0], n[1], n[2],
                           (const double*)dco, (const double*)(dco + m[0]), (const double*)(dco + m[0] + m[1]), m[0], m[1], npts,
                           cval, method == 3 ? 1 : method == 2 ? 2 : method == 4 ? 3 : 0);
    } else {
        std::vector<int> ii((size_t)msum), ins((size_t)msum);
        std::vector<double> tt((size_t)msum);
        i64 off = 0;
        for (int a = 0; a < 3; ++a) {
            const double* g = pts[a];
            for (i64 r = 0; r < m[a]; ++r, ++off) {
                const double v = xi[a][r];
                ins[off] = (has_fill && !(v >= g[0] && v <= g[n[a] - 1])) ? 0 : 1;
                i64 i = (i64)(std::lower_bound(g, g + n[a], v) - g) - 1;
                if (i < 0) i = 0;
                if (i > n[a] - 2) i = n[a] - 2;
                if (n[a] == 1) {                // one point: both corners are that point (stride zeroed below)
                    ii[off] = 0;
                    tt[off] = 0.0;
                    continue;
                }
                ii[off] = (int)i;
                tt[off] = (v - g[i]) / (g[i + 1] - g[i]);
            }
        }
        HIP_TRY(hipMemcpy(dco, tt.data(), tt.size() * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dii, ii.data(), ii.size() * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dins, ins.data(), ins.size() * sizeof(int), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_linear_eval_grid<T>, dim3(blocks), dim3(EMG_RCV_BLOCK), 0, nullptr, dout, (const T*)dv,
                           n[0] == 1 ? (i64)0 : (i64)1, n[1] == 1 ? (i64)0 : n[0], n[2] == 1 ? (i64)0 : n[0] * n[1],
                           (const int*)dii, (const double*)dco, (const int*)dins, m[0], m[1], npts, fill);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout, (size_t)npts * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}
