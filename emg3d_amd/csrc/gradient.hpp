// Adjoint-state gradient pieces on the device:
//   k_edges2cell  = maps.edges2cellaverages (reference emg3d/maps.py:578-630): edge values -> volume-weighted cell
//                   averages, one output array per component;
//   k_gradient    = optimize.gradient for one (source, frequency) pair on its computational grid (reference
//                   emg3d/optimize.py:176-199): -Re(lambda E s mu_0) on the edges, mapped to cells, components added;
//   k_gradient_acc = the same for all systems of a batch in one launch, added into a per-cell accumulator in system order;
//   k_sens_acc    = the survey sensitivity diagonal: W |row|^2 for all pairs of an adjoint and a forward system, into the same
//                   accumulators (no counterpart in the reference);
//   k_sens_rows   = the rows themselves, one per pair, into a planar row buffer (MG::sens_rows);
//   k_sens_rows_fill = the same rows, real and imaginary parts written straight into their rows of a row store (MG::sens_rows_fill;
//                   instantiated in csrc/rows.hip, the store's translation unit).
// The last five are the per-cell kernels: one thread per cell behind the same cell_frame, SPLIT = the sum of the three directions
// or the directions apart, launched through MG_CELL_LAUNCH (mg.hpp), the accumulators those of MG::cell_acc.
// Gather form: one thread per CELL sums the contributions of its 12 edges in the order in which the reference's
// loops (iz, iy, ix ascending, four statements per edge) add them -- deterministic and equal to the reference's
// accumulation order, no atomics.
#pragma once
#include "common.hpp"

// What the reference adds into cell (j0, j1, j2) for component c: sum over the cell's four c-edges (and the
// duplicated boundary statements) of vol * f / 4.  F(i0, i1, i2) returns the edge value.
template <class V, class F>
__device__ __forceinline__ V e2c_component(int c, const i64 j[3], const i64 nC[3], double vol, F f) {
    const int t1 = (c == 0) ? 1 : 0, t2 = (c == 2) ? 1 : 2;       // transverse axes, t1 < t2 (t2 is the outer loop)
    V acc = V();
    for (i64 e2 = j[t2]; e2 <= j[t2] + 1; ++e2) {
        const i64 m2 = e2 > 0 ? e2 - 1 : 0, p2 = e2 < nC[t2] - 1 ? e2 : nC[t2] - 1;
        for (i64 e1 = j[t1]; e1 <= j[t1] + 1; ++e1) {
            const i64 m1 = e1 > 0 ? e1 - 1 : 0, p1 = e1 < nC[t1] - 1 ? e1 : nC[t1] - 1;
            i64 e[3];
            e[c] = j[c]; e[t1] = e1; e[t2] = e2;
            const V v = (vol * f(e[0], e[1], e[2])) / 4.0;
            // the four statements of the reference, in its order: (m1, m2), (p1, m2), (m1, p2), (p1, p2)
            if (m1 == j[t1] && m2 == j[t2]) acc += v;
            if (p1 == j[t1] && m2 == j[t2]) acc += v;
            if (m1 == j[t1] && p2 == j[t2]) acc += v;
            if (p1 == j[t1] && p2 == j[t2]) acc += v;
        }
    }
    return acc;
}

template <class T>
struct E2CArgs {
    i64 nC[3];
    FieldLayout fl;
    const T* f;              // [fx|fy|fz]
    const double* vol;       // F-ordered (nx, ny, nz) cell volumes, or NULL: hx*hy*hz from h
    const double* h[3];
    T* out[3];               // out_x, out_y, out_z (+=)
};

template <class T>
__global__ void k_edges2cell(E2CArgs<T> a) {
    const i64 n = a.nC[0] * a.nC[1] * a.nC[2];
    const i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const i64 j[3] = {idx % a.nC[0], (idx / a.nC[0]) % a.nC[1], idx / (a.nC[0] * a.nC[1])};
    const double vol = a.vol ? a.vol[idx] : (a.h[0][j[0]] * a.h[1][j[1]]) * a.h[2][j[2]];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const T* comp = a.f + a.fl.off[c];
        const i64 s0 = a.fl.st[c][0], s1 = a.fl.st[c][1], s2 = a.fl.st[c][2];
        a.out[c][idx] += e2c_component<T>(c, j, a.nC, vol, [&](i64 i0, i64 i1, i64 i2) { return comp[i0 * s0 + i1 * s1 + i2 * s2]; });
    }
}

__device__ __forceinline__ double grad_prod(double b, double e, double s, double) { return -((b * e) * s); }
__device__ __forceinline__ double grad_prod(c128 b, c128 e, double sr, double si) {
    const c128 be = b * e;                         // -real(bfield * efield * smu0), optimize.py:181-184
    return -(be.re * sr - be.im * si);
}

// The three components of one cell's gradient value: g[c] = edges2cellaverages_c( -Re(b * e * smu0) ) at cell j.  One body for
// k_gradient and k_gradient_acc, so that both round (and contract) alike.
template <class T>
__device__ __forceinline__ void grad_cell(const i64 j[3], const i64 nC[3], double vol, const FieldLayout& fl, const T* e, const T* b,
                                          double sr, double si, double g[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const T* ec = e + fl.off[c];
        const T* bc = b + fl.off[c];
        const i64 s0 = fl.st[c][0], s1 = fl.st[c][1], s2 = fl.st[c][2];
        g[c] = e2c_component<double>(c, j, nC, vol, [&](i64 i0, i64 i1, i64 i2) {
            const i64 o = i0 * s0 + i1 * s1 + i2 * s2;
            return grad_prod(bc[o], ec[o], sr, si);
        });
    }
}

// The frame of one thread of the per-cell kernels (k_gradient, k_gradient_acc, k_sens_acc): its cell idx -> (j0, j1, j2), x fastest,
// and vol = (hx*hy)*hz (meshes cell_volumes).  false: the thread has no cell.
__device__ __forceinline__ bool cell_frame(i64 n0, i64 n1, i64 n2, const double* h0, const double* h1, const double* h2, i64& idx,
                                           i64 j[3], double& vol) {
    idx = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n0 * n1 * n2) return false;
    j[0] = idx % n0; j[1] = (idx / n0) % n1; j[2] = idx / (n0 * n1);
    vol = (h0[j[0]] * h1[j[1]]) * h2[j[2]];
    return true;
}

// The running sums of a cell: one read and one write of acc (SPLIT: of acc, acc1, acc2) per thread and launch.
template <bool SPLIT>
__device__ __forceinline__ void acc_load(i64 idx, const double* acc, const double* acc1, const double* acc2, double& run, double& run1,
                                         double& run2) {
    run = acc[idx]; run1 = 0.0; run2 = 0.0;
    if (SPLIT) { run1 = acc1[idx]; run2 = acc2[idx]; }
}
template <bool SPLIT>
__device__ __forceinline__ void acc_store(i64 idx, double* acc, double* acc1, double* acc2, double run, double run1, double run2) {
    acc[idx] = run;
    if (SPLIT) { acc1[idx] = run1; acc2[idx] = run2; }
}

// grad[cell] = sum_c edges2cellaverages_c( -Re(b * e * smu0) ), vol = (hx*hy)*hz (meshes cell_volumes).
// SPLIT: the three components go to g0, g1, g2 instead (emg3d_mg_gradient3); their sum (g0 + g1) + g2 is the one-output result.
template <class T, bool SPLIT>
__global__ void k_gradient(i64 n0, i64 n1, i64 n2, FieldLayout fl, const T* e, const T* b, double sr, double si,
                           const double* h0, const double* h1, const double* h2, double* g0, double* g1, double* g2) {
    const i64 nC[3] = {n0, n1, n2};
    i64 idx, j[3];
    double vol;
    if (!cell_frame(n0, n1, n2, h0, h1, h2, idx, j, vol)) return;
    double g[3];
    grad_cell<T>(j, nC, vol, fl, e, b, sr, si, g);
    if (SPLIT) { g0[idx] = g[0]; g1[idx] = g[1]; g2[idx] = g[2]; }
    else g0[idx] = (g[0] + g[1]) + g[2];          // grad_x + grad_y + grad_z, optimize.py:199
}

// Survey gradient (optimize.survey_gradient): acc[cell] = (((acc[cell] + g_0) + g_1) + ...) over the systems b = 0 .. nsys-1 (ascending)
// whose bit is set in `use`, g_b = what k_gradient<T, false> gives for the forward field e + b * nE (slice b of a batched vector) and
// the back-propagated field bk + b * nE (slice b of the level-0 field array).  One thread per cell, one read and one write of acc, no
// atomics: the order of the sum is fixed.  Per active system the two fields are read once (2 nE sizeof(T) bytes).
// SPLIT (optimize.SurveyJacobian, components=True): three accumulators, acc_c += g_c,b with g_c,b what k_gradient<T, true> gives --
// the same grad_cell, its three results kept apart instead of added.
template <class T, bool SPLIT>
__global__ void k_gradient_acc(i64 n0, i64 n1, i64 n2, FieldLayout fl, const T* e, const T* bk, i64 nE, int nsys, unsigned long long use,
                               double sr, double si, const double* h0, const double* h1, const double* h2, double* acc, double* acc1,
                               double* acc2) {
    const i64 nC[3] = {n0, n1, n2};
    i64 idx, j[3];
    double vol;
    if (!cell_frame(n0, n1, n2, h0, h1, h2, idx, j, vol)) return;
    double run, run1, run2;
    acc_load<SPLIT>(idx, acc, acc1, acc2, run, run1, run2);
    for (int b = 0; b < nsys; ++b) {
        if (!((use >> b) & 1ull)) continue;
        double g[3];
        grad_cell<T>(j, nC, vol, fl, e + (i64)b * nE, bk + (i64)b * nE, sr, si, g);
        if (SPLIT) { run += g[0]; run1 += g[1]; run2 += g[2]; }
        else run += (g[0] + g[1]) + g[2];
    }
    acc_store<SPLIT>(idx, acc, acc1, acc2, run, run1, run2);
}

// ---- survey sensitivity diagonal: diag(J^H W J) (optimize.SurveyJacobian.sensitivity_diagonal) -----------------------------
// Row (source s, receiver r) of J at a cell is c = c_x + c_y + c_z, c_c = edges2cellaverages_c(s mu_0 lambda_r E_s): the operator is
// complex symmetric, so lambda_r, the field of receiver r's adjoint source ALONE, serves every source.  An all-pairs product: the
// real part is NOT taken before averaging (the row is complex), and the sum over the pairs is one of squares.
__device__ __forceinline__ double sens_prod(double l, double e, double sr, double) { return (l * e) * sr; }
__device__ __forceinline__ c128 sens_prod(c128 l, c128 e, double sr, double si) { return (l * e) * mk(sr, si); }
__device__ __forceinline__ double sens_abs2(double c) { return c * c; }
__device__ __forceinline__ double sens_abs2(c128 c) { return c.re * c.re + c.im * c.im; }

// The twelve edges of a cell: component c, edge k = (i_t1 - j_t1) + 2 (i_t2 - j_t2) with the transverse axes t1 < t2 of
// e2c_component -- the order in which its loops visit them.  Indexed with compile-time constants only (registers, no scratch).
template <class V>
struct CellEdges { V v[3][4]; };

__device__ __forceinline__ void cell_edge_offsets(const i64 j[3], const FieldLayout& fl, CellEdges<i64>& o) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int t1 = (c == 0) ? 1 : 0, t2 = (c == 2) ? 1 : 2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            i64 e[3];
            e[c] = j[c]; e[t1] = j[t1] + (k & 1); e[t2] = j[t2] + (k >> 1);
            o.v[c][k] = fl.off[c] + e[0] * fl.st[c][0] + e[1] * fl.st[c][1] + e[2] * fl.st[c][2];
        }
    }
}
template <class T>
__device__ __forceinline__ void cell_edge_load(const T* f, const CellEdges<i64>& o, CellEdges<T>& out) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) out.v[c][k] = f[o.v[c][k]];
}

// The three components of one row of J at cell j: cc[c] = edges2cellaverages_c( (lambda * E) * s mu_0 ), the four statements per
// edge those of grad_cell (e2c_component), the edge values taken from registers.  One body for both forms of k_sens_acc.
template <class T>
__device__ __forceinline__ void sens_cell(const i64 j[3], const i64 nC[3], double vol, const CellEdges<T>& lam, const CellEdges<T>& ev,
                                          double sr, double si, T cc[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int t1 = (c == 0) ? 1 : 0, t2 = (c == 2) ? 1 : 2;
        const T(&lc)[4] = lam.v[c];
        const T(&ec)[4] = ev.v[c];
        cc[c] = e2c_component<T>(c, j, nC, vol, [&](i64 i0, i64 i1, i64 i2) {
            const i64 i[3] = {i0, i1, i2};
            const bool q1 = i[t1] != j[t1], q2 = i[t2] != j[t2];          // (selects, not an index: nothing to spill)
            const T l = q2 ? (q1 ? lc[3] : lc[2]) : (q1 ? lc[1] : lc[0]);
            const T e = q2 ? (q1 ? ec[3] : ec[2]) : (q1 ? ec[1] : ec[0]);
            return sens_prod(l, e, sr, si);
        });
    }
}

// acc[cell] += W[b_r nsys + b_s] |(c_x + c_y) + c_z|^2 over the pairs (b_r, b_s) -- LOOP ORDER (part of the contract): the adjoint
// systems b_r with bit b_r of `use_adj` set, ascending, outer; the forward systems b_s with bit b_s of `use_fwd` set, ascending,
// inner; a pair with W == 0 is skipped (no load, no term).  lambda_{b_r} = slice b_r of the level-0 field array `adj`, E_{b_s} =
// slice b_s of the batched vector `fwd`.  SPLIT: acc, acc1, acc2 += W |c_x|^2, W |c_y|^2, W |c_z|^2.  One thread per cell, one read
// and one write of each accumulator, no atomics; the twelve lambda values of a receiver stay in registers across the inner loop.
// Per launch a lambda field is read once, an E field once per active adjoint system (twelve edge values per cell and use, each
// edge shared by up to four cells through the caches): at most (n_adj + pairs) nE sizeof(T) bytes from HBM; W is wave-uniform and
// comes through the scalar cache.  Launched with 256 threads: the bound lets the complex
// kernel keep its 2 x 12 edge values and 12 offsets in registers (the default bound of 1024 threads caps it at 128 and spills).
template <class T, bool SPLIT>
__global__ void __launch_bounds__(256) k_sens_acc(i64 n0, i64 n1, i64 n2, FieldLayout fl, const T* fwd, const T* adj, i64 nE, int nsys, unsigned long long use_fwd,
                           unsigned long long use_adj, const double* W, double sr, double si, const double* h0, const double* h1,
                           const double* h2, double* acc, double* acc1, double* acc2) {
    const i64 nC[3] = {n0, n1, n2};
    i64 idx, j[3];
    double vol;
    if (!cell_frame(n0, n1, n2, h0, h1, h2, idx, j, vol)) return;
    if (nsys < 64) {                    // (never a shift by 64: nsys = 64 with bit 63 set is a valid batch)
        use_fwd &= (1ull << nsys) - 1ull;
        use_adj &= (1ull << nsys) - 1ull;
    }
    CellEdges<i64> o;
    cell_edge_offsets(j, fl, o);
    double run, run1, run2;
    acc_load<SPLIT>(idx, acc, acc1, acc2, run, run1, run2);
    for (unsigned long long ra = use_adj; ra; ra &= ra - 1ull) {          // (wave-uniform: the masks are kernel arguments)
        const int br = __builtin_ctzll(ra);
        const double* Wr = W + (i64)br * nsys;
        CellEdges<T> lam;
        cell_edge_load(adj + (i64)br * nE, o, lam);
        for (unsigned long long rf = use_fwd; rf; rf &= rf - 1ull) {
            const int bs = __builtin_ctzll(rf);
            const double w = Wr[bs];
            if (w == 0.0) continue;
            CellEdges<T> ev;
            cell_edge_load(fwd + (i64)bs * nE, o, ev);
            T cc[3];
            sens_cell<T>(j, nC, vol, lam, ev, sr, si, cc);
            if (SPLIT) { run += w * sens_abs2(cc[0]); run1 += w * sens_abs2(cc[1]); run2 += w * sens_abs2(cc[2]); }
            else run += w * sens_abs2((cc[0] + cc[1]) + cc[2]);
        }
    }
    acc_store<SPLIT>(idx, acc, acc1, acc2, run, run1, run2);
}

// ---- explicit rows of J (optimize.SurveyJacobian.sensitivity_rows) ----------------------------------------------------------
// One plane of a row is nC doubles; a complex value goes to two planes (re, then im), a real one to one.
__device__ __forceinline__ void row_store(double* p, i64, double c) { p[0] = c; }
__device__ __forceinline__ void row_store(double* p, i64 plane, c128 c) { p[0] = c.re; p[plane] = c.im; }

// The rows k_sens_acc squares, kept: rows[p][dir][part][cell] = row (b_r, b_s) of J at the cell, p the rank of the pair in
// k_sens_acc's LOOP ORDER (part of the contract: adjoint systems of `use_adj` ascending, outer; forward systems of `use_fwd`
// ascending, inner) -- no weight table, every pair of the two masks is a row.  dir: one plane (c_x + c_y) + c_z, SPLIT: the three
// c_x, c_y, c_z; part: re, im for c128, one plane for double; cells x fastest.  Planar, so that every plane is a real cell array
// (volume_average_adjoint_launch takes it as it is) and a wave stores 64 consecutive doubles.  The same frame, offsets, loads and
// sens_cell as k_sens_acc: row and |row|^2 round alike.  One thread per cell, every element written exactly once, no atomics, all
// offsets 64-bit; the twelve lambda values of a receiver stay in registers across the inner loop.  Per launch the reads of
// k_sens_acc, plus pairs * NDIR * sizeof(T) * nC bytes written.  `rows` must hold popcount(use_adj) * popcount(use_fwd) (masks
// clipped to nsys bits) * NDIR * NPART * nC doubles.  The two trailing pointers are those of the per-cell launch and not used.
template <class T, bool SPLIT>
__global__ void __launch_bounds__(256) k_sens_rows(i64 n0, i64 n1, i64 n2, FieldLayout fl, const T* fwd, const T* adj, i64 nE, int nsys, unsigned long long use_fwd,
                            unsigned long long use_adj, double sr, double si, const double* h0, const double* h1, const double* h2,
                            double* rows, double*, double*) {
    const i64 nC[3] = {n0, n1, n2};
    i64 idx, j[3];
    double vol;
    if (!cell_frame(n0, n1, n2, h0, h1, h2, idx, j, vol)) return;
    if (nsys < 64) {                    // (never a shift by 64: nsys = 64 with bit 63 set is a valid batch)
        use_fwd &= (1ull << nsys) - 1ull;
        use_adj &= (1ull << nsys) - 1ull;
    }
    constexpr i64 NDIR = SPLIT ? 3 : 1, NPART = (i64)(sizeof(T) / sizeof(double));
    const i64 plane = n0 * n1 * n2;
    CellEdges<i64> o;
    cell_edge_offsets(j, fl, o);
    double* dst = rows + idx;           // this cell in the first plane of pair p
    for (unsigned long long ra = use_adj; ra; ra &= ra - 1ull) {          // (wave-uniform: the masks are kernel arguments)
        const int br = __builtin_ctzll(ra);
        CellEdges<T> lam;
        cell_edge_load(adj + (i64)br * nE, o, lam);
        for (unsigned long long rf = use_fwd; rf; rf &= rf - 1ull) {
            const int bs = __builtin_ctzll(rf);
            CellEdges<T> ev;
            cell_edge_load(fwd + (i64)bs * nE, o, ev);
            T cc[3];
            sens_cell<T>(j, nC, vol, lam, ev, sr, si, cc);
            if (SPLIT) {
                row_store(dst, plane, cc[0]);
                row_store(dst + NPART * plane, plane, cc[1]);
                row_store(dst + 2 * NPART * plane, plane, cc[2]);
            } else {
                row_store(dst, plane, (cc[0] + cc[1]) + cc[2]);
            }
            dst += NDIR * NPART * plane;
        }
    }
}

// ---- the rows of J, both parts, straight into a row store (optimize.SurveyJacobian.park_rows(solves=1)) ----------------------
// Where the fused kernel writes: the block of a row store (csrc/rows.hip: n_cols doubles per row, columns [dir][cell]), the two
// destination tables of the call (device, one entry per pair in LOOP ORDER; a negative entry: that part of the pair is not kept;
// dest_im == nullptr: no imaginary part is kept) and what k_rows_park applies on the way: the store's chain factors (c[0] ==
// nullptr: none) and the sum of the three directions.
struct RowsFillArgs {
    double* R;
    i64 n_cols;
    const int32_t* dest_re;
    const int32_t* dest_im;
    const double* c[3];
    int sum3;
};

__device__ __forceinline__ double sens_part(double c, int) { return c; }
__device__ __forceinline__ double sens_part(c128 c, int part) { return part ? c.im : c.re; }

// One real part of one pair at one cell into its store row: the operations of k_rows_park in their order -- chain factor times
// value per direction, then (p0 + p1) + p2 --, without contraction, so that a filled row is the parked row bit for bit.  The pragma
// covers this body alone: the products of sens_cell keep the flags they have inside k_sens_rows, and none of them can fuse with an
// operation here, which carries no licence to contract.
template <bool SPLIT>
__device__ __forceinline__ void row_fill_part(double* out, i64 plane, double v0, double v1, double v2, bool chain, double ch0, double ch1,
                                              double ch2, int sum3) {
#pragma clang fp contract(off)
    if (chain) {
        v0 = ch0 * v0;
        if (SPLIT) { v1 = ch1 * v1; v2 = ch2 * v2; }
    }
    if (!SPLIT) { out[0] = v0; return; }
    if (sum3) out[0] = (v0 + v1) + v2;
    else { out[0] = v0; out[plane] = v1; out[2 * plane] = v2; }
}

// k_sens_rows with its stores replaced by the work of k_rows_park: the real part of pair p goes to store row dest_re[p], the
// imaginary part (c128) to row dest_im[p], columns [dir][cell] with cells x fastest -- consecutive lanes write consecutive doubles
// of one row.  The same frame, offsets, loads, sens_cell, mask clipping and LOOP ORDER as k_sens_rows (p = the rank of the pair),
// the twelve lambda values of a receiver in registers across the inner loop; a pair with both entries negative is skipped before its
// forward load (wave-uniform: the tables are indexed by the loop counter and come through the scalar cache).  !SPLIT: one column
// block, ((c_x + c_y) + c_z) formed as k_sens_rows forms it, times chain factor 0 if given; SPLIT: three blocks, or with sum3 the
// one block (p0 + p1) + p2 of the (scaled) directions.  One thread per cell, every element of a named row written exactly once, rows
// named in neither table not touched, no atomics, all offsets 64-bit.  Per launch the reads of k_sens_rows (a skipped pair's forward
// field apart) plus three chain factors per cell, and 8 bytes written per element kept: no row buffer, no second pass.  The host
// checks the tables (csrc/rows.hip: rows_fill_check): every entry < n_rows, no row named twice.
template <class T, bool SPLIT>
__global__ void __launch_bounds__(256) k_sens_rows_fill(i64 n0, i64 n1, i64 n2, FieldLayout fl, const T* fwd, const T* adj, i64 nE, int nsys,
                                                        unsigned long long use_fwd, unsigned long long use_adj, double sr, double si,
                                                        const double* h0, const double* h1, const double* h2, RowsFillArgs f) {
    const i64 nC[3] = {n0, n1, n2};
    i64 idx, j[3];
    double vol;
    if (!cell_frame(n0, n1, n2, h0, h1, h2, idx, j, vol)) return;
    if (nsys < 64) {                    // (never a shift by 64: nsys = 64 with bit 63 set is a valid batch)
        use_fwd &= (1ull << nsys) - 1ull;
        use_adj &= (1ull << nsys) - 1ull;
    }
    constexpr bool CPLX = sizeof(T) > sizeof(double);
    const i64 plane = n0 * n1 * n2;
    CellEdges<i64> o;
    cell_edge_offsets(j, fl, o);
    const bool chain = f.c[0] != nullptr;
    double ch0 = 0.0, ch1 = 0.0, ch2 = 0.0;
    if (chain) {
        ch0 = f.c[0][idx];
        if (SPLIT) { ch1 = f.c[1][idx]; ch2 = f.c[2][idx]; }
    }
    double* const out = f.R + idx;      // this cell in the first column block of row 0
    i64 p = 0;
    for (unsigned long long ra = use_adj; ra; ra &= ra - 1ull) {          // (wave-uniform: the masks are kernel arguments)
        const int br = __builtin_ctzll(ra);
        CellEdges<T> lam;
        cell_edge_load(adj + (i64)br * nE, o, lam);
        for (unsigned long long rf = use_fwd; rf; rf &= rf - 1ull, ++p) {
            const i64 dre = f.dest_re[p];
            const i64 dim = (CPLX && f.dest_im) ? (i64)f.dest_im[p] : (i64)-1;
            if (dre < 0 && dim < 0) continue;
            const int bs = __builtin_ctzll(rf);
            CellEdges<T> ev;
            cell_edge_load(fwd + (i64)bs * nE, o, ev);
            T cc[3];
            sens_cell<T>(j, nC, vol, lam, ev, sr, si, cc);
            if (!SPLIT) cc[0] = (cc[0] + cc[1]) + cc[2];
            if (dre >= 0)
                row_fill_part<SPLIT>(out + dre * f.n_cols, plane, sens_part(cc[0], 0), sens_part(cc[1], 0), sens_part(cc[2], 0), chain,
                                     ch0, ch1, ch2, f.sum3);
            if (CPLX && dim >= 0)
                row_fill_part<SPLIT>(out + dim * f.n_cols, plane, sens_part(cc[0], 1), sens_part(cc[1], 1), sens_part(cc[2], 1), chain,
                                     ch0, ch1, ch2, f.sum3);
        }
    }
}

// ---- the transpose: cells -> edges (J v of optimize.Jacobian) ---------------------------------------------------------------
// Gather form again: one thread per EDGE sums the (up to) four cells around it, in ascending cell order -- deterministic, no atomics,
// and never a scatter from the cells.  e2c_component above adds edge (e1, e2) (transverse indices) of component c into the cells
// (m1 | p1, m2 | p2), m = max(e - 1, 0), p = min(e, n - 1): the four statements of the reference, which hit the SAME cell twice (four
// times on a grid corner line) for a boundary edge.  Its transpose therefore gives a boundary edge its cell two / four times.
// W(j0, j1, j2) returns the cell's weight (vol * v); the result is sum W / 4.
template <class V, class W>
__device__ __forceinline__ V c2e_gather(int c, const i64 e[3], const i64 nC[3], W w) {
    const int t1 = (c == 0) ? 1 : 0, t2 = (c == 2) ? 1 : 2;
    const i64 e1 = e[t1], e2 = e[t2];
    const i64 a1[2] = {e1 > 0 ? e1 - 1 : 0, e1 < nC[t1] - 1 ? e1 : nC[t1] - 1};        // m1, p1
    const i64 a2[2] = {e2 > 0 ? e2 - 1 : 0, e2 < nC[t2] - 1 ? e2 : nC[t2] - 1};        // m2, p2
    V acc = V();
#pragma unroll
    for (int q2 = 0; q2 < 2; ++q2)
#pragma unroll
        for (int q1 = 0; q1 < 2; ++q1) {          // (m1, m2), (p1, m2), (m1, p2), (p1, p2)
            i64 j[3];
            j[c] = e[c]; j[t1] = a1[q1]; j[t2] = a2[q2];
            acc += w(j[0], j[1], j[2]) / 4.0;
        }
    return acc;
}

// Edge `idx` of [fx|fy|fz] in the reference numbering (x fastest inside a component): component and (i0, i1, i2).
__device__ __forceinline__ int edge_of(i64 idx, const i64 nC[3], i64 e[3]) {
    const i64 nx = nC[0] * (nC[1] + 1) * (nC[2] + 1), ny = (nC[0] + 1) * nC[1] * (nC[2] + 1);
    const int c = idx < nx ? 0 : (idx < nx + ny ? 1 : 2);
    const i64 lin = idx - (c == 0 ? 0 : (c == 1 ? nx : nx + ny));
    const i64 d0 = (c == 0) ? nC[0] : nC[0] + 1, d1 = (c == 1) ? nC[1] : nC[1] + 1, d2 = (c == 2) ? nC[2] : nC[2] + 1;
    unlin3(lin, d0, d1, d2, e[0], e[1], e[2]);
    return c;
}

// maps.cellaverages2edges: out_c[edge] += sum over the statements of edges2cellaverages that read this edge of vol * v_c / 4 --
// the exact transpose of k_edges2cell (boundary multiplicities included).  v[c] == nullptr: that component is left alone.
template <class T>
struct C2EArgs {
    i64 nC[3];
    FieldLayout fl;
    const T* v[3];           // F-ordered (nx, ny, nz) cell arrays
    const double* vol;
    T* out;                  // [fx|fy|fz] (+=)
};

template <class T>
__global__ void k_cells2edges(C2EArgs<T> a, i64 nE) {
    const i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nE) return;
    i64 e[3];
    const int c = edge_of(idx, a.nC, e);
    const T* v = a.v[c];
    if (!v) return;
    const double* vol = a.vol;
    const i64 n0 = a.nC[0], n01 = a.nC[0] * a.nC[1];
    const i64 o = a.fl.off[c] + e[0] * a.fl.st[c][0] + e[1] * a.fl.st[c][1] + e[2] * a.fl.st[c][2];
    a.out[o] += c2e_gather<T>(c, e, a.nC, [&](i64 j0, i64 j1, i64 j2) {
        const i64 q = j0 + j1 * n0 + j2 * n01;
        return vol[q] * v[q];
    });
}

__device__ __forceinline__ double jvec_prod(double cv, double e, double sr, double) { return (sr * cv) * e; }
__device__ __forceinline__ c128 jvec_prod(double cv, c128 e, double sr, double si) { return mk(sr * cv, si * cv) * e; }

// Right-hand side of the J v solve: s[edge] = s mu_0 * C(v)[edge] * E[edge], C(v) = 1/4 sum of V_c v_c over the four cells around
// the edge with that component's perturbation (v[c] == nullptr: none, the component's source is zero); PEC boundary edges are written
// as exact zeros.  V = (hx*hy)*hz as in k_gradient.  Per edge 16 B of E are read and 16 B written (c128); the cell reads hit the cache.
// jvec_edge: the part that does not depend on the field -- the edge's offset `o` in a field array and C(v)[edge]; false: the edge's
// source is zero (PEC boundary, or no perturbation of its component).  One body for k_jvec_source and k_jvec_source_b, so that both
// round (and contract) alike.
__device__ __forceinline__ bool jvec_edge(i64 idx, const i64 nC[3], const FieldLayout& fl, const double* v0, const double* v1,
                                          const double* v2, const double* h0, const double* h1, const double* h2, i64& o, double& cv) {
    i64 e[3];
    const int c = edge_of(idx, nC, e);
    const int t1 = (c == 0) ? 1 : 0, t2 = (c == 2) ? 1 : 2;
    o = fl.off[c] + e[0] * fl.st[c][0] + e[1] * fl.st[c][1] + e[2] * fl.st[c][2];
    const double* v = c == 0 ? v0 : (c == 1 ? v1 : v2);
    cv = 0.0;
    if (!(v && e[t1] > 0 && e[t1] < nC[t1] && e[t2] > 0 && e[t2] < nC[t2])) return false;
    const i64 n0 = nC[0], n1 = nC[1];
    cv = c2e_gather<double>(c, e, nC, [&](i64 j0, i64 j1, i64 j2) {
        return ((h0[j0] * h1[j1]) * h2[j2]) * v[j0 + n0 * (j1 + n1 * j2)];
    });
    return true;
}

template <class T>
__global__ void k_jvec_source(i64 n0, i64 n1, i64 n2, FieldLayout fl, const T* efield, double sr, double si, const double* v0,
                              const double* v1, const double* v2, const double* h0, const double* h1, const double* h2, T* s, i64 nE) {
    const i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nE) return;
    const i64 nC[3] = {n0, n1, n2};
    i64 o;
    double cv;
    T val = Zero<T>::v();
    if (jvec_edge(idx, nC, fl, v0, v1, v2, h0, h1, h2, o, cv)) val = jvec_prod(cv, efield[o], sr, si);
    s[o] = val;
}

// The same for the systems of a batch that share ONE perturbation but have a forward field each (optimize.SurveyJacobian.jvec):
// the thread forms C(v)[edge] once, then s_b[edge] = s mu_0 C(v)[edge] E_b[edge] for the systems b = 0 .. nsys-1 whose bit is set in
// `use`, E_b = slice b of the batched vector `efield`, s_b = slice b of the level-0 source array; the other systems' slices are not
// touched.  Slice b is bit for bit what k_jvec_source writes for system b.  Per edge and active system sizeof(T) bytes are read and
// sizeof(T) written, consecutive threads consecutive edges (x fastest); the loads of up to JVEC_GROUP active systems are issued
// together, before the first product.
#define JVEC_GROUP 4
template <class T>
__global__ void k_jvec_source_b(i64 n0, i64 n1, i64 n2, FieldLayout fl, const T* efield, int nsys, unsigned long long use, double sr,
                                double si, const double* v0, const double* v1, const double* v2, const double* h0, const double* h1,
                                const double* h2, T* s, i64 nE) {
    const i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nE) return;
    const i64 nC[3] = {n0, n1, n2};
    i64 o;
    double cv;
    const bool live = jvec_edge(idx, nC, fl, v0, v1, v2, h0, h1, h2, o, cv);
    if (nsys < 64) use &= (1ull << nsys) - 1ull;
    if (!live) {
        for (int b = 0; b < nsys && b < 64; ++b)      // (never a shift by 64: nsys = 64 with bit 63 set is a valid batch)
            if ((use >> b) & 1ull) s[(i64)b * nE + o] = Zero<T>::v();
        return;
    }
    while (use) {                       // (wave-uniform: `use` is a kernel argument)
        int bs[JVEC_GROUP];
        T ev[JVEC_GROUP];
        int k = 0;
#pragma unroll
        for (int q = 0; q < JVEC_GROUP; ++q) {
            bs[q] = -1;
            if (use) {
                bs[q] = __builtin_ctzll(use);
                use &= use - 1ull;
                ev[q] = efield[(i64)bs[q] * nE + o];
                ++k;
            }
        }
#pragma unroll
        for (int q = 0; q < JVEC_GROUP; ++q)
            if (q < k) s[(i64)bs[q] * nE + o] = jvec_prod(cv, ev[q], sr, si);
    }
}
