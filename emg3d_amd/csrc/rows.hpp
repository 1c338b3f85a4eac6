// Device-resident row store (csrc/rows.hip): rows of J parked in HBM, and the dense products a data-space method takes from them.
// This header is what the two translation units share: the geometry of the Gram launch (host arithmetic, also exported as
// emg3d_rows_gram_plan / emg3d_rows_gram_job / emg3d_rows_gram_batch) and the entries the multigrid handle calls (emg3d_mg_sens_rows_park:
// rows_park; emg3d_mg_sens_rows_fill: rows_fill_check, rows_fill).
#pragma once
#include "common.hpp"

struct emg3d_rows;      // the C ABI's emg3d_rows_t

// ---- geometry of k_rows_gram --------------------------------------------------------------------------------------------
// The store is cut into row blocks of ROWS_BLOCK rows (8 tiles of 16) and into K-slabs of `slab` columns.  A workgroup owns one
// slab and one JOB = one pair of row blocks (ba >= bb): job = ba (ba + 1) / 2 + bb.  A diagonal job (ba == bb) accumulates the 36
// tile pairs ta >= tb of its block, an off-diagonal job all 64; both deal them to the 8 waves as t = wave + 8 i, so that a wave
// holds at most 8 accumulators of 4 f64 per lane (64 VGPRs) -- a 256 x 256 off-diagonal pair of panels would need the whole
// register file of a compute unit.  The slab length is a function of n_cols ALONE (never of n_rows, the device or a row's
// position): the summation order of every element of G follows from n_cols.
constexpr int ROWS_BLOCK = 128;         // rows per block
constexpr int ROWS_TILE = 16;           // MFMA tile edge
constexpr int ROWS_KSTEP = 16;          // columns staged per step (4 MFMA k-steps of 4)
constexpr int ROWS_LD = 145;            // LDS row length of a staged [k][row] tile, doubles: 145 = 17 mod 32, so that the four k of an
                                        // operand read (16 rows each) fall on disjoint banks but one, and the 16 k of a staging write
                                        // (one row each) on 16 different ones
constexpr int ROWS_WAVES = 8;
constexpr i64 ROWS_SLAB_MIN = 2048;     // columns
constexpr i64 ROWS_SLABS_MAX = 256;     // at most this many slabs: slab = max(ROWS_SLAB_MIN, ceil(n_cols / 256) rounded up to 16)

struct RowsGramPlan {
    i64 slab = 0, nslab = 0, nblk = 0, njobs = 0, lds_bytes = 0;
};
inline i64 rows_slab_len(i64 n_cols) {
    const i64 per = (n_cols + ROWS_SLABS_MAX - 1) / ROWS_SLABS_MAX;
    const i64 s = (per + ROWS_KSTEP - 1) / ROWS_KSTEP * ROWS_KSTEP;
    return s > ROWS_SLAB_MIN ? s : ROWS_SLAB_MIN;
}
inline RowsGramPlan rows_gram_plan(i64 n_rows, i64 n_cols) {
    RowsGramPlan p;
    p.slab = rows_slab_len(n_cols);
    p.nslab = (n_cols + p.slab - 1) / p.slab;
    p.nblk = (n_rows + ROWS_BLOCK - 1) / ROWS_BLOCK;
    p.njobs = p.nblk * (p.nblk + 1) / 2;
    p.lds_bytes = 2 * (i64)ROWS_KSTEP * ROWS_LD * (i64)sizeof(double);
    return p;
}
// The jobs run in LAUNCHES of as many as fit ROWS_GRAM_SCRATCH bytes of slab partials (at least one): launch l holds the jobs
// l * batch .. min(njobs, (l + 1) * batch) - 1, one k_rows_gram and one k_rows_gram_reduce each.  A job's partials are its 64 tile
// pairs of 256 doubles per slab, so that `batch` depends on n_rows through njobs only.  What emg3d_rows_gram runs and what
// emg3d_rows_gram_batch reports.
constexpr i64 ROWS_GRAM_SCRATCH = (i64)256 << 20;       // bytes of slab partials held at a time
struct RowsGramBatch {
    i64 per_job = 0, batch = 0, launches = 0;           // bytes of one job's partials, jobs per launch, launches
};
inline RowsGramBatch rows_gram_batch(i64 n_rows, i64 n_cols) {
    const RowsGramPlan p = rows_gram_plan(n_rows, n_cols);
    RowsGramBatch b;
    b.per_job = 64 * p.nslab * 256 * (i64)sizeof(double);
    const i64 fit = ROWS_GRAM_SCRATCH / b.per_job > 1 ? ROWS_GRAM_SCRATCH / b.per_job : 1;
    b.batch = p.njobs < fit ? p.njobs : fit;
    b.launches = (p.njobs + b.batch - 1) / b.batch;
    return b;
}
// job -> its pair of row blocks
HD void rows_job_blocks(i64 job, i64& ba, i64& bb) {
    ba = 0;
    while ((ba + 1) * (ba + 2) / 2 <= job) ++ba;
    bb = job - ba * (ba + 1) / 2;
}
// tile pair number t of a job -> its tiles (ta: rows of G, tb: columns of G); false: the job has no such pair
HD bool rows_job_tile(bool diag, int t, int& ta, int& tb) {
    if (!diag) { ta = t >> 3; tb = t & 7; return t < 64; }
    ta = 0;
    while ((ta + 1) * (ta + 2) / 2 <= t) ++ta;
    tb = t - ta * (ta + 1) / 2;
    return t < 36;
}

// ---- geometry of k_rows_project (Y = M R) ---------------------------------------------------------------------------------
// The result is cut into PANELS of PROJ_COLS columns and into BLOCKS of PROJ_BLOCK output rows; a workgroup (4 waves) owns one
// panel of one block and walks all n_rows of the source in steps of PROJ_KSTEP, its accumulators in registers: wave w holds the
// row tiles (w & 1) NT .. + NT - 1 and the column tiles 2 (w >> 1), + 1 of its 32 NT x 64 piece, NT = 8 for a full block -- 16
// accumulators of 4 f64 per lane, half the registers of a lane at two workgroups per compute unit.  A block with at most 128,
// 64 or 32 live output rows -- the last or only one -- runs the instantiation NT = 4, 2 or 1, which stages and multiplies those
// rows only.  Every block is one pass over the source: 256 output rows (the rows of a store against themselves: K^-1 R) read it
// once.  The panels are a function of n_cols ALONE, and an element's accumulation chain of neither: see emg3d_rows_project.
constexpr int PROJ_BLOCK = 256;         // output rows per block
constexpr int PROJ_COLS = 64;           // columns per workgroup
constexpr int PROJ_KSTEP = 16;          // source rows staged per step (4 MFMA k-steps of 4)
constexpr int PROJ_THREADS = 256;
constexpr int PROJ_PAD = 16;            // LDS row lengths are 64 + 16 (the slice of R) and 32 NT + 16 (the slice of M) doubles, all
                                        // = 16 mod 32: the two k of a 32-lane half of an operand read (16 doubles each) fall on the
                                        // two halves of the 32 eight-byte bank slots, and a staging write is 64 doubles in a row

struct RowsProjectPlan {
    i64 passes = 0, panels = 0, wg = 0, ksteps = 0, last_rows = 0, lds_bytes = 0;
};
// rows that the instantiation for a block of `live` output rows covers
inline i64 rows_project_cover(i64 live) { return live <= 32 ? 32 : live <= 64 ? 64 : live <= 128 ? 128 : PROJ_BLOCK; }
inline i64 rows_project_lds(i64 cover) { return (i64)PROJ_KSTEP * ((cover + PROJ_PAD) + (PROJ_COLS + PROJ_PAD)) * (i64)sizeof(double); }
inline RowsProjectPlan rows_project_plan(i64 n_rows, i64 m, i64 n_cols) {
    RowsProjectPlan p;
    p.passes = (m + PROJ_BLOCK - 1) / PROJ_BLOCK;
    p.panels = (n_cols + PROJ_COLS - 1) / PROJ_COLS;
    p.wg = p.passes * p.panels;
    p.ksteps = (n_rows + PROJ_KSTEP - 1) / PROJ_KSTEP;
    p.last_rows = rows_project_cover(m - (p.passes - 1) * PROJ_BLOCK);
    p.lds_bytes = rows_project_lds(p.passes > 1 ? PROJ_BLOCK : p.last_rows);
    return p;
}

// Store row dest[p] <- plane part = 0 of pair p of `src` = [pairs][ndir][npart][ncells] doubles (device; the layout of k_sens_rows and
// of its model-grid image), on `stream`; dest[p] < 0 skips the pair.  chain != 0: direction q times the store's chain factor q
// (emg3d_rows_set_chain); sum3 != 0: one plane (p0 + p1) + p2 of the (scaled) directions.  -2: a store of another size than
// (sum3 ? 1 : ndir) * ncells columns, a dest[p] >= n_rows, sum3 without three directions, chain without factors of ncells
// entries, another device.  The caller synchronises `stream` before it returns (dest is read asynchronously).
int rows_park(emg3d_rows* rows, hipStream_t stream, int device, const double* src, i64 pairs, int ndir, int npart, i64 ncells,
              const int32_t* dest, int chain, int sum3);

// ---- both parts of the rows of a chunk, filled by the sensitivity kernel itself (emg3d_mg_sens_rows_fill) ---------------------------
// What a fill of `pairs` pairs of ndir directions, npart parts and ncells cells may ask of the store: the checks of rows_park for
// both tables, and -2 too for a dest_im with one part (a real handle), a row named twice (in one table or across the two) and a
// call in which every entry is negative.  0: the fill may run.  No device call.
int rows_fill_check(const emg3d_rows* rows, int device, i64 pairs, int ndir, int npart, i64 ncells, const int32_t* dest_re,
                    const int32_t* dest_im, int chain, int sum3);
// The cells and fields of a level-0 launch of the per-cell kernels (csrc/gradient.hpp), as MG_CELL_LAUNCH passes them.
template <class T>
struct RowsFillFields {
    i64 nC[3];
    FieldLayout fl;
    const T* fwd;           // batched vector of forward fields, [system][nE]
    const T* adj;           // level-0 field array, [system][nE]
    i64 nE;
    int nsys;
    unsigned long long use_fwd, use_adj;
    double sr, si;
    const double* h[3];
};
// ONE launch of k_sens_rows_fill<T, split> on `stream` into the store: the real part of pair p into row dest_re[p], the imaginary
// part into row dest_im[p] (nullptr: none), with the store's chain factors and sum3 as rows_park applies them.  The kernel lives in
// this unit so that the store's pointer, row length, chain factors and destination tables never leave it.  Runs rows_fill_check
// first (its -2, nothing launched); the caller synchronises `stream` before it returns.  T = double, c128.
template <class T>
int rows_fill(emg3d_rows* rows, hipStream_t stream, int device, const RowsFillFields<T>& f, int split, const int32_t* dest_re,
              const int32_t* dest_im, int chain, int sum3);
