// Which line-sweep kernel serves a (level, direction): ONE function of the selection knobs, the device's size and the level's shape.
//
// Host-only (no HIP header, no device memory, no launch): the cycle driver (mg.hpp) builds factors, working copies and launches from
// the SweepPlan this file computes, emg3d_sweep_plan (emg3d_hip.hip) exports the same value, and the kernel's name -- as
// `rocprofv3 --kernel-trace` and emg3d_mg_last_sweep_kernel show it -- is formatted here and nowhere else.
// (Reference: the one loop of core.gauss_seidel_x/_y/_z, emg3d/core.py:477-1316, has no such choice.)
//
//   k_line_sweep_qpl (scan along the line, smooth_qpl.hpp)  wherever the dependent chain of the lane-group
//       kernels would leave SIMDs idle: lines of <= qpl_max_nl (64) blocks; lines of any length <= 256
//       blocks when a colour has <= qpl_few_lines (1024) lines; every launch of the lexicographic order
//       (a hyperplane holds at most min(nP, nQ)/2 lines: 128-block lines 20 instead of 96 us per launch);
//   k_line_sweep_tha (the two-sided solve in affine form, helper waves, smooth_tha.hpp)   the mid levels (sweep_tha_helpers);
//   k_line_sweep_thm (two-sided chain on the mirrored factorisation, halves of 8 lines in a pair of waves, smooth_thm.hpp)
//                                                             colours of < 8192 longer lines (128^3 level 0);
//   k_line_sweep_qc  (quad per line, compact factor, smooth_qc.hpp)   colours of >= 8192 lines (256^3 levels 0, 1);
//   k_line_sweep_rp  (one-sided chain, lane per row)         where neither applies (factor beyond 4 GiB, EMG3D_TWIST=0);
//   k_line_sweep_qc<..., BIG> (the same with 64-bit field offsets)      levels whose field arrays reach 4 GiB (sweep_q_big);
//   k_line_sweep     (thread per line, 64-bit offsets)       such levels in the lexicographic order or with fewer lines, EMG3D_SWEEP=tpl.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

typedef int64_t i64;

// (common.hpp's macros, for a translation unit that includes this file alone: knobs exist only in the lab build, -DEMG3D_LAB)
#ifndef LAB_ENV
#ifdef EMG3D_LAB
inline long long lab_env_(const char* name, long long def) { const char* v = getenv(name); return v ? atoll(v) : def; }
inline int lab_env_ch_(const char* name) { const char* v = getenv(name); return v ? v[0] : 0; }
#define LAB_ENV(name, def) lab_env_(name, (long long)(def))
#define LAB_ENV_CH(name) lab_env_ch_(name)
#else
#define LAB_ENV(name, def) ((long long)(def))
#define LAB_ENV_CH(name) 0
#endif
#endif

// k_line_sweep_tha's launch shape and LDS need (smooth_tha.hpp: THA_LPW, tha_ring_depth, THA_MAX_DYN_LDS, THA_STATIC_LDS,
// tha_lds_bytes<T, 3>; mg.hpp asserts that the constants agree)
constexpr int SWEEP_THA_LPW = 8, SWEEP_THA_RING = 8, SWEEP_THA_MAX_DYN_LDS = 140 * 1024, SWEEP_THA_STATIC_LDS = 18 * 1024;
inline i64 sweep_tha_lds_bytes(i64 nL, int tsize) {
    return (2 * SWEEP_THA_RING * 5 + 2 * ((nL + 1) / 2 + 2)) * (5 * SWEEP_THA_LPW) * (i64)tsize;
}

// ---- the knobs and the device's size, filled once per handle ------------------------------------------------------------------
// The product library runs the measured defaults (why each is what it is: DESIGN.md 3; the A/B numbers behind them:
// profiles/HISTORY.md) and reads, of the selection, EMG3D_BATCH_TUNE alone.  The lab build (-DEMG3D_LAB: libemg3d_hip_lab.so, used by
// tests/test_gpu_variants.py and tools/) also compiles the superseded kernels and reads one variable per knob below (LAB_ENV).
//
// Launch-shape thresholds are in units of the DEVICE (256 CUs = 1024 SIMDs on MI355X; the literals of rounds 2-5 in brackets).
// A colour launch of the chain kernels is made of waves that all last the same time: W waves on S SIMDs take ceil(W / S) rounds
// (HISTORY R5.19), so every "how many lines" threshold is a number of waves per SIMD:
//   q_min_lines      8 S  [8192]  lines per colour from which the quad kernel serves: one wave per SIMD at 8 lines per wave
//   qpl_few_lines      S  [1024]  up to here the scan kernel serves lines of any length: one single-line wave per SIMD
//   tha_min_lines  1.07 S [1100]  measured crossover of the affine kernel against the scan kernel on 33..64-block lines
//   tha_big_lines   8 CUs [2048]  65..128-block lines in the affine kernel: one workgroup of 8 lines per CU, ONE round
//   qdesc_max      8.8 S  [9000]  threads of a colour launch up to which the descriptor table is cheaper than the arithmetic
constexpr i64 SCANTAB_THREADS = 40000;     // (sweep_scantab below)
struct SweepKnobs {
    // the device and the handle
    i64 simds = 1024;                   // 4 per CU
    i64 lds_limit = 160 * 1024;         // LDS bytes per workgroup
    bool tha_lds_granted = true;        // k_line_sweep_tha's dynamic LDS (up to 135 680 B, + SWEEP_THA_STATIC_LDS static) was asked for and
                                        // granted; a device or runtime that refuses it gets the other kernels (sweep_tha_helpers -> 0)
    bool thm_lds_granted = true;        // the same for k_line_sweep_thm's kept z (sweep_thm_zkeep below): refused, every step parks in e
    int order = 1, nsys = 1;            // 1: four-colour order, 0: lexicographic; batched systems per launch
    // EMG3D_BATCH_TUNE=1 (default 0): with batched systems, choose between the scan kernel and the chain kernels by the
    // lines a LAUNCH carries (lines x systems) instead of the lines of one system -- the scan kernel does 4 x the
    // arithmetic and only pays while the chain kernels leave SIMDs idle.  8 systems at 128^3: 50.3 -> 46.4 ms per cycle.
    // Off by default because the kernel choice then depends on the batch size: a system's result agrees with its
    // stand-alone solve to rounding (1e-12) instead of bit for bit.
    int batch_tune = getenv("EMG3D_BATCH_TUNE") ? atoi(getenv("EMG3D_BATCH_TUNE")) : 0;

    int sweep_kernel = LAB_ENV_CH("EMG3D_SWEEP") == 't' ? 1 : 0;       // 1: thread-per-line kernel everywhere
    // dir 0 (x-lines) runs on x<->y transposed working copies, on levels of at least xt_min_cells cells (small levels: the 6-9
    // transposition launches cost more than strided access)
    bool use_xt = LAB_ENV("EMG3D_XT", 1) != 0;
    i64 xt_min_cells = LAB_ENV("EMG3D_XT_MIN", 8192);
    int th_lpw = (int)LAB_ENV("EMG3D_TH_LPW", 0);                       // k_line_sweep_thm: lines per pair of waves 4|8|12 (0: by launch size)
    int force_lpw = (int)LAB_ENV("EMG3D_LPW", 0);                       // k_line_sweep_rp: lines per wave 4|8|12 (0: by size)
    bool use_twist = LAB_ENV("EMG3D_TWIST", 1) != 0;                    // two-sided factorisation below twist_max_lines
    i64 twist_max_lines_env = LAB_ENV("EMG3D_TWIST_MAX", 0);            // 0: q_min_lines()
    int tw_stages = (int)LAB_ENV("EMG3D_TW_STAGES", 0);                 // register prefetch depth of the two-sided kernels (0: 3)
    // k_line_sweep_thm: forward steps of a half whose z stays in LDS (sweep_thm_zkeep): -1 as many as fit, 0 none, n at most n
    i64 thm_zkeep = LAB_ENV("EMG3D_THM_ZKEEP", -1);
    // (retired: the 19-numbers-per-row LIFO the z keep replaced.  The name is still read, and ignored, so that lab scripts and test
    // cases that set it run the default path)
    int thm_lifo_retired = (int)LAB_ENV("EMG3D_THM_LIFO", 0);
    // sweeps on parity-split working copies (the lines of one colour contiguous in memory): 0 never, 1 every level and
    // ordering, 2 (default) colour-ordered levels of >= split_min_cells
    int use_split = (int)LAB_ENV("EMG3D_SPLIT", 2);
    i64 split_min_cells = LAB_ENV("EMG3D_SPLIT_MIN_CELLS", 2000000);
    // quad-per-line chain kernel (smooth_qc.hpp): 1 (default) on launches of >= q_min_lines lines per colour (bandwidth
    // bound: 256^3 level 0), 2 wherever a lane-group kernel would serve, 0 never
    int use_q = (int)LAB_ENV("EMG3D_Q", 1);
    i64 q_min_lines_env = LAB_ENV("EMG3D_Q_MIN_LINES", 0);              // 0: 8 lines per wave on every SIMD
    // register prefetch depth of k_line_sweep_qc: 0 = by the launch -- 2 stages at 16 lines per wave and at most one wave per SIMD (210 registers; the 3-stage
    // instantiation there is 322 registers with 84 / 310 AGPR writes / reads in its loop bodies, i.e. prefetched values that are
    // waited for when they are parked), 3 stages below (level 1 of a 256^3 cycle: 8 lines per wave); lab: 2 | 3 force one.
    // 256^3, same box, alternating (profiles/r05_qstages_ab.txt): launch 731 -> 713 us dense, 650 -> 637 dipole, V-cycle 30.88 -> 30.57 ms;
    // 2 stages everywhere: the launch the same, the cycle +0.15 ms (level 1).
    int q_stages = (int)LAB_ENV("EMG3D_Q_STAGES", 0);
    int q_lpw = (int)LAB_ENV("EMG3D_Q_LPW", 0);                         // lines per wave 16|8|4|2 (0: by launch size)
    int q_big_lab = (int)LAB_ENV("EMG3D_Q_BIG", 0);                     // 1: the 64-bit variant on levels that would fit 32 bits (parity tests at small sizes)
    // quad-per-block scan kernel (smooth_qpl.hpp): direction mask; lines of qpl_min_nl .. qpl_max_nl blocks (any length
    // <= 256 when a colour has <= qpl_few_lines lines, and in lexicographic order); two blocks per quad from qpl_m2_min on
    int use_qpl = (int)LAB_ENV("EMG3D_QPL", 7);
    i64 qpl_min_nl = LAB_ENV("EMG3D_QPL_MIN", 2);
    i64 qpl_max_nl = LAB_ENV("EMG3D_QPL_MAX_NL", 64);
    // (32 since round 4: with the launch prologues trimmed, the 32-block levels of a 128^3 F-cycle -- ~1000 lines per colour -- do
    // better with one wave per SIMD and two blocks per quad than with two waves per SIMD: cycle 8.75 / 8.72 -> 8.63 / 8.65 ms;
    // from 16 blocks on: 8.78 / 8.76; profiles/r04_qpl_m2_ab.txt)
    i64 qpl_m2_min = LAB_ENV("EMG3D_QPL_M2", 32);
    // chain form of the scan kernel (smooth_qpl.hpp CH) on lines of at most this many quads (0: never).  4-block lines: the 168 such
    // launches of a 128^3 F-cycle 5.27 -> 4.86 us (three DPP-fed steps against two Kogge-Stone steps through LDS); 8-block lines
    // (seven steps, lane shuffles across the row boundary) 5.78 -> 6.16 us: 4 (HISTORY R6.3, profiles/r06_qpl_chain_ab.txt)
    int qpl_chain_seg = (int)LAB_ENV("EMG3D_QPL_CHAIN", 4);
    i64 qpl_few_lines_env = LAB_ENV("EMG3D_QPL_FEW", 0);                // 0: one single-line wave per SIMD
    i64 qpl_max_lines = LAB_ENV("EMG3D_QPL_MAX", (i64)1 << 40);
    // Descriptors of the scan kernel's colour launches on levels of short lines (MG::ensure_qdesc, HISTORY R5.12): 176 B per thread,
    // only where a colour launch has at most qdesc_max_threads threads and the factor has fewer than 2^32 entries.  Measured
    // (profiles/r05_qdesc_ab.txt, 128^3 F-cycle, three alternating repetitions): off 8.57 / 8.54 / 8.50 ms; launches of <= 9000 threads
    // (308 of the 420 on <= 16-block lines) 8.456 / 8.458 / 8.451; <= 40 000 threads (all 420) 8.495 / 8.468 / 8.48; the 32-block level
    // too (two blocks per quad, 65 k threads) 8.72: beyond ~8 k threads the table costs more to read than the arithmetic it replaces.
    // In-kernel stamps at 128 x 4 x 4: 8330 -> 7500 cycles.
    int use_qdesc = (int)LAB_ENV("EMG3D_QDESC", 1);
    i64 qdesc_max_threads_env = LAB_ENV("EMG3D_QDESC_MAX", 0);
    // Scan tables of the scan kernel's colour launches (MG::ensure_scantab, smooth_qpl.hpp SM; the rule: sweep_scantab below):
    // -1 by the rule, 0 never, 1 wherever the kernel form allows it whatever the launch's size (lab); threads of a colour launch up to
    // which a table is admitted (0: scantab_max_threads()); bytes the four colours' tables of a (level, direction) may take
    int use_scantab = (int)LAB_ENV("EMG3D_QPL_SCANTAB", -1);
    i64 scantab_max_threads_env = LAB_ENV("EMG3D_QPL_SCANTAB_MAX", 0);
    i64 scantab_max_bytes = LAB_ENV("EMG3D_QPL_SCANTAB_BYTES", (i64)64 << 20);
    // Fused colour passes of a smoothing call on the levels of short lines (plan_fuse below): lines of at most fuse_max_seg quads (0:
    // never); own lines per slab (0: 2); bytes of private copies a
    // (level, direction) may take
    int fuse_max_seg = (int)LAB_ENV("EMG3D_QPL_FUSE", 4);
    i64 fuse_own = LAB_ENV("EMG3D_QPL_FUSE_W", 0);
    i64 fuse_max_bytes = LAB_ENV("EMG3D_QPL_FUSE_BYTES", (i64)64 << 20);
    // k_line_sweep_tha on the mid levels the scan kernel served: colour order, no split copies, lines of tha_min_nl .. tha_mid_nl
    // (33..64) blocks, at least tha_min_lines lines per colour.  Measured per launch (profiles/r04_rs_shapes.txt, r04_tha_ab.txt):
    // the launch is as long as its chain wave's work (~7 us + 0.6 us per step: 25 us at 64 blocks, 19 us at 40) whatever the
    // number of lines up to 2048 (one workgroup per CU at 8 lines each); the scan kernel grows with the lines (64-block lines:
    // 16 / 22 / 41 us at 512 / 1024 / 2048 lines per colour) and wins below ~1100; lines of <= 32 blocks stay with the scan kernel.
    // Batched handles take the same kernel: the choice must not depend on the batch size (a system stays bit for bit its own solve).
    int use_tha = (int)LAB_ENV("EMG3D_THA", 3);     // helper waves per half: 3 (lab: 2; 0: off, the scan kernel serves)
    i64 tha_min_nl = LAB_ENV("EMG3D_THA_MIN", 33), tha_mid_nl = LAB_ENV("EMG3D_THA_MID", 64), tha_min_lines_env = LAB_ENV("EMG3D_THA_MIN_LINES", 0);
    // It also serves lines of 65..128 blocks (tha_max_nl) when a colour has at most 2048 lines (tha_big_max_lines), i.e. ONE round
    // of workgroups at one per CU (142 KB of LDS at 128 blocks): 128 x 128 x 64, x- / y-lines: 74 -> 53 us per launch against
    // k_line_sweep_thm, the grid's F-cycle 6.71 -> 6.25 ms (profiles/r04_tha_long_lines.txt).  Level 0 of 128^3 (4032 lines per
    // colour = two rounds, each as long as its helper-bound forward pass) loses 103-105 to 86 us and keeps k_line_sweep_thm<8, ZS>
    // (lab: EMG3D_THA_BIG_LINES=8192; HISTORY R4.8).
    i64 tha_max_nl = LAB_ENV("EMG3D_THA_MAX", 128);
    i64 tha_big_max_lines_env = LAB_ENV("EMG3D_THA_BIG_LINES", 0);
    int tha_split = (int)LAB_ENV("EMG3D_THA_SPLIT", 0);     // lab: also on mid levels that have split copies (EMG3D_SPLIT_MIN_CELLS)

    i64 q_min_lines() const { return q_min_lines_env > 0 ? q_min_lines_env : 8 * simds; }
    i64 twist_max_lines() const { return twist_max_lines_env > 0 ? twist_max_lines_env : q_min_lines(); }
    i64 qpl_few_lines() const { return qpl_few_lines_env > 0 ? qpl_few_lines_env : simds; }
    i64 qdesc_max_threads() const { return qdesc_max_threads_env > 0 ? qdesc_max_threads_env : (9000 * simds + 1023) / 1024; }
    i64 scantab_max_threads() const { return scantab_max_threads_env > 0 ? scantab_max_threads_env : (SCANTAB_THREADS * simds + 1023) / 1024; }
    i64 tha_min_lines() const { return tha_min_lines_env > 0 ? tha_min_lines_env : (1100 * simds + 1023) / 1024; }
    i64 tha_big_max_lines() const { return tha_big_max_lines_env > 0 ? tha_big_max_lines_env : (i64)SWEEP_THA_LPW * (simds / 4); }
};

// ---- the level's shape: nC and the scalar's size; everything else the selection reads follows (MG::shape_level) --------------------
struct SweepShape {
    i64 nC[3];
    int tsize;          // sizeof(T): 8 float64, 16 complex128
    i64 cells() const { return nC[0] * nC[1] * nC[2]; }
    i64 edges() const {
        return nC[0] * (nC[1] + 1) * (nC[2] + 1) + (nC[0] + 1) * nC[1] * (nC[2] + 1) + (nC[0] + 1) * (nC[1] + 1) * nC[2];
    }
    // lines along dir: transverse axes P, Q as in MG::line_args; of the largest colour / of all four
    i64 lines(int dir) const { return (nC[dir == 0 ? 1 : 0] / 2) * (nC[dir == 2 ? 1 : 2] / 2); }
    i64 lines_tot(int dir) const { return (nC[dir == 0 ? 1 : 0] - 1) * (nC[dir == 2 ? 1 : 2] - 1); }
    // stride of field component c / of the cell arrays along axis ax, reference layout (x fastest) or x<->y transposed (y fastest)
    i64 field_stride(int c, int ax, bool transposed) const {
        const i64 d0 = (c == 0) ? nC[0] : nC[0] + 1, d1 = (c == 1) ? nC[1] : nC[1] + 1;
        return ax == 2 ? d0 * d1 : ((ax == 0) != transposed) ? 1 : (transposed ? d1 : d0);
    }
    i64 cell_stride(int ax, bool transposed) const {
        return ax == 2 ? nC[0] * nC[1] : ((ax == 0) != transposed) ? 1 : (transposed ? nC[1] : nC[0]);
    }
};

enum class SweepFamily { tpl, rp, qc, qc_big, thm, tha, qpl, qpl_chain };

// The name of an instantiation: p1, p2 = (stages, lines per wave) qc / qc_big / thm; (helpers) tha; (waves per workgroup, blocks per
// quad) qpl / qpl_chain; (lines per wave) rp.
inline void sweep_kernel_name(char* out, size_t len, SweepFamily f, int tsize, int p1 = 0, int p2 = 0) {
    static const char* const base[] = {"k_line_sweep", "k_line_sweep_rp", "k_line_sweep_qc", "k_line_sweep_qc_big", "k_line_sweep_thm",
                                       "k_line_sweep_tha", "k_line_sweep_qpl", "k_line_sweep_qpl_chain"};
    const char* tn = tsize == 16 ? "c128" : "f64";
    if (f == SweepFamily::tpl) snprintf(out, len, "%s<%s>", base[(int)f], tn);
    else if (f == SweepFamily::rp || f == SweepFamily::tha) snprintf(out, len, "%s<%s,%d>", base[(int)f], tn, p1);
    else snprintf(out, len, "%s<%s,%d,%d>", base[(int)f], tn, p1, p2);
}

struct SweepPlan {
    SweepFamily family = SweepFamily::tpl;
    // instantiation: prefetch stages (qc, thm); lines per wave / per pair of waves of the instantiation (qc, rp, thm); sweep_tha_helpers()
    // of the level whatever serves it (LineArgs::tha); qpl: waves per workgroup NW, blocks per quad M, quads per line seg (0: not qpl)
    int stages = 0, inst_lpw = 0, helpers = 0, NW = 0, M = 0, seg = 0;
    int qlpw = 0;               // qc: lines per wave the largest colour's launch runs at (<= inst_lpw: sweep_balanced_lpw)
    bool big = false;           // 64-bit field offsets
    bool split = false;         // the level's sweeps run on parity-split working copies
    bool xt = false;            // no split copies, x-lines on the x<->y transposed copy
    int work_id = 0;            // the working copy: 0 / 1 split (x-lines / y- and z-lines), 2 transposed, 3 + dir the reference layout
    int fac_kind = 0;           // layout of the cached factor (Level::fac_kind): 0 one-sided, 15 numbers per block (scan kernel, rp,
                                // thread per line); 3 mirrored two-sided (thm, tha); 4 one-sided compact, 11 numbers per block (qc)
    i64 fac_entries = 0;        // factor entries per line
    i64 mid = 0;                // middle block of the two-sided factor (one-sided: the last block)
    bool qdesc = false;         // the colour launches of the scan kernel load per-lane descriptors (MG::ensure_qdesc)
    bool scantab = false;       // ... and the scanned map matrices of every step (MG::ensure_scantab; sweep_scantab)
    i64 scantab_bytes = 0;      // bytes of the four colours' tables (0: the kernel form has no table)
    i64 nmax = 0;               // lines of the largest colour
    i64 lpw = 0;                // lines per wave (thm: per pair of waves; tha, qpl: per workgroup; thread per line: 64)
    i64 rounds = 0;             // rounds of waves / workgroups of the largest colour's launch
    char name[64] = "";
};

// ---- predicates of a LEVEL ------------------------------------------------------------------------------------------------------
// The lane-group kernels address with a uniform base and 32-bit per-lane byte offsets: (i) the field arrays, (ii) a plane of
// the factor, (iii) zeta must each stay below 4 GiB.  wide_fits: (ii) and (iii) only.
inline bool sweep_wide_fits(const SweepKnobs& K, const SweepShape& G) {
    const i64 lim = (i64)1 << 32;
    const i64 mx = std::max(G.lines_tot(0), std::max(G.lines_tot(1), G.lines_tot(2)));
    return K.sweep_kernel == 0 && mx * 15 * (i64)G.tsize < lim && G.cells() * 8 < lim;
}
// Fields of 4 GiB and more (complex: from ~445^3 cells on; 512^3 = 6.4 GB per field): the quad-per-line kernel with 64-bit
// field offsets (k_line_sweep_qc<..., BIG>) serves, on the split working copies like every other large level, where all
// three line directions have the lines for it (>= q_min_lines() per colour, i.e. 8 per wave on every SIMD: the 16-line instantiation
// at the balanced number of lines per wave); everything else of the cycle
// (residual, transfers, conversions) is 64-bit throughout.  Other shapes keep the thread-per-line kernel.
inline bool sweep_q_big_lines(const SweepKnobs& K, const SweepShape& G) {
    for (int d = 0; d < 3; ++d) if (G.lines(d) < std::max<i64>(K.q_min_lines(), 1)) return false;
    return K.order == 1 && K.use_q >= 1;
}
inline bool sweep_q_big(const SweepKnobs& K, const SweepShape& G) {
    return sweep_wide_fits(K, G) && sweep_q_big_lines(K, G) && (K.q_big_lab || G.edges() * (i64)G.tsize >= ((i64)1 << 32));
}
// does the row-parallel family (32-bit offsets) apply to this level?
inline bool sweep_rp_fits(const SweepKnobs& K, const SweepShape& G) {
    return sweep_wide_fits(K, G) && G.edges() * (i64)G.tsize < ((i64)1 << 32) && !(K.q_big_lab && sweep_q_big_lines(K, G));
}
inline bool sweep_split_on(const SweepKnobs& K, const SweepShape& G) {
    return (K.use_split == 1 || (K.use_split == 2 && K.order == 1 && G.cells() >= K.split_min_cells)) &&
           (sweep_rp_fits(K, G) || sweep_q_big(K, G));
}

// ---- predicates of a (level, direction) -------------------------------------------------------------------------------------------
// helper waves per half of k_line_sweep_tha (0: another kernel serves)
inline int sweep_tha_helpers(const SweepKnobs& K, const SweepShape& G, int dir) {
    if ((K.use_tha != 3 && K.use_tha != 2) || K.order != 1 || K.sweep_kernel != 0 || !K.use_twist || !sweep_rp_fits(K, G)) return 0;
    const i64 nL = G.nC[dir], lds = sweep_tha_lds_bytes(nL, G.tsize);
    if (nL < K.tha_min_nl || nL > K.tha_max_nl) return 0;
    if (!K.tha_lds_granted || lds > SWEEP_THA_MAX_DYN_LDS || lds + SWEEP_THA_STATIC_LDS > K.lds_limit) return 0;
    const bool big = nL > K.tha_mid_nl;
    if (!big && sweep_split_on(K, G) && !K.tha_split) return 0;
    const i64 lines = G.lines(dir);
    if (lines < K.tha_min_lines() || lines >= K.q_min_lines()) return 0;
    if (big && lines > K.tha_big_max_lines()) return 0;                 // (more than one round of workgroups at one per CU)
    return K.use_tha;
}
inline bool sweep_qpl_on(const SweepKnobs& K, const SweepShape& G, int dir) {
    if (!((K.use_qpl >> dir) & 1) || sweep_split_on(K, G) || K.sweep_kernel != 0 || sweep_tha_helpers(K, G, dir)) return false;
    const i64 nL = G.nC[dir], cap = (nL >= K.qpl_m2_min) ? 256 : 128;     // 8 waves x 16 quads x M blocks per line
    i64 lines = G.lines(dir), max_nl = K.qpl_max_nl;
    if (K.batch_tune && K.nsys > 1 && K.order == 1) {                 // a launch carries nsys x the lines (see batch_tune)
        lines *= K.nsys;
        max_nl = std::max<i64>(4, K.qpl_max_nl / K.nsys);
    }
    const i64 maxnl = (K.order == 0 || lines <= K.qpl_few_lines()) ? cap : std::min<i64>(max_nl, cap);
    if (nL < K.qpl_min_nl || nL > maxnl || !sweep_rp_fits(K, G)) return false;
    return lines <= K.qpl_max_lines;
}
// Two-sided sweeps on the MIRRORED factorisation (k_line_sweep_thm: left blocks [l_i; T_i] upwards, right blocks
// [l_j; T_{j-1}] downwards: the reference's accuracy; round 1's plain two-sided grouping was 1e-8 on ill-conditioned lines) for
// latency-bound launches: fewer than 8192 lines per colour (beyond that the sweep is HBM bound and the quad-per-line kernel on the
// compact factor moves fewer bytes), strides within the 24-bit multiplies of the kernel.  q_on: the quad-per-line kernel serves
// (it has its own compact, one-sided factorisation); transposed: the layout the x-lines' factor is built on.
inline bool sweep_twist_ok(const SweepKnobs& K, const SweepShape& G, int dir, bool q_on, bool transposed) {
    if (q_on || !K.use_twist || !sweep_rp_fits(K, G) || G.nC[dir] < 3) return false;
    if (G.lines(dir) >= K.twist_max_lines()) return false;
    const i64 lim24 = (i64)1 << 24;
    i64 mxs = 15 * G.lines_tot(dir) * (i64)G.tsize;
    for (int c = 0; c < 3; ++c) mxs = std::max(mxs, G.field_stride(c, dir, transposed) * (i64)G.tsize);
    mxs = std::max(mxs, G.cell_stride(dir, transposed) * 8);
    // the two-sided kernels form the factor offset block * stride + entry in 32 bits: the whole factor of
    // the direction must stay below 4 GiB (160 x 160 x 768 complex would wrap silently otherwise)
    const i64 fac_bytes = 15 * G.lines_tot(dir) * G.nC[dir] * (i64)G.tsize;
    return mxs < lim24 && G.nC[dir] < lim24 && fac_bytes < ((i64)1 << 32);
}
// A launch of the quad kernel at 16 lines per wave is ONE wave per SIMD (three prefetch stages: 322+ registers; with two stages a
// second wave fits, but one full wave per SIMD is the faster form -- 256^3: 9 lines per wave on two waves per SIMD 0.90 against
// 0.73 ms).  Its waves all last the same time, so a launch of W waves on C = SIMDs wave slots lasts ceil(W / C) rounds: 448^3 --
// 3136 waves = 3.06 rounds of 1024 -- pays four (12.9 % of the roofline where 512^3, exactly four rounds, reaches 16 %).  Deal the
// lines evenly instead: the fewest rounds r that 16 lines per wave allow, then ceil(lines / (C r)) lines per wave (>= 8: levels of
// 8192 ... 16383 lines per colour take the same path -- ONE round of waves instead of 8 lines per wave in up to two).  Measured by size
// (profiles/r05_balanced_lpw.txt, dense source, % of the algorithmic roofline): 288^3 11.6 -> 13.9, 320^3 14.8 -> 15.8, 368^3 12.5 ->
// 14.9, 384^3 13.4 -> 15.1, 448^3 12.9 -> 14.4, 480^3 14.1 -> 14.5; 256^3, 352^3, 512^3 (whole rounds already) unchanged.
// Bit-identical (a line's arithmetic does not know its wave).  lines: of ONE colour launch, all systems (every launch deals its own).
inline int sweep_balanced_lpw(const SweepKnobs& K, i64 lines) {
    const i64 rounds = std::max<i64>(1, (lines + 16 * K.simds - 1) / (16 * K.simds));
    const i64 lpw = (lines + K.simds * rounds - 1) / (K.simds * rounds);
    return (int)std::min<i64>(16, std::max<i64>(lpw, 8));
}

// ---- scan tables of the scan kernel (smooth_qpl.hpp SM) -----------------------------------------------------------------------------
// The matrix part of a lane's row after every full Kogge-Stone step depends on the factor and the level's coefficients only; a table
// [pass][step][k][threads] written once per factor build replaces 16 of the 20 complex multiply-adds, 4 of the 5 LDS writes and 16 of
// the 20 LDS reads of a step by 2 (log2(seg) - 1) 4 tsize bytes of loads per lane and launch (256 B at seg = 8, 384 B at seg = 16,
// complex128).  The kernel form: scan form in colour order, lines inside ONE wave (NW = 1), one block per quad.  The size rule: the
// colour launch has at most scantab_max_threads() threads -- the table is read from memory by every launch, and a launch of many
// threads reads more table than it saves arithmetic -- and the four colours' tables fit scantab_max_bytes.  threads: of the largest
// colour's launch, one system (batched systems share the table).
// Measured (profiles/scan_tables_ab.txt, HISTORY part S; 128^3 F-cycle, lab library, three alternating repetitions, ms per cycle):
// no table 8.217 / 8.242 / 8.214; launches of <= 9000 threads (the 140 launches on 8-block lines: 8192 threads, 2 MB per colour)
// 8.102 / 8.109 / 8.076; <= 40 000 threads (also the 112 launches on 16-block lines) 8.078 / 8.026 / 8.063; every launch the kernel
// form allows 8.080 / 8.070 / 8.061 (the same launches: the cycle has no larger one of this form).  Both classes pay, so
// SCANTAB_THREADS is the largest size that was measured to, 40 000 threads on 1024 SIMDs; nothing larger has been measured, and
// the one larger scan class of that cycle (32-block lines, two blocks per quad, 65 k threads) would read 33 MB of table in a launch
// of 13.7 us: it has no table by its form.
inline i64 sweep_scantab_bytes(int seg, i64 threads, int tsize) {
    int lseg = 0;
    while ((1 << lseg) < seg) ++lseg;
    return 4 * (((threads / 64 + 7) / 8) * 8 * 64) * 2 * (i64)(lseg - 1) * 4 * tsize;     // (grids are rounded up to the 8 XCDs)
}
inline bool sweep_scantab(const SweepKnobs& K, SweepFamily family, int NW, int M, int seg, i64 threads, int tsize) {
    if (K.use_scantab == 0 || K.order != 1 || family != SweepFamily::qpl || NW != 1 || M != 1 || seg < 4 || seg > 16) return false;
    const i64 bytes = sweep_scantab_bytes(seg, threads, tsize);
    if (bytes > K.scantab_max_bytes || bytes >= ((i64)1 << 32)) return false;
    return K.use_scantab == 1 || threads <= K.scantab_max_threads();
}

// ---- THE selection ------------------------------------------------------------------------------------------------------------
// Decided by the level's largest colour, for every colour launch of the (level, direction); the factor's layout follows the family.
inline SweepPlan plan_sweep(const SweepKnobs& K, const SweepShape& G, int dir) {
    SweepPlan p;
    const i64 nL = G.nC[dir], nmax = G.lines(dir), S = K.simds;
    const bool rp_fits = sweep_rp_fits(K, G), qpl = sweep_qpl_on(K, G, dir);
    p.nmax = nmax;
    p.split = sweep_split_on(K, G);
    p.xt = dir == 0 && K.use_xt && G.cells() >= K.xt_min_cells && !qpl;
    p.work_id = p.split ? (dir == 0 ? 0 : 1) : (p.xt ? 2 : 3 + dir);
    p.big = sweep_q_big(K, G) && !rp_fits;
    p.helpers = sweep_tha_helpers(K, G, dir);
    const bool q_on = K.use_q >= 2 || (K.use_q == 1 && nmax >= K.q_min_lines());
    p.fac_kind = (!qpl && sweep_twist_ok(K, G, dir, q_on, p.xt)) ? 3 : (!qpl && (rp_fits || p.big) && q_on) ? 4 : 0;
    p.mid = p.fac_kind == 3 ? (nL - 1) / 2 : nL - 1;            // (factor_m.hpp: qm_mid)
    p.fac_entries = (p.fac_kind == 4 ? 11 : 15) * nL;
    int p1 = 0, p2 = 0;
    if (p.fac_kind == 3 && p.helpers) {
        p.family = SweepFamily::tha;
        p1 = p.helpers;
        p.lpw = SWEEP_THA_LPW; p.rounds = (((nmax + p.lpw - 1) / p.lpw) * K.nsys + S / 4 - 1) / (S / 4);
    } else if (p.fac_kind == 3) {
        // 8 lines per pair of waves, or 12 (60 instead of 40 useful lanes per load instruction: a wave 15 % longer) where that saves a
        // ROUND of waves: the kernel keeps a SIMD's issue slots 43-80 % busy, so W waves on S SIMDs last ceil(W / S) rounds whatever the
        // registers would allow (HISTORY R5.19: 136^3 -- 4624 lines = 1156 waves at 8 lines per pair -- 0.166 ms against 0.092 at 128^3;
        // with 12 lines per pair 772 waves, 0.121 ms).  Single systems of 4097 ... 6144 lines per colour and batched launches (several waves
        // per SIMD either way: 16 128 lines 4 -> 3 rounds) take 12.  The lane mapping does not touch a line's arithmetic.
        p.family = SweepFamily::thm;
        const i64 lines = nmax * K.nsys, r8 = (2 * ((lines + 7) / 8) + S - 1) / S, r12 = (2 * ((lines + 11) / 12) + S - 1) / S;
        p.inst_lpw = (K.th_lpw == 4 || K.th_lpw == 8 || K.th_lpw == 12) ? K.th_lpw : (23 * r12 < 20 * r8) ? 12 : 8;
        p.stages = K.tw_stages ? K.tw_stages : 3;
        p1 = p.stages; p2 = p.inst_lpw;
        p.lpw = p.inst_lpw; p.rounds = (2 * ((nmax + p.lpw - 1) / p.lpw) * K.nsys + S - 1) / S;
    } else if (qpl) {
        // workgroup waves NW, blocks per quad M, quads per line seg (power of two, M * seg >= nL)
        // (lines that fit ONE wave -- seg <= 16 -- get single-wave workgroups: fewer, fatter workgroups were measured slower, 8.54 -> 8.8 /
        // 9.1 / 10.5 ms per 128^3 F-cycle at 2 / 4 / 8 waves, HISTORY R5.13)
        p.M = (nL >= K.qpl_m2_min) ? 2 : 1;
        p.seg = 4; while (p.seg < (nL + p.M - 1) / p.M) p.seg *= 2;
        p.NW = p.seg <= 16 ? 1 : p.seg / 16;
        // (the chain form: single-wave workgroups in colour order)
        p.family = (p.NW == 1 && p.M == 1 && K.order == 1 && p.seg <= K.qpl_chain_seg) ? SweepFamily::qpl_chain : SweepFamily::qpl;
        p1 = p.NW; p2 = p.M;
        p.fac_entries = 15 * (i64)p.M * p.seg;
        p.lpw = (16 * p.NW) / p.seg; p.rounds = (((nmax + p.lpw - 1) / p.lpw) * p.NW * K.nsys + S - 1) / S;
        p.qdesc = K.use_qdesc && K.order == 1 && p.NW == 1 && G.lines_tot(dir) * p.fac_entries < ((i64)1 << 32) &&
                  ((nmax + p.lpw - 1) / p.lpw) * 64 <= K.qdesc_max_threads();
        if (p.family == SweepFamily::qpl && p.NW == 1 && p.M == 1 && K.order == 1)
            p.scantab_bytes = sweep_scantab_bytes(p.seg, ((nmax + p.lpw - 1) / p.lpw) * 64, G.tsize);
        p.scantab = sweep_scantab(K, p.family, p.NW, p.M, p.seg, ((nmax + p.lpw - 1) / p.lpw) * 64, G.tsize);
    } else if ((rp_fits || p.big) && p.fac_kind == 4) {
        // lines per wave: aim at >= ~1000 waves (one per SIMD) before filling lanes
        p.family = p.big ? SweepFamily::qc_big : SweepFamily::qc;
        p.inst_lpw = p.big ? 16 : K.q_lpw ? K.q_lpw : (nmax >= K.q_min_lines() ? 16 : 4);
        // (384^3, 36.9 k lines per colour = 2.2 waves per SIMD: 3 stages again, 119.7 / 121.3 against 123.0 / 122.3 ms per V-cycle,
        // profiles/r05_qstages_ab.txt: the two-stage instantiation pays where a launch is ONE wave per SIMD)
        p.stages = (K.q_stages == 2 || K.q_stages == 3) ? K.q_stages
                 : (p.inst_lpw == 16 && nmax * K.nsys > 15 * S && nmax * K.nsys <= 16 * S) ? 2 : 3;
        p.qlpw = p.inst_lpw == 16 ? sweep_balanced_lpw(K, nmax * K.nsys) : p.inst_lpw;
        p1 = p.stages; p2 = p.inst_lpw;
        p.lpw = p.qlpw; p.rounds = (((nmax + p.lpw - 1) / p.lpw) * K.nsys + S - 1) / S;
    } else if (rp_fits || p.big) {
        // Lines per wave: with few lines the recurrence is latency bound and more waves win (4 lines/wave); with many lines the sweep
        // is HBM bound and fewer, fuller waves move fewer bytes (8 lines/wave).  Measured on MI355X: 128^3 (4032 lines/colour) 0.67 vs
        // 0.75 ms, 256^3 (16129) 5.6 vs 4.6 ms.  By the level's largest colour, not by a colour's own count: the colours of one level
        // must not straddle the threshold (256 x 128 x 128: 8192 / 8128 / 8064 / 8001 lines; 8 lines per wave 0.20 ms per launch, 4 lines
        // per wave 0.30 ms)
        p.family = SweepFamily::rp;
        p.lpw = K.force_lpw ? K.force_lpw : (nmax >= 8 * S ? 8 : 4);
        p.inst_lpw = (p.lpw == 8 || p.lpw == 12) ? (int)p.lpw : 4;
        p1 = p.inst_lpw;
        p.rounds = (((nmax + p.lpw - 1) / p.lpw) * K.nsys + S - 1) / S;
    } else {
        p.family = SweepFamily::tpl;
        p.lpw = 64; p.rounds = (((nmax + 63) / 64) * K.nsys + S - 1) / S;
    }
    sweep_kernel_name(p.name, sizeof p.name, p.family, G.tsize, p1, p2);
    return p;
}

// ---- kept z of k_line_sweep_thm (smooth_thm.hpp) ---------------------------------------------------------------------------------
// The forward pass of a half leaves one z per row and step for the backward pass.  The last kz steps keep theirs in LDS instead of
// parking them in e: 2 x tsize of the bytes a block moves (160 of ~790 B at complex128), in a kernel whose level-0 launch is priced
// by its bytes.  Static LDS and bytes per kept step of a 256-thread workgroup at lpw lines per pair of waves
// (smooth_thm.hpp: thm_static_lds, thm_keep_step_bytes; mg.hpp asserts that the two agree):
constexpr i64 sweep_thm_static_lds(int lpw, int tsize) { return (4 * 2 * 64 + 2 * 3 * 6 * (i64)lpw) * tsize; }
constexpr i64 sweep_thm_keep_step_bytes(int lpw, int tsize) { return 4 * 5 * (i64)lpw * tsize; }
// First kept forward step of a half of K steps under the cap kz: a multiple of the main loops' unroll (3- / 2-stage prefetch: 3 / 2),
// so that parked and kept steps run in branch-free loops of their own; K - result <= kz.  The kernel and the planner call this one.
#if defined(__HIPCC__)
#define SWEEP_HD __host__ __device__
#else
#define SWEEP_HD
#endif
SWEEP_HD inline int sweep_thm_keep_start(int K, int kz, int unroll) {
    if (kz <= 0) return K;
    if (K <= kz) return 0;
    const int k1 = ((K - kz + unroll - 1) / unroll) * unroll;
    return k1 < K ? k1 : K;
}
// The cap kz of a (level, direction): the longest half, or what fits beside the instantiation's static LDS in a workgroup's LDS;
// 0 where another family serves or the device refused the dynamic LDS.  EMG3D_THM_ZKEEP (lab): -1 this, 0 off, n at most n.
// The rule is the same for every launch: a full-depth keep fills the CU's LDS, so that a second workgroup cannot join the first on a
// CU, but the launches of more than one round were measured faster with it, not slower (profiles/thm_zkeep_ab.txt, parent -> keep,
// three alternating runs each): four batched systems at 128^3 (12 lines per pair, 3 rounds, 36 of 63 steps kept) 0.282 -> 0.242 ms per level-0 launch, 21.92 ->
// 20.86 ms per cycle; 144^3 at 12 lines per pair (38 of 71 steps kept) 0.120 -> 0.111 ms per launch.  So there is no
// restriction to one-round plans and no minimum kept share.
inline i64 sweep_thm_zkeep(const SweepKnobs& K, const SweepShape& G, int dir, const SweepPlan& P) {
    if (P.family != SweepFamily::thm || !K.thm_lds_granted || K.thm_zkeep == 0) return 0;
    const i64 n = G.nC[dir], m = (n - 1) / 2, half = std::max(m, n - m - 2);
    const i64 room = K.lds_limit - sweep_thm_static_lds(P.inst_lpw, G.tsize);
    i64 kz = std::min(half, room / sweep_thm_keep_step_bytes(P.inst_lpw, G.tsize));
    if (K.thm_zkeep > 0) kz = std::min(kz, K.thm_zkeep);
    return std::max<i64>(kz, 0);
}

// ---- fused colour passes: how MG::smooth_line ISSUES a call on a level of short lines -----------------------------------------------
// The colour passes of one smoothing call (7 for nu = 2: 4 nu less the colours repeated at the backward -> forward turn-arounds) are dependent launches of a
// few microseconds each.  Where the plan below says so, ONE launch of the same scan kernel (smooth_qpl.hpp, FZ) runs all of them:
// a workgroup owns a SLAB of `own` consecutive line nodes along the longer transverse axis X (P or Q), works on a private copy of
// the part of the field it touches, and recomputes a halo of neighbouring lines that shrinks by one node per pass.  A second launch
// (k_scatter_slabs) writes every edge of the level from its owner's private copy.  The kernel selection (SweepPlan) is untouched.
//
// Geometry along X (nX cells: lines at the nodes 1 .. nX - 1; node-type edges -- those along L and along the other transverse axis --
// sit at nodes 0 .. nX, X-directed edges at cells 0 .. nX - 1, cell c between the nodes c and c + 1):
//   slab k owns the line nodes [x0, x1) = [1 + k own, min(1 + (k + 1) own, nX));
//   pass p of n is LIVE on the nodes [max(1, x0 - h), min(nX - 1, x1 + h)], h = n - 1 - p  (one node wider at the upper end than
//     the own range: an X-directed edge at cell c is written by the lines c and c + 1, and the owner of cell c needs both);
//   a line at node j reads node-type edges at j - 1 .. j + 1 and X-directed edges at the cells j - 1, j, and writes node-type edges
//     at j and the cells j - 1, j.  INVARIANT: everything the live lines of pass p + 1 read is exact after pass p, because every
//     line that writes it in pass p is live in pass p (its own inputs exact by the same argument, the copied-in region covering
//     pass 0).  After the last pass the nodes [x0, x1] and the cells [x0 - 1, x1 - 1] are exact;
//   owner of index j (a node or a cell): slab (j - 1) / own, index 0 with slab 0, the indices past the last own range with the last
//     slab: every edge has exactly one owner, and the owner's copy of it is exact;
//   copied in: the indices [lo(0) - 1, hi(0) + 1] of every component.
constexpr int SWEEP_FUSE_MAX_PASSES = 16;      // (LineArgs::fseq: four bits per pass; nu = 2: 7 passes, nu = 3: 11, nu = 4: 14)
struct FuseGeom { int nX, own, nslabs, npass; };
SWEEP_HD inline int fuse_x0(const FuseGeom& g, int k) { return 1 + k * g.own; }
SWEEP_HD inline int fuse_x1(const FuseGeom& g, int k) { const int x = 1 + (k + 1) * g.own; return (k == g.nslabs - 1 || x > g.nX) ? g.nX : x; }
SWEEP_HD inline int fuse_lo(const FuseGeom& g, int k, int p) { const int v = fuse_x0(g, k) - (g.npass - 1 - p); return v < 1 ? 1 : v; }
SWEEP_HD inline int fuse_hi(const FuseGeom& g, int k, int p) { const int v = fuse_x1(g, k) + (g.npass - 1 - p); return v > g.nX - 1 ? g.nX - 1 : v; }
SWEEP_HD inline int fuse_owner(const FuseGeom& g, int j) { const int k = j <= 0 ? 0 : (j - 1) / g.own; return k > g.nslabs - 1 ? g.nslabs - 1 : k; }

struct FusePlan {
    bool fused = false;
    int axis = 0;               // slabs along 0: P, 1: Q (the longer one; P on a tie)
    int nw = 0;                 // waves per workgroup
    FuseGeom g = {0, 0, 0, 0};
    i64 scratch_bytes = 0;      // private copies: systems x slabs x edges of the level
};
// transverse axes of a line direction (MG::line_args)
inline void sweep_axes(int dir, int& P, int& Q) { P = dir == 0 ? 1 : 0; Q = dir == 2 ? 1 : 2; }
inline FusePlan plan_fuse(const SweepKnobs& K, const SweepShape& G, int dir, int npass) {
    FusePlan f;
    const SweepPlan p = plan_sweep(K, G, dir);
    // the scan kernel, one wave per line, descriptors (the fused loop indexes the per-colour tables of MG::ensure_qdesc)
    if (K.order != 1 || (p.family != SweepFamily::qpl && p.family != SweepFamily::qpl_chain) || p.NW != 1 || p.M != 1 || !p.qdesc) return f;
    if (p.seg > K.fuse_max_seg || p.seg > 8 || npass < 3 || npass > SWEEP_FUSE_MAX_PASSES) return f;
#ifndef EMG3D_LAB
    if (p.family != SweepFamily::qpl_chain) return f;      // (the scan form of the fused loop lost its A/B: lab build only)
#endif
    int P, Q;
    sweep_axes(dir, P, Q);
    f.axis = G.nC[Q] > G.nC[P] ? 1 : 0;
    const i64 nX = G.nC[f.axis ? Q : P];
    if (nX < 2 || nX > (1 << 20)) return f;
    i64 own = K.fuse_own > 0 ? K.fuse_own : 2;
    own = std::min<i64>(own, nX - 1);
    f.g.nX = (int)nX; f.g.own = (int)own; f.g.nslabs = (int)((nX - 1 + own - 1) / own); f.g.npass = npass;
    f.nw = p.family == SweepFamily::qpl_chain ? 8 : 4;     // (8 waves: a pass of a 4-block slab is one round; 4 at 4 waves per round lost)
    f.scratch_bytes = (i64)K.nsys * f.g.nslabs * G.edges() * (i64)G.tsize;
    f.fused = f.scratch_bytes <= K.fuse_max_bytes;
    return f;
}
