// Device-resident multigrid hierarchy and cycle driver.
//
// Restates the control flow of solver.multigrid / smoothing / restriction /
// prolongation / residual (reference emg3d/solver.py:434-607, 738-1039) with
// every array resident in HBM: the host only enqueues kernels on one stream.
// The reference rebuilds the coarse grid, model, weights and prolongator at
// every visit (solver.py:859-899, 933-963); here each hierarchy (one per
// global semicoarsening direction var.sc_dir in 0..3) is built once, lazily,
// and the line factorisations are cached per (level, direction).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <chrono>
#include <vector>

#include "common.hpp"
#include "smooth.hpp"
#include "stencil.hpp"
#include "gradient.hpp"        // k_gradient_acc, k_sens_acc (acc_add, sens_acc_add)
#include "regrid.hpp"          // k_volume_average_adjoint (regrid_acc)
#include "rows.hpp"            // rows_park (sens_rows_park): the row store is a unit of its own
#include "smooth_qpl.hpp"
#include "smooth_qc.hpp"
#include "smooth_thm.hpp"
#include "smooth_tha.hpp"
#include "sweep_launch.hpp"     // the four sweep families are compiled in units of their own; this file launches through these
#include "sweep_plan.hpp"       // ... and which of them serves a (level, direction) is decided there, on the host

template <class T>
struct Level {
    i64 nC[3];
    i64 nE, nCells;
    FieldLayout fl;
    CellLayout cl;
    std::vector<double> h_host[3], nodes[3], centers[3];
    double* h[3] = {nullptr, nullptr, nullptr};
    double* ih[3] = {nullptr, nullptr, nullptr};   // 1/h
    T* eta[3] = {nullptr, nullptr, nullptr};
    double* zeta = nullptr;
    unsigned char* sflag[3] = {nullptr, nullptr, nullptr};   // level 0: per line direction, which lines carry a source
    bool sflag_valid[3] = {false, false, false};
    bool s_dense = false;       // the source came from a Krylov vector (emg3d_mg_vec_copy): every line counts as carrying one
    bool zeta_sep = false;      // zeta == (hx hy) hz bit for bit (level 0 of a model without mu_r): MG::check_zeta
    T *s = nullptr, *e = nullptr, *r = nullptr;
    // x<->y transposed working copies (y fastest) for line relaxation along x:
    // lanes run across lines, so the transverse axis must be the contiguous one.
    T *eT = nullptr, *sT = nullptr;
    T* etaT[3] = {nullptr, nullptr, nullptr};
    double* zetaT = nullptr;
    bool sT_valid = false;
    FieldLayout flT;
    CellLayout clT;
    // parity-split working copies for the sweeps: [0] x-lines: (y-split, x, z);
    // [1] y-/z-lines: (x-split, y, z).  Same strides as flT / fl.
    T *eW[2] = {nullptr, nullptr}, *sW[2] = {nullptr, nullptr};
    double* zetaW[2] = {nullptr, nullptr};
    bool sW_valid[2] = {false, false};
    // levels with split working copies: where the field currently lives -- 0: e (reference layout), 1: eW[1] (x-split;
    // e is then stale).  Level 0 moves between the two (MG::home_on); the coarse levels are at home in eW[1] / sW[1] for
    // good (MG::home_lvl: the restriction writes there, the prolongation reads there; e and s are never touched).
    int e_home = 0;
    // cached line factorisations
    T* fac[3] = {nullptr, nullptr, nullptr};
    // per-lane launch descriptors of the scan kernel's colour launches (LineArgs::qd; smooth_qpl.hpp DM): [direction][colour]
    void* qd[3][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};
    unsigned qdn[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    // scan tables of the same launches (LineArgs::sm; smooth_qpl.hpp SM): [direction][colour]; they hold products of the factor, and
    // are rewritten whenever it is recomputed
    void* sm[3][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};
    unsigned smn[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    // private slab copies of the fused smoothing calls (MG::ensure_fuse): [system][slab][nE], elements allocated
    T* fz[3] = {nullptr, nullptr, nullptr};
    i64 fz_n[3] = {0, 0, 0};
    // how a smoothing call of fuse_key = nu * 256 + order + 2 * systems is issued (MG::ensure_fuse; -1: not yet), and the colours of its passes
    FusePlan fuse[3];
    int fuse_key[3] = {-1, -1, -1};
    std::vector<int> passes[3];
    i64 fac_lines[3] = {0, 0, 0};
    i64 fac_mid[3] = {0, 0, 0};   // middle block of the (two-sided) factorisation
    int fac_kind[3] = {0, 0, 0};  // 0: one-sided, 15 numbers per block (k_line_sweep_rp / _qpl, k_line_sweep); 3: mirrored
                                  // two-sided (k_line_factor_m, for k_line_sweep_thm); 4: one-sided compact (11 numbers per
                                  // block, k_line_sweep_qc)
    // the launch selection of each direction (MG::plan), computed for plan_key = order + 2 * systems (-1: not yet)
    SweepPlan plan[3];
    int plan_key[3] = {-1, -1, -1};
};

// Transfer operators between a level and the next coarser one of a hierarchy.
struct Transfer {
    int sc = -1;         // current sc_dir (0..6) used to build the child
    int co[3] = {0, 0, 0};
    double* w[3][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    int* pidx[3] = {nullptr, nullptr, nullptr};
    double* pwt[3] = {nullptr, nullptr, nullptr};
};

template <class T>
struct Hierarchy {
    std::vector<std::shared_ptr<Level<T>>> lv;
    std::vector<Transfer> tr;     // tr[l]: between lv[l] and lv[l+1]
};

// Freed device blocks are kept for the next handle of the process (exact-size reuse).  Solves come in
// series on the same grid (frequencies, sources, Krylov restarts), so a new handle asks for exactly the
// sizes the last one returned; going through hipFree / hipMalloc instead costs ~13 ms per close of a 128^3
// handle plus the allocation time of the next one.  Bounded by EMG3D_POOL_GB (default 96 GiB per process; 0 disables);
// emg3d_hip_release_cached() returns everything to the driver.
class DevicePool {
    std::mutex mu;
    // A parked block remembers the ROLE it was placed for (MG::place_level0: tag 1 / 2 = the working copy the x- / the y- and z-line
    // sweeps of a large level 0 write; 0 = none): the next handle of the same size asks for its working copies by role and gets the
    // blocks the last handle had searched for, instead of searching again.
    struct Parked { void* p; int tag; };
    std::multimap<std::pair<int, size_t>, Parked> free_blocks;     // device < 0: pinned host memory of device -1 - key
    size_t held = 0, cap;
public:
    DevicePool() {
        const char* g = getenv("EMG3D_POOL_GB");
        cap = (size_t)((g ? atof(g) : 96.0) * (double)((size_t)1 << 30));
    }
    // tag != 0: a block parked with that tag if there is one (*hit = true), else an untagged one, else any; tag == 0: untagged
    // blocks first (the tagged ones stay for the working copies that will ask for them)
    void* take(int device, size_t nb, int tag = 0, bool* hit = nullptr) {
        std::lock_guard<std::mutex> lk(mu);
        if (hit) *hit = false;
        auto rng = free_blocks.equal_range({device, nb});
        if (rng.first == rng.second) return nullptr;
        auto pick = rng.second;
        for (auto it = rng.first; it != rng.second; ++it) if (it->second.tag == tag) { pick = it; break; }
        if (pick == rng.second && tag != 0)
            for (auto it = rng.first; it != rng.second; ++it) if (it->second.tag == 0) { pick = it; break; }
        if (pick == rng.second) pick = rng.first;
        if (hit) *hit = tag != 0 && pick->second.tag == tag;
        void* p = pick->second.p;
        free_blocks.erase(pick);
        held -= nb;
        return p;
    }
    bool give(int device, void* p, size_t nb, int tag = 0) {     // false: not kept, the caller frees
        std::lock_guard<std::mutex> lk(mu);
        if (held + nb > cap) return false;
        free_blocks.insert({{device, nb}, Parked{p, tag}});
        held += nb;
        return true;
    }
    size_t release_all() {
        std::lock_guard<std::mutex> lk(mu);
        const size_t n = held;
        int cur = 0;
        (void)hipGetDevice(&cur);
        for (auto& kv : free_blocks) {
            if (kv.first.first < 0) { (void)hipHostFree(kv.second.p); continue; }
            (void)hipSetDevice(kv.first.first); (void)hipFree(kv.second.p);
        }
        for (auto& kv : free_streams) { (void)hipSetDevice(kv.first); (void)hipStreamDestroy(kv.second); }
        free_streams.clear();
        (void)hipSetDevice(cur);
        free_blocks.clear();
        held = 0;
        return n;
    }
    size_t bytes_held() { std::lock_guard<std::mutex> lk(mu); return held; }
    size_t bytes_held_on(int device) {      // device memory parked for `device` (keys < 0 are pinned host blocks)
        std::lock_guard<std::mutex> lk(mu);
        size_t n = 0;
        for (auto& kv : free_blocks) if (kv.first.first == device) n += kv.first.second;
        return n;
    }
    // HIP streams of closed handles (creating and destroying one costs about a millisecond each; a solve makes two):
    // idle -- their handle synchronised them before giving them back -- and non-blocking
    std::multimap<int, hipStream_t> free_streams;
    hipStream_t take_stream(int device) {
        {
            std::lock_guard<std::mutex> lk(mu);
            auto it = free_streams.find(device);
            if (it != free_streams.end()) { hipStream_t s = it->second; free_streams.erase(it); return s; }
        }
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return s;
    }
    void give_stream(int device, hipStream_t s) {
        std::lock_guard<std::mutex> lk(mu);
        if (free_streams.count(device) < 16) free_streams.insert({device, s});
        else (void)hipStreamDestroy(s);
    }
    static DevicePool& get() { static DevicePool* p = new DevicePool(); return *p; }   // never destroyed: no HIP calls at exit
};

inline int current_sc_dir(int sc_dir, const i64 nC[3]) {   // solver.py:1467-1514
    const bool xs = nC[0] % 2 != 0 || nC[0] < 3 || sc_dir == 1;
    const bool ys = nC[1] % 2 != 0 || nC[1] < 3 || sc_dir == 2;
    const bool zs = nC[2] % 2 != 0 || nC[2] < 3 || sc_dir == 3;
    if (xs) { if (ys) return 6; return zs ? 5 : 1; }
    if (ys) return zs ? 4 : 2;
    return zs ? 3 : 0;
}

inline int current_lr_dir(int lr, const i64 nC[3]) {       // solver.py:1517-1572
    if (nC[0] == 2) { if (lr == 1) lr = 0; else if (lr == 5) lr = 3; else if (lr == 6) lr = 2; else if (lr == 7) lr = 4; }
    if (nC[1] == 2) { if (lr == 2) lr = 0; else if (lr == 4) lr = 3; else if (lr == 6) lr = 1; else if (lr == 7) lr = 5; }
    if (nC[2] == 2) { if (lr == 3) lr = 0; else if (lr == 4) lr = 2; else if (lr == 5) lr = 1; else if (lr == 7) lr = 6; }
    return lr;
}

inline void sc_axes(int sc, int co[3]) {                    // solver.py:850-856
    co[0] = !(sc == 1 || sc == 5 || sc == 6);
    co[1] = !(sc == 2 || sc == 4 || sc == 6);
    co[2] = !(sc == 3 || sc == 4 || sc == 5);
}

// core.restrict_weights, emg3d/core.py:1970-2041 (O(n) host work).
inline void restrict_weights_host(const double* vectorN, const double* vectorCC, const double* h, i64 nh,
                                  const double* cvectorN, const double* cvectorCC, const double* ch,
                                  i64 n, double* wl, double* w0, double* wr) {
    std::vector<double> d(n + 1);
    d[0] = h[0] / 2; d[n] = h[nh - 1] / 2;
    for (i64 i = 1; i < n; ++i) d[i] = (h[2 * i - 2] + h[2 * i - 1]) / 2.;
    for (i64 i = 0; i < n; ++i) wl[i] = 1 / d[i];
    wl[0] *= (vectorN[0] - h[0] / 2) - (cvectorN[0] - ch[0] / 2);
    for (i64 i = 1; i < n; ++i) wl[i] *= vectorCC[2 * i - 1] - cvectorCC[i - 1];
    for (i64 i = 0; i < n; ++i) w0[i] = 1.0;
    for (i64 i = 0; i < n; ++i) wr[i] = 1 / d[i + 1];
    wr[n - 1] *= (cvectorN[n - 1] + ch[n - 2] / 2) - (vectorN[nh] + h[nh - 1] / 2);
    for (i64 i = 0; i < n - 1; ++i) wr[i] *= cvectorCC[i] - vectorCC[2 * i];
}

// RegularGridProlongator._set_edges_and_weights, solver.py:1432-1447:
// i = searchsorted(c, x) - 1 clipped to [0, size-2]; t = (x - c[i])/(c[i+1]-c[i]).
inline void prolong_weights_host(const std::vector<double>& cn, const std::vector<double>& fn,
                                 std::vector<int>& idx, std::vector<double>& wt) {
    idx.resize(fn.size()); wt.resize(fn.size());
    for (size_t j = 0; j < fn.size(); ++j) {
        i64 i = (i64)(std::lower_bound(cn.begin(), cn.end(), fn[j]) - cn.begin()) - 1;
        if (i < 0) i = 0;
        if (i > (i64)cn.size() - 2) i = (i64)cn.size() - 2;
        idx[j] = (int)i;
        wt[j] = (fn[j] - cn[i]) / (cn[i + 1] - cn[i]);
    }
}

struct emg3d_mg {
    virtual ~emg3d_mg() {}
    int dtype = 1;
};

// Every kernel launch of a handle goes through MG_LAUNCH: after a failed device allocation (MG::broken) some array of the
// handle is missing, and a kernel that touches a null pointer takes the whole PROCESS down with a memory fault instead of
// returning the error.  A broken handle launches nothing; every entry point answers hipErrorOutOfMemory until it is destroyed.
#define MG_LAUNCH(...) do { if (!broken) hipLaunchKernelGGL(__VA_ARGS__); } while (0)

// One launch of a per-cell kernel K<T, SPLIT> of gradient.hpp on level 0 of the handle `mg` (one thread per cell, 256 per block),
// SPLIT chosen by `split` here and nowhere else: nC and the field layout go in front of the kernel's own arguments (...), the widths
// and the three output pointers `a` behind them.
#define MG_CELL_LAUNCH_(mg, K, S, a, ...)                                                                                          \
    hipLaunchKernelGGL((K<T, S>), dim3((unsigned)(((mg).lv0->nCells + 255) / 256)), dim3(256), 0, (mg).stream, (mg).lv0->nC[0],     \
                       (mg).lv0->nC[1], (mg).lv0->nC[2], (mg).lv0->fl, __VA_ARGS__, (const double*)(mg).lv0->h[0],                 \
                       (const double*)(mg).lv0->h[1], (const double*)(mg).lv0->h[2], (a)[0], (a)[1], (a)[2])
#define MG_CELL_LAUNCH(mg, K, split, a, ...)                            \
    do {                                                                \
        if ((mg).broken) break;                                         \
        if (split) MG_CELL_LAUNCH_(mg, K, true, a, __VA_ARGS__);        \
        else MG_CELL_LAUNCH_(mg, K, false, a, __VA_ARGS__);             \
    } while (0)

// The device's part of the selection knobs (sweep_plan.hpp): its SIMDs, its LDS per workgroup, and whether k_line_sweep_tha gets the
// dynamic LDS it needs -- more than 64 KB must be asked for per instantiation and device, once (tha_attrs, on the current device).
static_assert(SWEEP_THA_LPW == THA_LPW && SWEEP_THA_RING == tha_ring_depth<3>() && SWEEP_THA_RING == tha_ring_depth<2>() &&
              SWEEP_THA_MAX_DYN_LDS == THA_MAX_DYN_LDS && SWEEP_THA_STATIC_LDS == THA_STATIC_LDS, "sweep_plan.hpp restates smooth_tha.hpp");
// ... and the kept z of k_line_sweep_thm (sweep_thm_zkeep): asked for in the same place, with the device's LDS per workgroup
template <class T, int LPW>
constexpr bool sweep_thm_lds_agrees() {
    return sweep_thm_static_lds(LPW, (int)sizeof(T)) == (i64)thm_static_lds<T, LPW>() &&
           sweep_thm_keep_step_bytes(LPW, (int)sizeof(T)) == (i64)thm_keep_step_bytes<T, LPW>();
}
static_assert(sweep_thm_lds_agrees<double, 4>() && sweep_thm_lds_agrees<double, 8>() && sweep_thm_lds_agrees<double, 12>() &&
              sweep_thm_lds_agrees<c128, 4>() && sweep_thm_lds_agrees<c128, 8>() && sweep_thm_lds_agrees<c128, 12>(),
              "sweep_plan.hpp restates smooth_thm.hpp");
template <class T>
inline void sweep_device_knobs(SweepKnobs& K, int device) {
    int cus = 0, lds = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) { (void)hipGetLastError(); lds = 0; }
    K.simds = 4 * (i64)cus;
    K.lds_limit = lds;
    K.tha_lds_granted = lds >= THA_MAX_DYN_LDS + THA_STATIC_LDS && tha_attrs<T>(THA_MAX_DYN_LDS);
    K.thm_lds_granted = thm_attrs<T>(lds);
}

template <class T>
struct MG : emg3d_mg {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    double origin[3] = {0, 0, 0};
    std::shared_ptr<Level<T>> lv0;
    std::map<int, Hierarchy<T>> hier;   // key: global sc_dir
    std::vector<std::pair<void*, size_t>> allocs;
    i64 bytes = 0;
    // parameters (MGParameters subset)
    int cycle = 'F', cycmax = 2, nu_init = 0, nu_pre = 2, nu_coarse = 1, nu_post = 2, order = 1;
    int clevel[4] = {0, 0, 0, 0};
    bool eta_alias[3] = {false, false, false};   // eta_y/eta_z alias eta_x
    // scratch
    double* partials = nullptr; i64 n_partials = 0;
    double* norms = nullptr;    // device
    T* scratch_field = nullptr; // nE scratch (Krylov matvec input)
    static const int NORM_SLOTS = 4096;
    int err = 0;
    bool broken = false;        // a device allocation failed: arrays are missing, nothing is launched any more (MG_LAUNCH)
    // ---- kernel selection: sweep_plan.hpp ------------------------------------------------------------------------------------
    // The product library reads six documented variables: EMG3D_POOL_GB, EMG3D_GRAPH, EMG3D_LOG, EMG3D_LOG_SETUP, EMG3D_BATCH_TUNE,
    // EMG3D_PLACE_TRIES; the lab build (-DEMG3D_LAB) one per knob (LAB_ENV, common.hpp).  The selection's knobs and the device's size
    // are filled once per handle; the plan of a (level, direction) is kept on the Level.
    SweepKnobs knobs;
    bool knobs_device = false;          // the device's part of `knobs` has been asked for
    const SweepPlan& plan(Level<T>& L, int dir) {
        if (!knobs_device) { sweep_device_knobs<T>(knobs, device); knobs_device = true; }
        if (L.plan_key[dir] != order + 2 * nsys) {
            knobs.order = order; knobs.nsys = nsys;
            L.plan[dir] = plan_sweep(knobs, SweepShape{{L.nC[0], L.nC[1], L.nC[2]}, (int)sizeof(T)}, dir);
            L.plan_key[dir] = order + 2 * nsys;
        }
        return L.plan[dir];
    }
    bool use_graph = !(getenv("EMG3D_GRAPH") && getenv("EMG3D_GRAPH")[0] == '0');    // replay captured cycles (0: eager launches)
    // verb = 5 of the reference (solver.py:502-578): the residual norm after every smoothing call of every level.  With
    // `trace` on the cycles run eagerly; each smoothing call is followed by a norm-only residual into trace_norms and a
    // record (iteration and cycmax of the level's loop, level, grid, kind 0 coarsest / 1 pre- / 2 post-smoothing).
    bool trace = false;
    struct TraceRec { int it, level, cycmax, kind; i64 n[3]; };
    std::vector<TraceRec> trace_recs;
    static const int TRACE_MAX = 16384;
    int trace_dropped = 0;      // smoothing calls beyond TRACE_MAX since the last emg3d_mg_get_trace (reported there)
    double* trace_norms = nullptr;
    double* norm_out = nullptr;             // where residual(mode 2) puts its norms (nullptr: norms)
    std::map<int, hipGraphExec_t> graphs;
    std::map<int, std::pair<int, int>> graph_home;      // per captured cycle: Level::e_home of level 0 on entry / on exit
    std::map<int, int> graph_seen;
    bool dry = false;           // dry run: allocate/prepare only, launch nothing
    bool log_launches = getenv("EMG3D_LOG") != nullptr;                 // one line per sweep launch on stderr
    int xcd_map = (int)LAB_ENV("EMG3D_XCD", 1);                         // XCD-aware workgroup -> line map
    // k_residual: block map and node planes per thread (stencil.hpp; every setting gives identical results): levels of
    // >= 1 M cells run k_residual_zm with 4 planes per thread (8 from 8 M cells x systems on) on y-strips per XCD, smaller
    // levels the plain kernel on z-slabs per XCD; launches of < 16 blocks per plane keep the plain map.
    int res_xcd = (int)LAB_ENV("EMG3D_RES_XCD", -1);                    // -1: by kernel (zm: 2, plain: 1)
    int res_xcd_min = (int)LAB_ENV("EMG3D_RES_XCD_MIN", 16);
    int res_kz = res_kz_env();                                          // 0: by size
    i64 res_zm_min = LAB_ENV("EMG3D_RES_ZM_MIN_CELLS", (i64)1 << 20);
    static int res_kz_env() {
        const int k = (int)LAB_ENV("EMG3D_RES_KZ", 0);
        return (k == 0 || k == 2 || k == 4 || k == 8 || k == 16) ? k : 1;
    }
    bool skip_idempotent = LAB_ENV("EMG3D_SKIP_IDEMPOTENT", 1) != 0;    // colour mode: skip the repeated colour at turn-arounds
    // The order in which the sweeps of a smoothing call visit the four line colours c = cP + 2 cQ: the odd ("backward")
    // sweeps 0,3,2,1, the even ("forward") ones 1,3,0,2 -- two sweeps visit 0,3,2,1,(1),3,0,2: the colour at the turn-around
    // would be solved twice in a row and is skipped (skip_idempotent).  Chosen by measurement over the 24 x 24 pairs of
    // orders (profiles/HISTORY.md A.12): forward 0,1,2,3 / backward 3,2,1,0, the mirror image of the reference's
    // lexicographic back-and-forth, is the slowest of all (0.417 mean reduction per cycle on six problems; this schedule
    // 0.356; the 128^3 F-cycle bench problem 9 -> 7 cycles at the same 7 colour passes per two sweeps).  The oracle's
    // colour twin uses the same tables.  EMG3D_COLOUR_ORDER / EMG3D_COLOUR_ORDER_B=<4 digits> (lab): other orders.
    int colour_perm[4] = {1, 3, 0, 2};
    int colour_perm_b[4] = {0, 3, 2, 1};        // as visited
    // point smoother: 8 colours c = cx + 2 cy + 4 cz, visited 0..7 in EVERY sweep (plain multi-colour Gauss-Seidel): the
    // reversed pair 7..0 / 0..7 of rounds 1-3 needed 7 / 8 / 13 cycles where this needs 5 / 6 / 9, any order repeated
    // unchanged does as well (profiles/r03_point_order.txt, HISTORY.md A.12).  EMG3D_POINT_ORDER / _B (lab): other orders.
    int point_perm[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    int point_perm_b[8] = {0, 1, 2, 3, 4, 5, 6, 7};
#ifdef EMG3D_LAB
    void read_colour_perm() {
        const char* e = getenv("EMG3D_COLOUR_ORDER");
        if (e && strlen(e) == 4) for (int k = 0; k < 4; ++k) { colour_perm[k] = (e[k] - '0') & 3; colour_perm_b[3 - k] = colour_perm[k]; }
        e = getenv("EMG3D_COLOUR_ORDER_B");
        if (e && strlen(e) == 4) for (int k = 0; k < 4; ++k) colour_perm_b[k] = (e[k] - '0') & 3;
        e = getenv("EMG3D_POINT_ORDER");
        if (e && strlen(e) == 8) for (int k = 0; k < 8; ++k) { point_perm[k] = (e[k] - '0') & 7; point_perm_b[7 - k] = point_perm[k]; }
        e = getenv("EMG3D_POINT_ORDER_B");
        if (e && strlen(e) == 8) for (int k = 0; k < 8; ++k) point_perm_b[k] = (e[k] - '0') & 7;
    }
#endif
    int use_zsep = (int)LAB_ENV("EMG3D_ZSEP", 1);                       // lab: 0 = always read zeta
    int q_tile = (int)LAB_ENV("EMG3D_Q_TILE", 0);                       // lab: switches of in-kernel instrumentation (LineArgs::tile; 256: timestamps of k_line_sweep_tha)

#ifdef EMG3D_LAB
    MG() { read_colour_perm(); }
#else
    MG() {}
#endif

    ~MG() override {
        hipSetDevice(device);
        if (stream) hipStreamSynchronize(stream);
        if (side) hipStreamSynchronize(side);
        drop_graphs();
        for (auto& pn : allocs)
            if (!DevicePool::get().give(device, pn.first, pn.second, tag_of(pn.first))) hipFree(pn.first);
        if (stage && !DevicePool::get().give(-1 - device, stage, STAGE_BYTES)) hipHostFree(stage);
        if (ev_norm) hipEventDestroy(ev_norm);
        if (ev_prep) hipEventDestroy(ev_prep);
        if (broken) {       // (streams of a handle that failed half-way -- possibly inside a capture -- are not passed on)
            if (side) (void)hipStreamDestroy(side);
            if (own_stream && stream) (void)hipStreamDestroy(stream);
            (void)hipGetLastError();
            return;
        }
        if (side) DevicePool::get().give_stream(device, side);
        if (own_stream && stream) DevicePool::get().give_stream(device, stream);
    }

    // A handle makes ~500 device allocations (levels x work copies x factor caches), most of them small:
    // hipMalloc/hipFree cost tens of microseconds each, so requests up to ARENA_CHUNK/4 are carved out of
    // 32 MiB chunks (256-byte aligned, freed together with the handle); larger ones get their own hipMalloc.
    static constexpr size_t ARENA_CHUNK = (size_t)32 << 20;
    char* arena_cur = nullptr;
    size_t arena_left = 0;
    // role tags of blocks that were placed (DevicePool): block -> tag; want_tag / got_tag: the role the next dalloc asks the pool for
    std::map<void*, int> block_tag;
    int want_tag = 0;
    bool got_tag = false;
    int tag_of(void* p) const { auto it = block_tag.find(p); return it == block_tag.end() ? 0 : it->second; }
    void* raw_alloc(size_t nb) {
        if (broken) return nullptr;             // (one failure is reported; the handle asks for nothing more)
        void* p = DevicePool::get().take(device, nb, want_tag, &got_tag);
        if (!p) {
            hipError_t st = hipMalloc(&p, nb);
            if (st != hipSuccess) {     // out of memory with blocks parked in the pool: release them and retry once
                (void)hipGetLastError();
                if (DevicePool::get().release_all() > 0) st = hipMalloc(&p, nb);
            }
            if (st != hipSuccess) {
                (void)hipGetLastError();
                if (alloc_quiet) return nullptr;        // (try_alloc: optional memory)
                err = (int)st; broken = true;
                fprintf(stderr, "[emg3d_hip] hipMalloc(%zu) failed: %s\n", nb, hipGetErrorString(st)); return nullptr;
            }
        }
        allocs.push_back({p, nb});
        return p;
    }
    template <class U>
    U* dalloc(i64 n) {
        const size_t nb = (((size_t)std::max<i64>(n, 1) * sizeof(U)) + 255) & ~(size_t)255;
        bytes += (i64)nb;
        if (nb > ARENA_CHUNK / 4) return (U*)raw_alloc(nb);
        if (nb > arena_left) {
            arena_cur = (char*)raw_alloc(ARENA_CHUNK);
            arena_left = arena_cur ? ARENA_CHUNK : 0;
            if (!arena_cur) return nullptr;
        }
        U* p = (U*)arena_cur;
        arena_cur += nb;
        arena_left -= nb;
        return p;
    }
    // Host -> device copy of a set-up array (widths, transfer weights: ~150 small arrays per hierarchy).
    // The host buffers may be temporaries, so small ones are staged through a pinned ring buffer and
    // copied asynchronously (one stream synchronisation per STAGE_BYTES instead of one per array).
    static constexpr size_t STAGE_BYTES = (size_t)2 << 20;
    static constexpr size_t STAGE_RING = STAGE_BYTES - 4096;      // the last 4 KiB: pinned landing place of the norms
    char* stage = nullptr;
    size_t stage_off = 0;
    hipEvent_t ev_norm = nullptr;
    void ensure_stage() {
        if (!stage) stage = (char*)DevicePool::get().take(-1 - device, STAGE_BYTES);
        if (!stage && hipHostMalloc((void**)&stage, STAGE_BYTES, hipHostMallocDefault) != hipSuccess) { stage = nullptr; (void)hipGetLastError(); }
    }
    // One cycle, and while the device runs it the loop-invariant set-up of the NEXT (sc_dir, lr_dir) pair on the host
    // (hierarchy, factor kernels, graph capture: 5 ms at 128^3 -- the solver rotates through up to three pairs, so the
    // second and third cycle of a solve otherwise wait for it).  The norms come back through pinned memory behind an
    // event recorded right after the cycle; what prepare() enqueues runs after it.
    // prepare() with everything it enqueues -- uploads, coarse models, factor kernels, the graph upload -- on a second
    // stream, so that the device runs it BESIDE the cycle instead of behind it (the coarse levels of a cycle leave most
    // CUs idle); the handle's stream then waits for it before whatever comes next.  The new pair's buffers are not
    // touched by the running cycle, and what it shares with it (level-0 model, source, widths) is only read.
    hipStream_t side = nullptr;
    hipEvent_t ev_prep = nullptr;
    void prepare_aside(int g, int lr_dir) {
        // (a pair whose set-up still has to place level 0's working copies times sweeps: on the handle's own stream, behind the cycle)
        if (!prepare_on_side || placement_pending(lr_dir)) { prepare(g, lr_dir); return; }
        if (!side) side = DevicePool::get().take_stream(device);
        if (!side || (!ev_prep && hipEventCreateWithFlags(&ev_prep, hipEventDisableTiming) != hipSuccess)) {
            (void)hipGetLastError();
            prepare(g, lr_dir);
            return;
        }
        std::swap(stream, side);
        prepare(g, lr_dir);
        hipError_t st = hipEventRecord(ev_prep, stream);
        std::swap(stream, side);
        if (st == hipSuccess) st = hipStreamWaitEvent(stream, ev_prep, 0);
        if (st != hipSuccess) {                       // cannot order the streams: wait on the host instead
            (void)hipGetLastError();
            hipStreamSynchronize(side);
        }
    }
    int prepare_on_side = (int)LAB_ENV("EMG3D_PREPARE_SIDE", 1);
    int cycle_then_prepare(int g, int lr_dir, int ng, int nlr, double* out) {
        cycle0(g, lr_dir, 0);
        ensure_stage();
        if (!stage || nsys * sizeof(double) > 4096) {           // no pinned memory: plain order
            if (ng >= 0) prepare(ng, nlr);
            hipError_t st = d2h(out, norms, (size_t)nsys * sizeof(double));
            if (st != hipSuccess && err == 0) err = (int)st;
            return 0;
        }
        double* land = (double*)(stage + STAGE_RING);
        hipError_t st = hipMemcpyAsync(land, norms, (size_t)nsys * sizeof(double), hipMemcpyDeviceToHost, stream);
        if (st == hipSuccess && !ev_norm) st = hipEventCreateWithFlags(&ev_norm, hipEventDisableTiming);
        if (st == hipSuccess) st = hipEventRecord(ev_norm, stream);
        if (st == hipSuccess && ng >= 0) prepare_aside(ng, nlr);
        if (st == hipSuccess) st = hipEventSynchronize(ev_norm);
        if (st != hipSuccess) { if (err == 0) err = (int)st; return 0; }
        memcpy(out, land, (size_t)nsys * sizeof(double));
        return 0;
    }
    template <class U>
    U* upload(const U* host, i64 n) {
        U* d = dalloc<U>(n);
        if (!d || n <= 0) return d;
        const size_t nb = (size_t)n * sizeof(U);
        hipError_t st;
        ensure_stage();
        if (stage && nb <= STAGE_RING / 4) {
            if (stage_off + nb > STAGE_RING) {      // (both streams: copies out of the ring may be pending on either)
                hipStreamSynchronize(stream);
                if (side) hipStreamSynchronize(side);
                stage_off = 0;
            }
            memcpy(stage + stage_off, host, nb);
            st = hipMemcpyAsync(d, stage + stage_off, nb, hipMemcpyHostToDevice, stream);
            stage_off += (nb + 63) & ~(size_t)63;
        } else {
            st = h2d(d, host, nb);
        }
        if (st != hipSuccess) err = (int)st;
        return d;
    }
    // Whole-field host <-> device copies, synchronous (the runtime pins the caller's array and DMAs from
    // it: 102 MB in 2-8 ms; staging through own pinned chunks was measured slower and is not needed).
    hipError_t h2d(void* dst, const void* src, size_t nb) {
        hipError_t st = hipMemcpyAsync(dst, src, nb, hipMemcpyHostToDevice, stream);
        return st == hipSuccess ? hipStreamSynchronize(stream) : st;
    }
    hipError_t d2h(void* dst, const void* src, size_t nb) {
        hipError_t st = hipMemcpyAsync(dst, src, nb, hipMemcpyDeviceToHost, stream);
        return st == hipSuccess ? hipStreamSynchronize(stream) : st;
    }

    void check_launch() {
        hipError_t st = hipGetLastError();
        if (st != hipSuccess && err == 0) { err = (int)st; fprintf(stderr, "[emg3d_hip] launch failed: %s\n", hipGetErrorString(st)); }
    }

    // --------------------------------------------------------------- levels
    // sizes and layouts that follow from nC alone (no device memory)
    static void shape_level(Level<T>& L) {
        L.nE = n_edges(L.nC);
        L.nCells = L.nC[0] * L.nC[1] * L.nC[2];
        L.fl = ref_field_layout(L.nC);
        L.cl = ref_cell_layout(L.nC);
        L.flT = L.fl;
        for (int c = 0; c < 3; ++c) {
            const i64 d0 = (c == 0) ? L.nC[0] : L.nC[0] + 1, d1 = (c == 1) ? L.nC[1] : L.nC[1] + 1;
            L.flT.st[c][0] = d1; L.flT.st[c][1] = 1; L.flT.st[c][2] = d0 * d1;
        }
        L.clT.st[0] = L.nC[1]; L.clT.st[1] = 1; L.clT.st[2] = L.nC[0] * L.nC[1];
    }
    std::shared_ptr<Level<T>> make_level(const std::vector<double> hh[3]) {
        auto L = std::make_shared<Level<T>>();
        for (int a = 0; a < 3; ++a) {
            L->nC[a] = (i64)hh[a].size();
            L->h_host[a] = hh[a];
            // nodes = r_[0, cumsum(h)] + origin ; centers (meshes.py:84-97)
            L->nodes[a].resize(hh[a].size() + 1);
            double cs = 0.0;
            L->nodes[a][0] = 0.0 + origin[a];
            for (size_t i = 0; i < hh[a].size(); ++i) { cs += hh[a][i]; L->nodes[a][i + 1] = cs + origin[a]; }
            L->centers[a].resize(hh[a].size());
            for (size_t i = 0; i < hh[a].size(); ++i) L->centers[a][i] = (L->nodes[a][i + 1] + L->nodes[a][i]) / 2;
            L->h[a] = upload<double>(hh[a].data(), (i64)hh[a].size());
            std::vector<double> inv(hh[a].size());
            for (size_t i = 0; i < hh[a].size(); ++i) inv[i] = 1.0 / hh[a][i];
            L->ih[a] = upload<double>(inv.data(), (i64)inv.size());
        }
        shape_level(*L);
        L->s = dalloc<T>(nsys * L->nE);
        L->e = dalloc<T>(nsys * L->nE);
        L->r = dalloc<T>(nsys * L->nE);
        return L;
    }

    // Build the transfer operators + child model of `L` for current sc_dir `sc`.
    std::shared_ptr<Level<T>> make_child(Level<T>& L, Transfer& X, int sc) {
        X.sc = sc;
        sc_axes(sc, X.co);
        std::vector<double> ch[3];
        for (int a = 0; a < 3; ++a) {
            if (X.co[a]) {   // ch = diff(nodes[::2]), solver.py:859-861
                const i64 n = L.nC[a] / 2;
                ch[a].resize(n);
                for (i64 i = 0; i < n; ++i) ch[a][i] = L.nodes[a][2 * i + 2] - L.nodes[a][2 * i];
            } else {
                // np.diff(nodes[::1])
                ch[a].resize(L.nC[a]);
                for (i64 i = 0; i < L.nC[a]; ++i) ch[a][i] = L.nodes[a][i + 1] - L.nodes[a][i];
            }
        }
        auto C = make_level(ch);
        // model (solver.py:874-884), aliasing preserved
        const int blocks = (int)((C->nCells + EMG_BLOCK - 1) / EMG_BLOCK);
        C->eta[0] = dalloc<T>(C->nCells);
        MG_LAUNCH(k_restrict_model<T>, dim3(blocks), dim3(EMG_BLOCK), 0, stream, C->eta[0],
                           (const T*)L.eta[0], C->nC[0], C->nC[1], C->nC[2], L.nC[0], L.nC[1], X.co[0], X.co[1], X.co[2]);
        for (int c = 1; c < 3; ++c) {
            if (eta_alias[c]) { C->eta[c] = C->eta[0]; continue; }
            C->eta[c] = dalloc<T>(C->nCells);
            MG_LAUNCH(k_restrict_model<T>, dim3(blocks), dim3(EMG_BLOCK), 0, stream, C->eta[c],
                               (const T*)L.eta[c], C->nC[0], C->nC[1], C->nC[2], L.nC[0], L.nC[1], X.co[0], X.co[1], X.co[2]);
        }
        C->zeta = dalloc<double>(C->nCells);
        MG_LAUNCH(k_restrict_model<double>, dim3(blocks), dim3(EMG_BLOCK), 0, stream, C->zeta,
                           (const double*)L.zeta, C->nC[0], C->nC[1], C->nC[2], L.nC[0], L.nC[1], X.co[0], X.co[1], X.co[2]);
        check_launch();
        // restriction weights (solver.py:1787-1838) and prolongation weights
        for (int a = 0; a < 3; ++a) {
            if (X.co[a]) {
                const i64 n = C->nC[a] + 1;
                std::vector<double> wl(n), w0(n), wr(n);
                restrict_weights_host(L.nodes[a].data(), L.centers[a].data(), L.h_host[a].data(), L.nC[a],
                                      C->nodes[a].data(), C->centers[a].data(), C->h_host[a].data(), n,
                                      wl.data(), w0.data(), wr.data());
                X.w[a][0] = upload<double>(wl.data(), n);
                X.w[a][1] = upload<double>(w0.data(), n);
                X.w[a][2] = upload<double>(wr.data(), n);
            }
            std::vector<int> idx; std::vector<double> wt;
            prolong_weights_host(C->nodes[a], L.nodes[a], idx, wt);
            X.pidx[a] = upload<int>(idx.data(), (i64)idx.size());
            X.pwt[a] = upload<double>(wt.data(), (i64)wt.size());
        }
        return C;
    }

    // ---- another frequency on the same handle (handles created from sigma*V, emg3d_mg_create_sv) ----
    // eta = s mu_0 sigma V changes with the frequency, nothing else does: grids, transfer weights, work buffers and the
    // captured launch graphs (they hold pointers, not values) stay.  Recomputed with the kernels and in the order of a
    // fresh handle, so the results are those of a fresh handle bit for bit: level-0 eta, the coarse models of every
    // hierarchy built so far, transposed model copies, every cached line factorisation.
    double* sv[3] = {nullptr, nullptr, nullptr};
    double* volw = nullptr;        // != nullptr: sv[] holds the conductivities, eta = (b V) sigma (k_eta_vs: VolumeModel's rounding)
    double* epsr = nullptr;        // != nullptr (with volw): relative permittivities, eta = (b V) (sigma - c eps_r) (k_eta_vs_eps)
    double seps0 = 0.0;            // c = s eps_0 (Laplace domain) resp. Im(s) eps_0 (frequency domain) of the current frequency
    static double imag_or_real(double x) { return x; }
    static double imag_or_real(c128 x) { return x.im; }
    T smu0_now = T();              // the s mu_0 the level-0 eta was last formed with (form_eta): where the handle stands
    void form_eta(Level<T>& L0, T smu0) {
        smu0_now = smu0;
        const unsigned blocks = (unsigned)std::min<i64>((L0.nCells + EMG_BLOCK - 1) / EMG_BLOCK, 4096);
        for (int c = 0; c < 3; ++c) {
            if (c > 0 && eta_alias[c]) continue;
            if (volw && epsr)
                MG_LAUNCH(k_eta_vs_eps<T>, dim3(blocks), dim3(EMG_BLOCK), 0, stream, L0.eta[c], (const double*)volw,
                                   (const double*)sv[c], (const double*)epsr, imag_or_real(smu0), seps0, L0.nCells);
            else if (volw)
                MG_LAUNCH(k_eta_vs<T>, dim3(blocks), dim3(EMG_BLOCK), 0, stream, L0.eta[c], (const double*)volw,
                                   (const double*)sv[c], imag_or_real(smu0), L0.nCells);
            else
                MG_LAUNCH(k_scale_real_to<T>, dim3(blocks), dim3(EMG_BLOCK), 0, stream, L0.eta[c], (const double*)sv[c], smu0, L0.nCells);
        }
    }
    void restrict_eta(Level<T>& L, const Transfer& X, Level<T>& C) {
        const int blocks = (int)((C.nCells + EMG_BLOCK - 1) / EMG_BLOCK);
        for (int c = 0; c < 3; ++c) {
            if (c > 0 && eta_alias[c]) continue;
            MG_LAUNCH(k_restrict_model<T>, dim3(blocks), dim3(EMG_BLOCK), 0, stream, C.eta[c],
                               (const T*)L.eta[c], C.nC[0], C.nC[1], C.nC[2], L.nC[0], L.nC[1], X.co[0], X.co[1], X.co[2]);
        }
    }
    int set_smu0(T smu0) {
        if (!sv[0]) return -7;
        refresh_model(smu0);
        return 0;
    }
    // sigma = backward(p) of property map `map` (k_sigma_of_map) from the device array `p` into `out`, which may be `p`
    void sigma_of_map(double* out, const double* p, int map, i64 n) {
        if (map == 0 && out == p) return;
        MG_LAUNCH(k_sigma_of_map, dim3((unsigned)std::min<i64>((n + EMG_BLOCK - 1) / EMG_BLOCK, 4096)), dim3(EMG_BLOCK), 0, stream,
                  out, p, map, n);
    }
    // ---- another model on the same handle (handles that keep sigma and V apart: emg3d_mg_create_vs / _vse) ----
    // The property arrays of a model on the same grid, in the same anisotropy case, go into the sv[] the handle has; then
    // everything that depends on sigma is recomputed as for another frequency, at the frequency the handle stands at.  No buffer
    // moves: launch graphs, placement, workspace vectors and accumulators stay.  A failed upload may leave sv[] half
    // written: the handle is then broken.
    int set_model(int map, const double* px, const double* py, const double* pz) {
        if (!sv[0] || !volw) return -7;
        if (map < 0 || map >= EMG_MAP_CODES || !px) return -2;
        const double* p[3] = {px, py, pz};
        for (int c = 1; c < 3; ++c)
            if ((p[c] == nullptr || p[c] == px) != eta_alias[c]) return -2;
        const i64 nC = lv0->nCells;
        for (int c = 0; c < 3; ++c) {
            if (c > 0 && eta_alias[c]) continue;
            const hipError_t st = h2d(sv[c], p[c], (size_t)nC * sizeof(double));
            if (st != hipSuccess) { (void)hipGetLastError(); err = (int)st; broken = true; return (int)st; }
            sigma_of_map(sv[c], sv[c], map, nC);
        }
        refresh_model(smu0_now);
        return 0;
    }
    void refresh_model(T smu0) {
        Level<T>& L0 = *lv0;
        form_eta(L0, smu0);
        for (auto& kv : hier) {
            Hierarchy<T>& H = kv.second;
            for (size_t l = 0; l + 1 < H.lv.size(); ++l) restrict_eta(*H.lv[l], H.tr[l], *H.lv[l + 1]);
        }
        std::vector<Level<T>*> seen;
        auto refresh = [&](Level<T>& L) {
            for (auto* p : seen) if (p == &L) return;
            seen.push_back(&L);
            if (L.zetaT) {
                transpose_xy(L.etaT[0], (const T*)L.eta[0], L.nC[0], L.nC[1], L.nC[2], true, 0);
                for (int c = 1; c < 3; ++c)
                    if (L.eta[c] != L.eta[0]) transpose_xy(L.etaT[c], (const T*)L.eta[c], L.nC[0], L.nC[1], L.nC[2], true, 0);
            }
            for (int d = 0; d < 3; ++d) if (L.fac[d]) { compute_factor(L, d); fill_scantab(L, d); }
        };
        refresh(L0);
        for (auto& kv : hier) for (auto& l : kv.second.lv) if (l) refresh(*l);
        check_launch();
    }

    // Level 0 of a model without magnetic permeabilities: zeta is the cell volume (hx hy) hz.  Checked bit for bit on the
    // device; the level-0 sweep kernels then form zeta from the width vectors instead of reading it (smooth_qc.hpp).
    void check_zeta() {
        Level<T>& L = *lv0;
        int* flag = dalloc<int>(1);
        if (!flag) return;
        hipMemsetAsync(flag, 0, sizeof(int), stream);
        MG_LAUNCH(k_zeta_is_volume, dim3((unsigned)std::min<i64>((L.nCells + EMG_BLOCK - 1) / EMG_BLOCK, 4096)), dim3(EMG_BLOCK),
                           0, stream, (const double*)L.zeta, (const double*)L.h[0], (const double*)L.h[1], (const double*)L.h[2],
                           L.nC[0], L.nC[1], L.nC[2], flag);
        int host = 1;
        if (hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) { (void)hipGetLastError(); host = 1; }
        L.zeta_sep = (host == 0);
    }

    // Hierarchy for global sc_dir g: levels 0..clevel[g] (solver.py:480, 524, 551).
    Hierarchy<T>& hierarchy(int g) {
        auto it = hier.find(g);
        if (it != hier.end()) return it->second;
        Hierarchy<T> H;
        H.lv.push_back(lv0);              // level 0 (arrays + caches) is shared by all hierarchies
        for (int lev = 0; lev < clevel[g]; ++lev) {
            Level<T>& L = *H.lv.back();
            const int sc = current_sc_dir(g, L.nC);
            H.tr.emplace_back();
            H.lv.push_back(make_child(L, H.tr.back(), sc));
        }
        hier[g] = H;
        return hier[g];
    }

    // ------------------------------------------- Krylov vector workspace
    // nE-sized device vectors addressed by index; -1 = level-0 source s, -2 = level-0 field e.
    std::vector<T*> vecs;
    double* dot_partials = nullptr;
    double* dot_out = nullptr;
    static const int DOT_BLOCKS = 1024;
    int vec_alloc(int n) {
        while ((int)vecs.size() < n) {
            T* v = try_alloc<T>(lv0->nE);       // (optional memory: the caller falls back to the host iteration; the handle stays usable)
            if (!v) return (int)hipErrorOutOfMemory;                   // (nothing pushed: vec() keeps answering nullptr)
            hipMemsetAsync(v, 0, (size_t)lv0->nE * sizeof(T), stream);
            vecs.push_back(v);
        }
        if (!dot_partials) { dot_partials = dalloc<double>(2 * DOT_BLOCKS); dot_out = dalloc<double>(2); }
        return broken ? (int)hipErrorOutOfMemory : err;
    }
    T* vec(int id) {
        if (id == -1) return sel_s();
        if (id == -2) return sel_e();
        if (id < 0 || id >= (int)vecs.size()) return nullptr;
        return vecs[id];
    }
    unsigned vec_grid() const { return (unsigned)std::min<i64>((lv0->nE + EMG_BLOCK - 1) / EMG_BLOCK, 4096); }
    void touched(int id) {      // the level-0 source changed: its working copies are stale
        if (id == -1) { source_changed(); lv0->s_dense = true; }      // a dense vector: no point in scanning it for zeros
    }
    int vec_copy(int dst, int src) {
        T *d = vec(dst), *s_ = vec(src);
        if (!d || !s_) return -2;
        if (d != s_) hipMemcpyAsync(d, s_, (size_t)lv0->nE * sizeof(T), hipMemcpyDeviceToDevice, stream);
        touched(dst);
        return 0;
    }
    int vec_axpy(int y, T alpha, int x) {
        T *py = vec(y), *px = vec(x);
        if (!py || !px || py == px) return -2;
        MG_LAUNCH(k_axpy<T>, dim3(vec_grid()), dim3(EMG_BLOCK), 0, stream, py, (const T*)px, alpha, lv0->nE);
        touched(y);
        return 0;
    }
    int vec_scale(int y, T alpha) {
        T* py = vec(y);
        if (!py) return -2;
        MG_LAUNCH(k_scale<T>, dim3(vec_grid()), dim3(EMG_BLOCK), 0, stream, py, alpha, lv0->nE);
        touched(y);
        return 0;
    }
    int vec_dot(int a, int b, double out[2]) {     // <a, b> with a conjugated
        T *pa = vec(a), *pb = vec(b);
        if (!pa || !pb || !dot_partials) return -2;
        MG_LAUNCH(k_dot_partials<T>, dim3(DOT_BLOCKS), dim3(EMG_BLOCK), 0, stream, (const T*)pa, (const T*)pb,
                           lv0->nE, dot_partials);
        MG_LAUNCH(k_sum_pairs, dim3(1), dim3(EMG_BLOCK), 0, stream, (const double*)dot_partials, (i64)DOT_BLOCKS, dot_out);
        hipError_t st = hipMemcpyAsync(out, dot_out, 2 * sizeof(double), hipMemcpyDeviceToHost, stream);
        if (st == hipSuccess) st = hipStreamSynchronize(stream);
        return st == hipSuccess ? 0 : (int)st;
    }
    // dst = A src  (A = the system matrix; reference amatvec, solver.py:646-660)
    int vec_amatvec(int dst, int src) {
        T *pd = vec(dst), *ps = vec(src);
        if (!pd || !ps || pd == ps) return -2;
        Level<T>& L = *lv0;
        hipMemsetAsync(pd, 0, (size_t)L.nE * sizeof(T), stream);
        ResidualArgs<T> a;
        for (int q = 0; q < 3; ++q) { a.nC[q] = L.nC[q]; a.eta[q] = L.eta[q]; a.h[q] = L.h[q]; a.ih[q] = L.ih[q]; }
        a.fl = L.fl; a.r = pd; a.s = pd; a.e = ps; a.zeta = L.zeta; a.partials = nullptr; a.bt = Batch();
        const i64 plane = (L.nC[0] + 1) * (L.nC[1] + 1);
        dim3 grid((unsigned)((plane + EMG_BLOCK - 1) / EMG_BLOCK), (unsigned)(L.nC[2] + 1));
        if (!broken) residual_launch<T>(0, 1, grid, stream, a);   // pd = 0 - A ps
        MG_LAUNCH(k_negate<T>, dim3(vec_grid()), dim3(EMG_BLOCK), 0, stream, pd, L.nE);
        touched(dst);
        check_launch();
        return err;
    }

    // ------------------------------------------- batched Krylov vector workspace (emg3d_mg_bvec_*)
    // Beside the single-system workspace above (whose vectors stay nE-sized and address the SELECTED system): vectors
    // [nsys][nE] addressed by index, -1 = the whole level-0 source array, -2 = the whole level-0 field array.  Every
    // primitive acts on the systems that are not frozen (set_mask) and gives each of them bit for bit what the
    // single-system primitive gives on that system's vectors: same kernels' bodies, per system the same launch geometry.
    std::vector<T*> bvecs;
    double* bdot_partials = nullptr;    // [nsys][2 DOT_BLOCKS]
    double* bdot_out = nullptr;         // [nsys][2]
    std::vector<double> bdot_host;
    std::vector<int> hmask;             // host mirror of bmask (empty: every system is active)
    bool sys_on(int b) const { return hmask.empty() || hmask[(size_t)b] != 0; }
    int bvec_alloc(int n) {
        while ((int)bvecs.size() < n) {
            T* v = try_alloc<T>((i64)nsys * lv0->nE);      // (optional memory, as vec_alloc: the handle stays usable)
            if (!v) return (int)hipErrorOutOfMemory;
            hipMemsetAsync(v, 0, (size_t)nsys * (size_t)lv0->nE * sizeof(T), stream);
            bvecs.push_back(v);
        }
        if (!bdot_partials) {
            bdot_partials = dalloc<double>((i64)nsys * 2 * DOT_BLOCKS); bdot_out = dalloc<double>(2 * (i64)nsys);
            bdot_host.assign((size_t)(2 * nsys), 0.0);
        }
        return broken ? (int)hipErrorOutOfMemory : err;
    }
    T* bvec(int id) {
        if (id == -1) return lv0->s;
        if (id == -2) { e_to_ref(*lv0); return lv0->e; }
        if (id < 0 || id >= (int)bvecs.size()) return nullptr;
        return bvecs[(size_t)id];
    }
    // fn(first, count) for every run of consecutive active systems
    template <class F>
    void active_runs(F fn) {
        for (int b = 0; b < nsys;) {
            if (!sys_on(b)) { ++b; continue; }
            int e = b;
            while (e < nsys && sys_on(e)) ++e;
            fn(b, e - b);
            b = e;
        }
    }
    int bvec_copy(int dst, int src) {
        T *d = bvec(dst), *s_ = bvec(src);
        if (!d || !s_) return -2;
        const i64 nE = lv0->nE;
        if (d != s_) active_runs([&](int b, int k) {
            hipMemcpyAsync(d + (i64)b * nE, s_ + (i64)b * nE, (size_t)k * (size_t)nE * sizeof(T), hipMemcpyDeviceToDevice, stream);
        });
        touched(dst);
        return 0;
    }
    int bvec_zero(int id) {
        // the whole field array is overwritten: whatever layout it was in needs no conversion (as emg3d_mg_set_efield)
        bool all_on = true;
        for (int b = 0; b < nsys; ++b) all_on = all_on && sys_on(b);
        if (id == -2 && all_on) lv0->e_home = 0;
        T* d = bvec(id);
        if (!d) return -2;
        const i64 nE = lv0->nE;
        active_runs([&](int b, int k) { hipMemsetAsync(d + (i64)b * nE, 0, (size_t)k * (size_t)nE * sizeof(T), stream); });
        touched(id);
        return 0;
    }
    int bvec_axpy(int y, const BatchCoef<T>& alpha, int x) {
        T *py = bvec(y), *px = bvec(x);
        if (!py || !px || py == px) return -2;
        MG_LAUNCH(k_axpy_b<T>, bgrid_y(vec_grid()), dim3(EMG_BLOCK), 0, stream, py, (const T*)px, alpha, lv0->nE, batch(*lv0));
        touched(y);
        return 0;
    }
    int bvec_scale(int y, const BatchCoef<T>& alpha) {
        T* py = bvec(y);
        if (!py) return -2;
        MG_LAUNCH(k_scale_b<T>, bgrid_y(vec_grid()), dim3(EMG_BLOCK), 0, stream, py, alpha, lv0->nE, batch(*lv0));
        touched(y);
        return 0;
    }
    int bvec_dot(int a, int b, double* out) {       // out[2 b], out[2 b + 1] = <a_b, b_b>, a conjugated; frozen systems: untouched
        T *pa = bvec(a), *pb = bvec(b);
        if (!pa || !pb || !bdot_partials) return -2;
        const Batch bt = batch(*lv0);
        MG_LAUNCH(k_dot_partials_b<T>, bgrid_y(DOT_BLOCKS), dim3(EMG_BLOCK), 0, stream, (const T*)pa, (const T*)pb, lv0->nE,
                  bdot_partials, bt);
        MG_LAUNCH(k_sum_pairs_b, bgrid_y(1), dim3(EMG_BLOCK), 0, stream, (const double*)bdot_partials, (i64)DOT_BLOCKS, bdot_out, bt);
        hipError_t st = hipMemcpyAsync(bdot_host.data(), bdot_out, (size_t)(2 * nsys) * sizeof(double), hipMemcpyDeviceToHost, stream);
        if (st == hipSuccess) st = hipStreamSynchronize(stream);
        if (st != hipSuccess) return (int)st;
        for (int s_ = 0; s_ < nsys; ++s_)
            if (sys_on(s_)) { out[2 * s_] = bdot_host[(size_t)(2 * s_)]; out[2 * s_ + 1] = bdot_host[(size_t)(2 * s_ + 1)]; }
        return 0;
    }
    // dst_b = A src_b: the residual launch of vec_amatvec over all systems, then the negate
    int bvec_amatvec(int dst, int src) {
        T *pd = bvec(dst), *ps = bvec(src);
        if (!pd || !ps || pd == ps) return -2;
        Level<T>& L = *lv0;
        active_runs([&](int b, int k) { hipMemsetAsync(pd + (i64)b * L.nE, 0, (size_t)k * (size_t)L.nE * sizeof(T), stream); });
        ResidualArgs<T> a;
        for (int q = 0; q < 3; ++q) { a.nC[q] = L.nC[q]; a.eta[q] = L.eta[q]; a.h[q] = L.h[q]; a.ih[q] = L.ih[q]; }
        a.fl = L.fl; a.r = pd; a.s = pd; a.e = ps; a.zeta = L.zeta; a.partials = nullptr; a.bt = batch(L);
        const i64 plane = (L.nC[0] + 1) * (L.nC[1] + 1);
        dim3 grid((unsigned)((plane + EMG_BLOCK - 1) / EMG_BLOCK), (unsigned)(L.nC[2] + 1), (unsigned)nsys);
        if (!broken) residual_launch<T>(0, 1, grid, stream, a);   // pd = 0 - A ps
        MG_LAUNCH(k_negate_b<T>, bgrid_y(vec_grid()), dim3(EMG_BLOCK), 0, stream, pd, L.nE, a.bt);
        touched(dst);
        check_launch();
        return err;
    }

    // ------------------------------------------- per-cell accumulators (emg3d_mg_grad_acc(3)_*, emg3d_mg_sens_acc_add)
    // Two blocks of the handle's own (not the residual buffer emg3d_mg_gradient stages in), indexed by `split`: cell_acc[0] = nC
    // doubles, the summed form; cell_acc[1] = 3 nC doubles [acc_x | acc_y | acc_z], the per-direction form (optimize.SurveyJacobian).
    // Independent of each other, each allocated on first use, counted in `bytes`, freed with the handle; cycles, set_smu0 and
    // set_mask do not touch them.
    double* cell_acc[2] = {nullptr, nullptr};
    int acc_reset(int split) {
        const i64 n = (split ? 3 : 1) * lv0->nCells;
        if (!cell_acc[split]) cell_acc[split] = dalloc<double>(n);
        if (!cell_acc[split]) return err ? err : (int)hipErrorOutOfMemory;
        hipMemsetAsync(cell_acc[split], 0, (size_t)n * sizeof(double), stream);
        return 0;
    }
    int acc_ready(int split) { return cell_acc[split] ? 0 : acc_reset(split); }         // first use: allocated and zero
    // what the per-cell kernels take as acc, acc1, acc2
    void acc_ptrs(int split, double* out[3]) const {
        out[0] = cell_acc[split];
        out[1] = split ? cell_acc[1] + lv0->nCells : nullptr;
        out[2] = split ? cell_acc[1] + 2 * lv0->nCells : nullptr;
    }
    unsigned long long use_bits(const int32_t* use) const {         // bit b = use[b] != 0, b = 0 .. nsys-1
        unsigned long long bits = 0;
        for (int b = 0; b < nsys; ++b) if (use[b]) bits |= 1ull << b;
        return bits;
    }
    // the forward fields of a batch: a saved copy, not the live field array (which holds the back-propagated fields); nullptr: no such
    const T* saved_bvec(int id) const { return (id < 0 || id >= (int)bvecs.size()) ? nullptr : bvecs[(size_t)id]; }
    // acc += g_b (split: acc_c += g_c,b, bit for bit emg3d_mg_gradient3's) for the systems with use[b] != 0, ascending b, in ONE
    // launch (k_gradient_acc): forward fields = batched vector `fwd_bvec`, back-propagated fields = the level-0 field array.
    int acc_add(int split, int fwd_bvec, double sr, double si, const int32_t* use) {
        const T* fwd = saved_bvec(fwd_bvec);
        if (!fwd) return -2;
        { const int st = acc_ready(split); if (st) return st; }
        double* a[3];
        acc_ptrs(split, a);
        e_to_ref(*lv0);
        MG_CELL_LAUNCH(*this, k_gradient_acc, split, a, fwd, (const T*)lv0->e, lv0->nE, nsys, use_bits(use), sr, si);
        check_launch();
        return err;
    }
    // Survey sensitivity diagonal (emg3d_mg_sens_acc_add, k_sens_acc): acc += W[b_r nsys + b_s] |row(b_r, b_s)|^2 over all pairs of an
    // adjoint system b_r (slice of the level-0 field array) and a forward system b_s (slice of batched vector `fwd_bvec`), into
    // cell_acc[split], in ONE launch.  The weight table is nsys x nsys doubles of the handle's own, allocated at the first call
    // (counted in `bytes`; nsys is fixed once a batched vector exists) and uploaded by every call.  -2: a bad vector, an accumulator
    // that was never reset, a non-finite weight.
    double* sens_w = nullptr;
    int sens_acc_add(int fwd_bvec, double sr, double si, const int32_t* use_fwd, const int32_t* use_adj, const double* weights, int split) {
        const T* fwd = saved_bvec(fwd_bvec);
        if (!fwd || !cell_acc[split]) return -2;
        const i64 nw = (i64)nsys * nsys;
        for (i64 q = 0; q < nw; ++q) if (!std::isfinite(weights[q])) return -2;
        if (!sens_w) sens_w = dalloc<double>(nw);
        if (!sens_w) return err ? err : (int)hipErrorOutOfMemory;
        const hipError_t st = h2d(sens_w, weights, (size_t)nw * sizeof(double));
        if (st != hipSuccess) return (int)st;
        double* a[3];
        acc_ptrs(split, a);
        e_to_ref(*lv0);
        MG_CELL_LAUNCH(*this, k_sens_acc, split, a, fwd, (const T*)lv0->e, lv0->nE, nsys, use_bits(use_fwd), use_bits(use_adj),
                       (const double*)sens_w, sr, si);
        check_launch();
        return err;
    }

    // ------------------------------------------- model grid (emg3d_mg_set_model_grid, _set_regrid_factors, _grad_acc(3)_get_model)
    // The model of an inversion lives on a coarser grid and reaches this one by volume averaging (regrid.hpp: A); the accumulators
    // go back to it as Q_c (.) A^T (F_c (.) acc_c), so that only nM-sized arrays cross PCIe.  The handle keeps the segment tables
    // of the three axes with both sets of offsets, the factors (F_c: nC doubles, Q_c: nM doubles per direction; directions given
    // with the pointer of direction x share its copy), nC doubles of scratch for t and 3 nM doubles for the results: all counted in
    // `bytes`, freed with the handle.  The tables are allocated for the most segments an axis can have, so that another model grid
    // of the same size (and other factors with the same sharing) replace the first in place: `bytes` stays.
    struct ModelGridLink {
        bool set = false, factors = false;
        i64 n[3] = {0, 0, 0}, nM = 0;
        double* w[3] = {nullptr, nullptr, nullptr};
        i64 *in[3] = {nullptr, nullptr, nullptr}, *out[3] = {nullptr, nullptr, nullptr}, *ptr[3] = {nullptr, nullptr, nullptr},
            *iptr[3] = {nullptr, nullptr, nullptr};
        double *F[3] = {nullptr, nullptr, nullptr}, *Q[3] = {nullptr, nullptr, nullptr};
        double *t = nullptr, *res = nullptr;
    } mgl;
    int set_model_grid(const i64 n[3], const double* const edges[3]) {
        Level<T>& L = *lv0;
        if (mgl.set && (n[0] != mgl.n[0] || n[1] != mgl.n[1] || n[2] != mgl.n[2])) return -2;
        const double* nodes[3] = {L.nodes[0].data(), L.nodes[1].data(), L.nodes[2].data()};
        VolAvgTables tb;
        tb.build(n, edges, L.nC, nodes);
        if (!mgl.set) {
            for (int a = 0; a < 3; ++a) {
                const i64 cap = n[a] + L.nC[a] + 1;
                mgl.w[a] = dalloc<double>(cap); mgl.in[a] = dalloc<i64>(cap); mgl.out[a] = dalloc<i64>(cap);
                mgl.ptr[a] = dalloc<i64>(L.nC[a] + 1); mgl.iptr[a] = dalloc<i64>(n[a] + 1);
                mgl.n[a] = n[a];
            }
            mgl.nM = n[0] * n[1] * n[2];
            mgl.t = dalloc<double>(L.nCells);
            mgl.res = dalloc<double>(3 * mgl.nM);
            if (broken) return err ? err : (int)hipErrorOutOfMemory;
            mgl.set = true;
        }
        for (int a = 0; a < 3; ++a) {
            hipError_t st = h2d(mgl.w[a], tb.w[a].data(), (size_t)tb.ns[a] * sizeof(double));
            if (st == hipSuccess) st = h2d(mgl.in[a], tb.in[a].data(), (size_t)tb.ns[a] * sizeof(i64));
            if (st == hipSuccess) st = h2d(mgl.out[a], tb.out[a].data(), (size_t)tb.ns[a] * sizeof(i64));
            if (st == hipSuccess) st = h2d(mgl.ptr[a], tb.ptr[a].data(), (size_t)(L.nC[a] + 1) * sizeof(i64));
            if (st == hipSuccess) st = h2d(mgl.iptr[a], tb.iptr[a].data(), (size_t)(n[a] + 1) * sizeof(i64));
            if (st != hipSuccess) { mgl.set = false; return (int)st; }      // (half-written tables are not used)
        }
        return 0;
    }
    int set_regrid_factors(const double* const F[3], const double* const Q[3]) {
        if (!mgl.set) return -7;
        if (!F[0] || !Q[0]) return -2;
        const bool have = mgl.F[0] != nullptr;          // (allocated by an earlier call, whether or not its uploads succeeded)
        for (int c = 1; c < 3; ++c) {
            if (!F[c] || !Q[c]) return -2;
            if (have && ((F[c] == F[0]) != (mgl.F[c] == mgl.F[0]) || (Q[c] == Q[0]) != (mgl.Q[c] == mgl.Q[0]))) return -2;
        }
        const i64 nC = lv0->nCells;
        if (!have) {
            for (int c = 0; c < 3; ++c) {
                mgl.F[c] = (c > 0 && F[c] == F[0]) ? mgl.F[0] : dalloc<double>(nC);
                mgl.Q[c] = (c > 0 && Q[c] == Q[0]) ? mgl.Q[0] : dalloc<double>(mgl.nM);
            }
            if (broken) return err ? err : (int)hipErrorOutOfMemory;
        }
        mgl.factors = false;
        for (int c = 0; c < 3; ++c) {
            hipError_t st = hipSuccess;
            if (c == 0 || mgl.F[c] != mgl.F[0]) st = h2d(mgl.F[c], F[c], (size_t)nC * sizeof(double));
            if (st == hipSuccess && (c == 0 || mgl.Q[c] != mgl.Q[0])) st = h2d(mgl.Q[c], Q[c], (size_t)mgl.nM * sizeof(double));
            if (st != hipSuccess) return (int)st;
        }
        mgl.factors = true;
        return 0;
    }
    // res[k] = Q_k (.) A^T (F_k (.) acc[k]) for the ndir = 1 (split: 3) accumulators of cell_acc[split], which are left as they are
    int regrid_acc(int split) {
        if (!mgl.set || !mgl.factors) return -7;
        Level<T>& L = *lv0;
        const double* acc = cell_acc[split];
        const int ndir = split ? 3 : 1;
        VolAvgAdjAxes ax;
        for (int a = 0; a < 3; ++a) { ax.iptr[a] = mgl.iptr[a]; ax.out[a] = mgl.out[a]; ax.w[a] = mgl.w[a]; }
        for (int k = 0; k < ndir && !broken; ++k)
            volume_average_adjoint_launch(stream, mgl.res + k * mgl.nM, mgl.t, acc + k * L.nCells, mgl.F[k], mgl.Q[k], nullptr,
                                          (const double*)L.h[0], (const double*)L.h[1], (const double*)L.h[2], mgl.n, L.nC, ax);
        check_launch();
        return err;
    }

    // ------------------------------------------- explicit rows of J (emg3d_mg_sens_rows, k_sens_rows)
    // Two buffers of doubles of the handle's own: row_buf[0] = [pairs][dir][part][nC], what the kernel writes; row_buf[1] =
    // [pairs][dir][part][nM], the same planes on the model grid.  Optional memory (quiet, as try_alloc and the batched vectors): each
    // grows to the largest call so far -- the old block is given back first (its contents are never needed again) --, is counted in
    // `bytes` and freed with the handle; a buffer that does not fit answers hipErrorOutOfMemory and leaves the handle usable (with
    // no buffer of that kind).  ALWAYS A BLOCK OF ITS OWN (raw_alloc), whatever its size, never a piece of an arena chunk: release()
    // gives back whole blocks only, and the first piece of a chunk has the chunk's address -- releasing it would free the chunk
    // under every piece carved after it.
    double* row_buf[2] = {nullptr, nullptr};
    i64 row_cap[2] = {0, 0};
    double* row_ensure(int which, i64 n) {
        if (row_cap[which] >= n) return row_buf[which];
        if (row_buf[which]) {
            hipStreamSynchronize(stream);
            release(row_buf[which]);                // (its `allocs` entry is this block alone, with the size counted below)
            row_buf[which] = nullptr; row_cap[which] = 0;
        }
        const size_t nb = (((size_t)std::max<i64>(n, 1) * sizeof(double)) + 255) & ~(size_t)255;
        alloc_quiet = true;
        row_buf[which] = (double*)raw_alloc(nb);
        alloc_quiet = false;
        if (row_buf[which]) { row_cap[which] = n; bytes += (i64)nb; }
        return row_buf[which];
    }
    static i64 bit_count(unsigned long long v) { i64 n = 0; for (; v; v &= v - 1ull) ++n; return n; }
    // out (host) <- the rows of all pairs (adjoint system of use_adj, forward system of use_fwd) in k_sens_rows's order, planes
    // [p][dir][part][cells]: ONE launch into row_buf[0]; on_model: every plane through volume_average_adjoint_launch with the
    // factors of its direction (one plane after the other through the scratch mgl.t) into row_buf[1]; then ONE copy to the host.
    // The summed form on the model grid is Q_x (.) A^T (F_x (.) (c_x + c_y + c_z)): right only if the three directions share
    // their factors, -2 otherwise.  -2 too: a bad fwd_bvec (a saved copy, as sens_acc_add), an empty mask.  -7: on_model without
    // model grid or factors.
    int sens_rows(int fwd_bvec, double sr, double si, const int32_t* use_fwd, const int32_t* use_adj, int split, int on_model, double* out) {
        SensRowsOnDevice d;
        const int rc = sens_rows_device(fwd_bvec, sr, si, use_fwd, use_adj, split, on_model, d);
        if (rc) return rc;
        const hipError_t st = d2h(out, d.planes, (size_t)(d.pairs * d.ndir * d.npart * d.ncells) * sizeof(double));
        return st == hipSuccess ? 0 : (int)st;
    }
    // The same rows, parked in a row store instead of copied to the host (emg3d_mg_sens_rows_park, csrc/rows.hpp: rows_park): plane
    // part = 0 of pair p into store row dest[p], on this handle's stream; the caller synchronises it.
    int sens_rows_park(int fwd_bvec, double sr, double si, const int32_t* use_fwd, const int32_t* use_adj, int split, int on_model,
                       emg3d_rows* rows, const int32_t* dest, int chain, int sum3) {
        SensRowsOnDevice d;
        const int rc = sens_rows_device(fwd_bvec, sr, si, use_fwd, use_adj, split, on_model, d);
        if (rc) return rc;
        return rows_park(rows, stream, device, d.planes, d.pairs, (int)d.ndir, (int)d.npart, d.ncells, dest, chain, sum3);
    }
    // Both parts of the same rows into a row store (emg3d_mg_sens_rows_fill): the real part of pair p into store row dest_re[p], the
    // imaginary part into dest_im[p] (nullptr: none; a real handle has none).  On the computational grid ONE launch of
    // k_sens_rows_fill (csrc/rows.hpp: rows_fill) from the fields into the store: no row buffer is allocated or grown, `bytes` stays.
    // On the model grid the planes of both parts lie in row_buf[1] after sens_rows_device, and rows_park runs once per part -- part
    // 1 is the same planes offset by ncells.  The checks of sens_rows_park, and those of rows_fill_check before anything is launched.
    int sens_rows_fill(int fwd_bvec, double sr, double si, const int32_t* use_fwd, const int32_t* use_adj, int split, int on_model,
                       emg3d_rows* rows, const int32_t* dest_re, const int32_t* dest_im, int chain, int sum3) {
        const T* fwd = saved_bvec(fwd_bvec);
        const unsigned long long uf = use_bits(use_fwd), ua = use_bits(use_adj);
        if (!fwd || !uf || !ua) return -2;
        if (on_model && (!mgl.set || !mgl.factors)) return -7;
        Level<T>& L = *lv0;
        const int ndir = split ? 3 : 1, npart = (int)(sizeof(T) / sizeof(double));
        {
            const int rc = rows_fill_check(rows, device, bit_count(uf) * bit_count(ua), ndir, npart, on_model ? mgl.nM : L.nCells, dest_re,
                                           dest_im, chain, sum3);
            if (rc) return rc;
        }
        if (on_model) {
            SensRowsOnDevice d;
            int rc = sens_rows_device(fwd_bvec, sr, si, use_fwd, use_adj, split, on_model, d);
            if (rc) return rc;
            rc = rows_park(rows, stream, device, d.planes, d.pairs, (int)d.ndir, (int)d.npart, d.ncells, dest_re, chain, sum3);
            if (rc || !dest_im) return rc;
            return rows_park(rows, stream, device, d.planes + d.ncells, d.pairs, (int)d.ndir, (int)d.npart, d.ncells, dest_im, chain, sum3);
        }
        e_to_ref(L);
        if (broken) return err ? err : (int)hipErrorOutOfMemory;
        RowsFillFields<T> f;
        for (int a = 0; a < 3; ++a) { f.nC[a] = L.nC[a]; f.h[a] = (const double*)L.h[a]; }
        f.fl = L.fl; f.fwd = fwd; f.adj = (const T*)L.e; f.nE = L.nE; f.nsys = nsys; f.use_fwd = uf; f.use_adj = ua; f.sr = sr; f.si = si;
        return rows_fill<T>(rows, stream, device, f, split, dest_re, dest_im, chain, sum3);
    }
    // what both share: the checks, the launches, and where the planes [p][dir][part][ncells] lie afterwards
    struct SensRowsOnDevice { const double* planes = nullptr; i64 pairs = 0, ndir = 0, npart = 0, ncells = 0; };
    int sens_rows_device(int fwd_bvec, double sr, double si, const int32_t* use_fwd, const int32_t* use_adj, int split, int on_model,
                         SensRowsOnDevice& res) {
        const T* fwd = saved_bvec(fwd_bvec);
        const unsigned long long uf = use_bits(use_fwd), ua = use_bits(use_adj);
        if (!fwd || !uf || !ua) return -2;
        if (on_model) {
            if (!mgl.set || !mgl.factors) return -7;
            if (!split && (mgl.F[1] != mgl.F[0] || mgl.F[2] != mgl.F[0] || mgl.Q[1] != mgl.Q[0] || mgl.Q[2] != mgl.Q[0])) return -2;
        }
        Level<T>& L = *lv0;
        const i64 ndir = split ? 3 : 1, npart = (i64)(sizeof(T) / sizeof(double));
        const i64 planes = bit_count(uf) * bit_count(ua) * ndir * npart;        // <= 64 * 64 * 6
        double* rb = row_ensure(0, planes * L.nCells);
        if (!rb) return broken ? err : (int)hipErrorOutOfMemory;
        double* mb = on_model ? row_ensure(1, planes * mgl.nM) : nullptr;
        if (on_model && !mb) return broken ? err : (int)hipErrorOutOfMemory;
        e_to_ref(L);
        double* a[3] = {rb, nullptr, nullptr};
        MG_CELL_LAUNCH(*this, k_sens_rows, split, a, fwd, (const T*)L.e, L.nE, nsys, uf, ua, sr, si);
        if (on_model) {
            VolAvgAdjAxes ax;
            for (int q = 0; q < 3; ++q) { ax.iptr[q] = mgl.iptr[q]; ax.out[q] = mgl.out[q]; ax.w[q] = mgl.w[q]; }
            for (i64 q = 0; q < planes && !broken; ++q) {
                const int k = (int)((q / npart) % ndir);
                volume_average_adjoint_launch(stream, mb + q * mgl.nM, mgl.t, rb + q * L.nCells, mgl.F[k], mgl.Q[k], nullptr,
                                              (const double*)L.h[0], (const double*)L.h[1], (const double*)L.h[2], mgl.n, L.nC, ax);
            }
        }
        check_launch();
        if (err) return err;
        res.planes = on_model ? mb : rb;
        res.pairs = planes / (ndir * npart); res.ndir = ndir; res.npart = npart; res.ncells = on_model ? mgl.nM : L.nCells;
        return 0;
    }

    // ------------------------------------------------------------ smoothers
    // ---- working copies: x<->y transpose and parity split ------------------
    // bt: the batch of a FIELD array (model arrays are shared by the systems: Batch())
    template <class U>
    void transpose_xy(U* dst, const U* src, i64 d0, i64 d1, i64 d2, bool to_T, int split, Batch bt = Batch()) {
        // src (d0 fastest, d1, d2) -> dst (d1 fastest, d0, d2) if to_T, else the inverse;
        // split: 1 = the d1-fastest side is parity-split, 2 = both sides are
        const i64 a0 = to_T ? d0 : d1, a1 = to_T ? d1 : d0;
        dim3 grid((unsigned)((a0 + 31) / 32), (unsigned)((a1 + 31) / 32), (unsigned)(d2 * (bt.st ? nsys : 1)));
        if (!split) MG_LAUNCH((k_transpose01<U, 0>), grid, dim3(32, 8), 0, stream, dst, src, a0, a1, (int)d2, bt);
        else if (split == 2) MG_LAUNCH((k_transpose01<U, 2>), grid, dim3(32, 8), 0, stream, dst, src, a0, a1, (int)d2, bt);
        else if (to_T) MG_LAUNCH((k_transpose01<U, 1>), grid, dim3(32, 8), 0, stream, dst, src, a0, a1, (int)d2, bt);
        else MG_LAUNCH((k_transpose01<U, -1>), grid, dim3(32, 8), 0, stream, dst, src, a0, a1, (int)d2, bt);
    }
    template <class U>
    void split_x(U* dst, const U* src, i64 d0, i64 rows, bool to_split, Batch bt = Batch()) {
        const i64 n = d0 * rows;
        const dim3 blocks((unsigned)std::min<i64>((n + EMG_BLOCK - 1) / EMG_BLOCK, 16384), bt.st ? nsys : 1);
        if (to_split) MG_LAUNCH((k_split0<U, 1>), blocks, dim3(EMG_BLOCK), 0, stream, dst, src, d0, rows, bt);
        else MG_LAUNCH((k_split0<U, -1>), blocks, dim3(EMG_BLOCK), 0, stream, dst, src, d0, rows, bt);
    }
    // ---- batched systems ------------------------------------------------------------------------------
    int nsys = 1;               // systems (right-hand sides) that run through every launch of the cycle
    int cur = 0;                // the system the single-field entry points (set/get field, source, receivers) address
    int* bmask = nullptr;       // device, nsys flags: 0 = frozen (nullptr: all active)
    // level-0 arrays of the selected system
    T* sel_s() { return lv0->s + (i64)cur * lv0->nE; }
    T* sel_e() { e_to_ref(*lv0); return lv0->e + (i64)cur * lv0->nE; }
    T* sel_r() { return lv0->r + (i64)cur * lv0->nE; }
    void source_changed() {
        lv0->sT_valid = false; lv0->sW_valid[0] = lv0->sW_valid[1] = false;
        lv0->sflag_valid[0] = lv0->sflag_valid[1] = lv0->sflag_valid[2] = false;
        lv0->s_dense = false;
    }
    // Source-free lines of level 0 (smooth_qc.hpp): flags per line direction, kept current like the source's working copies --
    // recomputed outside the captured graphs whenever the source has changed.  Batched systems: [system][line].
    int use_sflag = (int)LAB_ENV("EMG3D_SFLAG", 1);                     // lab: 0 = the sweeps always read the source
    bool sflag_on(const Level<T>& L, int dir) const {
        return use_sflag && &L == lv0.get() && order == 1 && L.fac[dir] && (L.fac_kind[dir] == 3 || L.fac_kind[dir] == 4);
    }
    void ensure_sflags(Level<T>& L, int dir) {
        if (!sflag_on(L, dir)) return;
        LineArgs<T> a;
        line_args(L, dir, a, false);
        if (!L.sflag[dir]) { L.sflag[dir] = dalloc<unsigned char>(a.nLinesTot * nsys); L.sflag_valid[dir] = false; }
        if (dry || L.sflag_valid[dir] || !L.sflag[dir]) return;
        const i64 nmax = a.nA[0] * a.nB2[0];
        if (L.s_dense) hipMemsetAsync(L.sflag[dir], 1, (size_t)(a.nLinesTot * nsys), stream);
        else if (nmax > 0)
            MG_LAUNCH(k_source_line_flags<T>, dim3((unsigned)((nmax + EMG_LINE_BLOCK - 1) / EMG_LINE_BLOCK), 4, (unsigned)nsys),
                               dim3(EMG_LINE_BLOCK), 0, stream, a, (const T*)L.s, L.fl, L.sflag[dir], L.nE);
        L.sflag_valid[dir] = true;
    }
    // Give a large allocation back (only whole hipMalloc blocks; arena pieces stay until the handle goes).
    void release(void* p) {
        for (size_t i = 0; i < allocs.size(); ++i)
            if (allocs[i].first == p) {
                bytes -= (i64)allocs[i].second;
                block_tag.erase(p);             // (given back untagged: a candidate that lost, an array of another shape)
                if (!DevicePool::get().give(device, p, allocs[i].second)) hipFree(p);
                allocs.erase(allocs.begin() + (long)i);
                return;
            }
    }
    // n systems per launch.  Only before the first cycle (no hierarchy, no captured graph yet): the level-0
    // arrays are re-allocated as [n][nE]; the model and everything derived from it is shared.
    int set_batch(int n) {
        if (n < 1 || n > 64) return -2;
        if (!hier.empty() || !graphs.empty() || lv0->eT || lv0->eW[0] || lv0->eW[1] || !vecs.empty() || !bvecs.empty()) return -6;
        if (n == nsys) return 0;
        Level<T>& L = *lv0;
        hipStreamSynchronize(stream);
        release(L.s); release(L.e); release(L.r);
        nsys = n; cur = 0;
        L.s = dalloc<T>(nsys * L.nE); L.e = dalloc<T>(nsys * L.nE); L.r = dalloc<T>(nsys * L.nE);
        if (!L.s || !L.e || !L.r) return err ? err : -3;
        hipMemsetAsync(L.s, 0, (size_t)(nsys * L.nE) * sizeof(T), stream);
        hipMemsetAsync(L.e, 0, (size_t)(nsys * L.nE) * sizeof(T), stream);
        hipMemsetAsync(L.r, 0, (size_t)(nsys * L.nE) * sizeof(T), stream);
        bmask = nullptr; n_partials = 0;
        hmask.clear();
        if (nsys > 1) {
            bmask = dalloc<int>(nsys);
            std::vector<int> ones((size_t)nsys, 1);
            hipMemcpyAsync(bmask, ones.data(), (size_t)nsys * sizeof(int), hipMemcpyHostToDevice, stream);
        }
        source_changed();
        hipError_t st = hipStreamSynchronize(stream);
        return st == hipSuccess ? 0 : (int)st;
    }
    int set_mask(const int* host) {
        if (nsys == 1) return 0;
        hmask.assign(host, host + nsys);
        hipError_t st = hipMemcpyAsync(bmask, host, (size_t)nsys * sizeof(int), hipMemcpyHostToDevice, stream);
        if (st == hipSuccess) st = hipStreamSynchronize(stream);
        source_changed();       // a system that was frozen while a working copy of the source was refreshed
        return st == hipSuccess ? 0 : (int)st;
    }
    Batch batch(const Level<T>& L) const { return Batch{nsys > 1 ? L.nE : 0, nsys > 1 ? bmask : nullptr, nsys}; }
    dim3 bgrid(unsigned g) const { return dim3(g * (unsigned)nsys, 1, 1); }      // line sweeps: EMG_SWEEP_WG
    dim3 bgrid_y(unsigned g) const { return dim3(g, (unsigned)nsys, 1); }
    // field: reference layout <-> working copy w (0: transposed + y-split, 1: x-split,
    // -1: plain transpose); w = 2: working copy 1 -> working copy 0 (to_work) or back.  all: frozen systems too.
    void convert_field(Level<T>& L, T* dst, const T* src, int w, bool to_work, bool all = false) {
        Batch bt = batch(L);
        if (all) bt.mask = nullptr;
        if (w == -1) {      // plain x<->y transposition: the three components in one launch
            FieldTransArgs t;
            i64 m0 = 0, m1 = 0;
            for (int c = 0; c < 3; ++c) {
                const i64 d0 = (c == 0) ? L.nC[0] : L.nC[0] + 1, d1 = (c == 1) ? L.nC[1] : L.nC[1] + 1,
                          d2 = (c == 2) ? L.nC[2] : L.nC[2] + 1;
                t.off[c] = L.fl.off[c]; t.a0[c] = to_work ? d0 : d1; t.a1[c] = to_work ? d1 : d0; t.nz[c] = (int)d2;
                m0 = std::max(m0, t.a0[c]); m1 = std::max(m1, t.a1[c]);
            }
            dim3 grid((unsigned)((m0 + 31) / 32), (unsigned)((m1 + 31) / 32), (unsigned)((t.nz[0] + t.nz[1] + t.nz[2]) * nsys));
            MG_LAUNCH((k_transpose01_field<T>), grid, dim3(32, 8), 0, stream, dst, src, t, bt);
            return;
        }
        for (int c = 0; c < 3; ++c) {
            const i64 d0 = (c == 0) ? L.nC[0] : L.nC[0] + 1, d1 = (c == 1) ? L.nC[1] : L.nC[1] + 1,
                      d2 = (c == 2) ? L.nC[2] : L.nC[2] + 1;
            if (w == 1) split_x(dst + L.fl.off[c], src + L.fl.off[c], d0, d1 * d2, to_work, bt);
            else transpose_xy(dst + L.fl.off[c], src + L.fl.off[c], d0, d1, d2, to_work, w == 2 ? 2 : 1, bt);
        }
    }
    void ensure_transposed_model(Level<T>& L) {
        if (L.zetaT) return;
        L.eT = dalloc<T>(nsys * L.nE); L.sT = dalloc<T>(nsys * L.nE);
        L.etaT[0] = dalloc<T>(L.nCells);
        transpose_xy(L.etaT[0], (const T*)L.eta[0], L.nC[0], L.nC[1], L.nC[2], true, 0);
        for (int c = 1; c < 3; ++c) {
            if (L.eta[c] == L.eta[0]) { L.etaT[c] = L.etaT[0]; continue; }
            L.etaT[c] = dalloc<T>(L.nCells);
            transpose_xy(L.etaT[c], (const T*)L.eta[c], L.nC[0], L.nC[1], L.nC[2], true, 0);
        }
        L.zetaT = dalloc<double>(L.nCells);
        transpose_xy(L.zetaT, (const double*)L.zeta, L.nC[0], L.nC[1], L.nC[2], true, 0);
        L.sT_valid = false;
    }
    void ensure_work(Level<T>& L, int w) {
        if (L.eW[w]) return;
        if (&L == lv0.get() && place_applies(L) && !placed[w]) {
            // a block that an earlier handle of this process searched for this role (DevicePool tags): no second search
            want_tag = 1 + w;
            L.eW[w] = dalloc<T>(nsys * L.nE);
            want_tag = 0;
            if (L.eW[w] && got_tag) { placed[w] = true; block_tag[L.eW[w]] = 1 + w; place_rec[w] = PlaceRec(); place_rec[w].reused = 1; }
        } else
        L.eW[w] = dalloc<T>(nsys * L.nE);
        L.sW[w] = dalloc<T>(nsys * L.nE);
        L.zetaW[w] = dalloc<double>(L.nCells);
        if (w == 1) split_x(L.zetaW[w], (const double*)L.zeta, L.nC[0], L.nC[1] * L.nC[2], true);
        else transpose_xy(L.zetaW[w], (const double*)L.zeta, L.nC[0], L.nC[1], L.nC[2], true, 1);
        L.sW_valid[w] = false;
    }
    bool split_on(Level<T>& L) { return plan(L, 0).split; }     // (a property of the level: the same for every direction)
    // Level 0 with split working copies: the field STAYS in the x-split copy eW[1] between the sweeps -- the residual and
    // the prolongation address it there (ResidualArgs::xs, ProlongArgs::fxs), the x-line sweeps convert eW[1] <-> eW[0]
    // -- and returns to the reference layout only when something outside the cycle asks for it (sel_e).  Saves the
    // un-split / split passes around every smoothing step (5 % of a 256^3 V-cycle).  EMG3D_HOME=0 (lab): off.
    // The coarse levels with split copies never see the reference layout at all: restriction and prolongation address
    // eW[1] / sW[1] directly (RestrictArgs::cxs, ProlongArgs::cxs).
    int use_home = (int)LAB_ENV("EMG3D_HOME", 1);
    bool home_on(Level<T>& L) { return use_home && &L == lv0.get() && split_on(L); }
    bool home_lvl(Level<T>& L) { return use_home && &L != lv0.get() && split_on(L); }
    void e_to_ref(Level<T>& L) {
        if (L.e_home != 1) return;
        convert_field(L, L.e, L.eW[1], 1, false, true);
        L.e_home = 0;
    }
    void e_to_w1(Level<T>& L) {
        if (L.e_home == 1) return;
        ensure_work(L, 1);
        convert_field(L, L.eW[1], L.e, 1, true, true);
        L.e_home = 1;
    }

    // lexicographic order, lines of <= 16 blocks: hyperplane loop inside one workgroup instead of a launch per hyperplane
    int lex_loop = (int)LAB_ENV("EMG3D_LEX_LOOP", 1);
    // sweep = false: arguments for k_line_factor (un-split model arrays);
    // sweep = true : arguments for the sweep kernels (working copies).
    void line_args(Level<T>& L, int dir, LineArgs<T>& a, bool sweep) {
        if (dir == 0) { a.L = 0; a.P = 1; a.Q = 2; }
        else if (dir == 1) { a.L = 1; a.P = 0; a.Q = 2; }
        else { a.L = 2; a.P = 0; a.Q = 1; }
        const SweepPlan& P = plan(L, dir);
        const bool sp = sweep && P.split;
        // the split working copy of the x direction is always the transposed one
        const bool t = (sp && dir == 0) ? true : P.xt;
        const int w = (dir == 0) ? 0 : 1;
        for (int q = 0; q < 3; ++q) {
            a.nC[q] = L.nC[q]; a.eta[q] = t ? L.etaT[q] : L.eta[q]; a.h[q] = L.h[q]; a.ih[q] = L.ih[q];
        }
        a.fl = t ? L.flT : L.fl; a.cl = t ? L.clT : L.cl;
        a.split = sp ? 1 : 0;
        if (sp) { a.e = L.eW[w]; a.s = L.sW[w]; a.zeta = L.zetaW[w]; }
        else { a.e = t ? L.eT : L.e; a.s = t ? L.sT : L.s; a.zeta = t ? L.zetaT : L.zeta; }
        const i64 nP = L.nC[a.P], nQ = L.nC[a.Q];
        a.nA[0] = (nP - 0) / 2; a.nA[1] = (nP - 1) / 2;
        const i64 nB[2] = {(nQ - 0) / 2, (nQ - 1) / 2};
        a.nB2[0] = nB[0]; a.nB2[1] = nB[1];
        i64 o = 0;
        for (int c = 0; c < 4; ++c) { a.base[c] = o; o += a.nA[c & 1] * nB[c >> 1]; }
        a.nLinesTot = o;   // == (nP-1)*(nQ-1)
        a.fac = L.fac[dir];
        a.mid = L.fac[dir] ? L.fac_mid[dir] : L.nC[a.L] - 1;
        a.qm = (L.fac[dir] && L.fac_kind[dir] == 3) ? 2 : 0;       // 2: mirrored two-sided factor, k_line_sweep_thm
        a.fcomp = (L.fac[dir] && L.fac_kind[dir] == 4) ? 1 : 0;
        a.zsep = (sweep && L.zeta_sep && use_zsep) ? 1 : 0;
        a.sflag = (sweep && sflag_on(L, dir) && L.sflag[dir] && L.sflag_valid[dir]) ? L.sflag[dir] : nullptr;
        a.xcd = xcd_map;
        a.tile = q_tile;
        {
            const int ax[3] = {a.L, a.P, a.Q};
            a.rs.ihL = a.ih[a.L]; a.rs.ihP = a.ih[a.P]; a.rs.ihQ = a.ih[a.Q];
            a.rs.hL = a.h[a.L]; a.rs.hP = a.h[a.P]; a.rs.hQ = a.h[a.Q];
            a.rs.nL = (unsigned)a.nC[a.L]; a.rs.slot0 = 0;
            a.rs.nP = (unsigned)a.nC[a.P]; a.rs.nQ = (unsigned)a.nC[a.Q];
            a.rs.csL = (unsigned)a.cl.st[a.L]; a.rs.csP = (unsigned)a.cl.st[a.P]; a.rs.csQ = (unsigned)a.cl.st[a.Q];
            for (int c = 0; c < 3; ++c) {
                a.rs.off[c] = (unsigned)a.fl.off[ax[c]];
                for (int d = 0; d < 3; ++d) a.rs.st[c][d] = (unsigned)a.fl.st[ax[c]][ax[d]];
            }
        }
        a.qd = nullptr; a.qdn = 0;
        a.sm = nullptr; a.smn = 0;
        a.fe = nullptr; a.fnE = 0; a.fax = a.fnX = a.fown = a.fns = a.fnp = 0; a.fseq = 0;
        for (int c = 0; c < 4; ++c) { a.fqd[c] = nullptr; a.fqdn[c] = 0; }
        a.qpl = P.NW; a.qM = P.M; a.seg = P.seg; a.qlpw = 0;
        a.tha = P.helpers;
        a.mode = 0; a.cP = a.cQ = 0; a.cntA = a.cntB = 0; a.t = a.jQ0 = a.cnt = 0;
        a.bt = sweep ? batch(L) : Batch();
    }

    // The cached factorisation of (level, direction), in the layout of the kernel family that will sweep it (SweepPlan::fac_kind).
    void ensure_factor(Level<T>& L, int dir) {
        const SweepPlan& P = plan(L, dir);
        if (P.xt) ensure_transposed_model(L);
        if (L.fac[dir]) return;
        L.fac_lines[dir] = (L.nC[dir == 0 ? 1 : 0] - 1) * (L.nC[dir == 2 ? 1 : 2] - 1);
        L.fac[dir] = dalloc<T>(L.fac_lines[dir] * P.fac_entries);
        L.fac_mid[dir] = P.mid;
        L.fac_kind[dir] = P.fac_kind;
        compute_factor(L, dir);
    }
    // (re)compute the cached factorisation of (level, direction) into its buffer: the model may have changed (set_smu0)
    void compute_factor(Level<T>& L, int dir) {
        LineArgs<T> a;
        line_args(L, dir, a, false);
        a.fac = L.fac[dir];
        a.fcomp = L.fac_kind[dir] == 4;
        if (L.fac_kind[dir] == 3) {  // all four colours in one launch
            a.mid = L.fac_mid[dir];
            const i64 nQ_ = L.nC[a.Q];
            const i64 nmax_ = a.nA[0] * ((nQ_ - 0) / 2);
            a.mode = 3;
            if (nmax_ > 0)
                MG_LAUNCH(k_line_factor_m<T>, dim3((unsigned)((nmax_ + EMG_LINE_BLOCK - 1) / EMG_LINE_BLOCK), 4),
                                   dim3(EMG_LINE_BLOCK), 0, stream, a);
            check_launch();
            return;
        }
        a.mid = L.fac_mid[dir];
        const i64 nQ = L.nC[a.Q];
        const i64 nB[2] = {(nQ - 0) / 2, (nQ - 1) / 2};
        // the four colours are independent here: one launch (blockIdx.y = colour), 4 x the threads of a
        // chain-latency-bound kernel (128^3 level 0: 4 x 0.45 ms -> one launch)
        a.mode = 3; a.cP = a.cQ = 0; a.cntA = a.cntB = 0;
        const i64 nmax = a.nA[0] * nB[0];
#ifdef EMG3D_LAB
        // lab: one launch per colour -- the thread-per-line factor recurrence with only ONE colour's lines on the chip is
        // the lower bound of a sweep that recomputes the factor instead of reading it (profiles/HISTORY.md, recompute)
        if (LAB_ENV("EMG3D_FACTOR_PER_COLOUR", 0)) {
            for (int c = 0; c < 4; ++c) {
                a.mode = 0; a.cP = c & 1; a.cQ = c >> 1; a.cntA = a.nA[a.cP]; a.cntB = nB[a.cQ];
                const i64 n = a.cntA * a.cntB;
                if (n > 0)
                    MG_LAUNCH(k_line_factor<T>, dim3((unsigned)((n + EMG_LINE_BLOCK - 1) / EMG_LINE_BLOCK)),
                                       dim3(EMG_LINE_BLOCK), 0, stream, a);
            }
            check_launch();
            return;
        }
#endif
        if (nmax > 0)
            MG_LAUNCH(k_line_factor<T>, dim3((unsigned)((nmax + EMG_LINE_BLOCK - 1) / EMG_LINE_BLOCK), 4),
                               dim3(EMG_LINE_BLOCK), 0, stream, a);
        check_launch();
    }

    // workgroups of a lane-group launch (a multiple of the 8 XCDs when the XCD-aware map is on: the kernels drop the workgroups
    // past the last line)
    unsigned xcd_grid(i64 nb) const { return (unsigned)(xcd_map ? ((nb + 7) / 8) * 8 : nb); }
    unsigned rp_grid(i64 nt) const { return xcd_grid((nt + EMG_RP_BLOCK - 1) / EMG_RP_BLOCK); }
    // Descriptors of the scan kernel's colour launches on levels of short lines (one wave per workgroup): everything of the
    // prologue that depends on grid and model only -- 11 element offsets / flags and 15 coefficient products per lane and block --
    // is computed ONCE, by the kernel's own prologue in generating mode, and loaded by the 7 launches of every smoothing call
    // thereafter (HISTORY R5.12).  Where: SweepPlan::qdesc.
    void ensure_qdesc(Level<T>& L, int dir) {
        const SweepPlan& P = plan(L, dir);
        if (!P.qdesc || L.qd[dir][0] || L.qdn[dir][0] == ~0u) return;
        L.qdn[dir][0] = ~0u;                                    // (asked once)
        if (!L.fac[dir]) return;
        LineArgs<T> a;
        line_args(L, dir, a, true);
        const i64 lpg = 16 / a.seg;
        a.bt = Batch();                                         // (the descriptors do not depend on the system)
        for (int c = 0; c < 4; ++c) {
            a.mode = 0; a.cP = c & 1; a.cQ = c >> 1;
            a.cntA = a.nA[a.cP]; a.cntB = a.nB2[a.cQ];
            a.rs.slot0 = (unsigned)a.base[c];
            const i64 n = a.cntA * a.cntB;
            if (n <= 0) continue;
            const unsigned grid = xcd_grid((n + lpg - 1) / lpg);
            const i64 nthreads = (i64)grid * 64;
            void* tab = try_alloc<char>(nthreads * a.qM * (3 * 16 + 8 * 16));     // (pure optimisation data: without it the kernel computes)
            if (!tab) return;
            a.qd = tab; a.qdn = (unsigned)nthreads;
            if (!broken) qpl_launch<T>(1, a.qM, false, 1, false, dim3(grid), stream, a);
            L.qd[dir][c] = tab; L.qdn[dir][c] = (unsigned)nthreads;
        }
        check_launch();
    }
    // Scan tables of the same colour launches (SweepPlan::scantab; smooth_qpl.hpp SM): the matrix part of every lane's row after
    // every full step of the two scans is a function of the factor and the level's coefficients, not of e or s.  The kernel's own
    // scans write it once (fill_scantab: the sweep as it runs without a table, storing the matrices instead of the field), every
    // sweep launch thereafter loads it and scans the offsets alone.  Optional memory: a refusal keeps the computing path.
    void ensure_scantab(Level<T>& L, int dir) {
        const SweepPlan& P = plan(L, dir);
        if (!P.scantab || L.sm[dir][0] || L.smn[dir][0] == ~0u) return;
        L.smn[dir][0] = ~0u;                                    // (asked once)
        if (!L.fac[dir]) return;
        LineArgs<T> a;
        line_args(L, dir, a, true);
        const i64 lpg = 16 / a.seg;
        const i64 rows = 2 * (i64)(__builtin_ctz((unsigned)a.seg) - 1) * 4;      // [pass][step][k]
        void* tab[4] = {nullptr, nullptr, nullptr, nullptr};
        unsigned nth[4] = {0, 0, 0, 0};
        for (int c = 0; c < 4; ++c) {
            const i64 n = a.nA[c & 1] * a.nB2[c >> 1];
            if (n <= 0) continue;
            nth[c] = xcd_grid((n + lpg - 1) / lpg) * 64u;
            tab[c] = try_alloc<T>((i64)nth[c] * rows);
            if (!tab[c]) return;                                // (all colours or none: the blocks taken stay with the handle)
        }
        for (int c = 0; c < 4; ++c) { L.sm[dir][c] = tab[c]; L.smn[dir][c] = nth[c]; }
        fill_scantab(L, dir);
    }
    // (re)write the scan tables of (level, direction) from the factor as it stands: after ensure_factor and after every
    // compute_factor of a factor that has tables (refresh_model, set_smu0)
    void fill_scantab(Level<T>& L, int dir) {
        if (!L.sm[dir][0] && !L.sm[dir][1] && !L.sm[dir][2] && !L.sm[dir][3]) return;
        LineArgs<T> a;
        line_args(L, dir, a, true);
        const i64 lpg = 16 / a.seg;
        a.bt = Batch();                                         // (the tables do not depend on the system)
        for (int c = 0; c < 4; ++c) {
            if (!L.sm[dir][c]) continue;
            a.mode = 0; a.cP = c & 1; a.cQ = c >> 1;
            a.cntA = a.nA[a.cP]; a.cntB = a.nB2[a.cQ];
            a.rs.slot0 = (unsigned)a.base[c];
            const i64 n = a.cntA * a.cntB;
            a.sm = L.sm[dir][c]; a.smn = L.smn[dir][c];
            if (!broken) qpl_scantab_launch<T>(1, 0, dim3(xcd_grid((n + lpg - 1) / lpg)), stream, a);
        }
        check_launch();
    }
    // name of the kernel instantiation the last line-sweep launch selected (bench.py's roofline object and the
    // sweep-level parity tests report it instead of guessing from the grid size)
    char sweep_name[64] = "";
    char res_name[64] = "";            // the same for the most recent residual launch
    // k_line_sweep_thm keeps the z of the last forward steps of a half in LDS instead of parking them in e (smooth_thm.hpp; how
    // many: sweep_thm_zkeep, sweep_plan.hpp -- what fits beside the static LDS in the CU's 160 KB, 59 of a 128-block line's 63 steps
    // per half at complex128).  The dynamic LDS was asked for per instantiation when the handle's knobs were filled
    // (sweep_device_knobs: before any launch sequence is captured); a device that refused it runs with kz = 0, every step parked.
    // Measured: profiles/thm_zkeep_ab.txt.
    int thm_keep(const SweepPlan& P, const LineArgs<T>& a) {
        const SweepShape G{{a.nC[0], a.nC[1], a.nC[2]}, (int)sizeof(T)};
        const i64 kz = sweep_thm_zkeep(knobs, G, a.L, P);
        const i64 granted = knobs.thm_lds_granted ? knobs.lds_limit - sweep_thm_static_lds(P.inst_lpw, (int)sizeof(T)) : 0;
        if (kz < 0 || kz * sweep_thm_keep_step_bytes(P.inst_lpw, (int)sizeof(T)) > granted) {
            fprintf(stderr, "emg3d_hip: k_line_sweep_thm would keep %lld steps in %lld bytes of LDS\n", (long long)kz, (long long)granted);
            abort();
        }
        return (int)kz;
    }
    // One launch of n lines (a colour, or a hyperplane of the lexicographic order) with the kernel the plan names: the grid, and the
    // instantiation through sweep_launch.hpp.
    void launch_sweep(const SweepPlan& P, const LineArgs<T>& a, i64 n) {
        if (log_launches) fprintf(stderr, "[sweep] nC %lld %lld %lld L %d lines %lld kernel %s split %d\n", (long long)a.nC[0], (long long)a.nC[1], (long long)a.nC[2], a.L, (long long)n,
                                  P.name, a.split);
        memcpy(sweep_name, P.name, sizeof sweep_name);
        if (broken) return;
        switch (P.family) {
        case SweepFamily::tha: {        // one workgroup per THA_LPW lines
            const size_t dyn = P.helpers == 2 ? tha_lds_bytes<T, 2>((int)a.nC[a.L]) : tha_lds_bytes<T, 3>((int)a.nC[a.L]);
            tha_launch<T>(P.helpers, a.zsep != 0, bgrid(xcd_grid((n + THA_LPW - 1) / THA_LPW)), dyn, stream, a);
            break;
        }
        case SweepFamily::thm: {        // a pair of waves per inst_lpw lines
            const i64 npairs = (n + P.inst_lpw - 1) / P.inst_lpw;
            thm_launch<T>(P.stages, P.inst_lpw, a.zsep != 0, thm_keep(P, a), bgrid(rp_grid(npairs * 128)), stream, a);
            break;
        }
        case SweepFamily::qpl:
        case SweepFamily::qpl_chain: {  // (16 NW) / seg lines per workgroup; single-wave workgroups load the descriptors of ensure_qdesc
            const i64 lpg = (16 * P.NW) / P.seg;
            if (a.sm && P.NW == 1 && P.M == 1 && P.family == SweepFamily::qpl) {
                qpl_scantab_launch<T>(2, a.qd ? 2 : 0, bgrid(xcd_grid((n + lpg - 1) / lpg)), stream, a);
                break;
            }
            qpl_launch<T>(P.NW, P.M, false, (P.NW == 1 && a.qd) ? 2 : 0, P.family == SweepFamily::qpl_chain,
                          bgrid(xcd_grid((n + lpg - 1) / lpg)), stream, a);
            break;
        }
        case SweepFamily::qc:
        case SweepFamily::qc_big: {     // the 16-line instantiation runs at the balanced number of lines per wave of THIS launch
            LineArgs<T> b = a;
            b.qlpw = P.inst_lpw == 16 ? sweep_balanced_lpw(knobs, n * nsys) : P.inst_lpw;
            qc_launch<T>(P.stages, P.inst_lpw, a.zsep != 0, P.big, bgrid(rp_grid(((n + b.qlpw - 1) / b.qlpw) * 64)), stream, b);
            break;
        }
        case SweepFamily::rp: {
            const unsigned g = rp_grid(((n + P.inst_lpw - 1) / P.inst_lpw) * 64);
            if (P.inst_lpw == 8) hipLaunchKernelGGL((k_line_sweep_rp<T, 8>), bgrid(g), dim3(EMG_RP_BLOCK), 0, stream, a);
            else if (P.inst_lpw == 12) hipLaunchKernelGGL((k_line_sweep_rp<T, 12>), bgrid(g), dim3(EMG_RP_BLOCK), 0, stream, a);
            else hipLaunchKernelGGL((k_line_sweep_rp<T, 4>), bgrid(g), dim3(EMG_RP_BLOCK), 0, stream, a);
            break;
        }
        case SweepFamily::tpl:
            hipLaunchKernelGGL(k_line_sweep<T>, bgrid_y((unsigned)((n + EMG_LINE_BLOCK - 1) / EMG_LINE_BLOCK)), dim3(EMG_LINE_BLOCK), 0, stream, a);
            break;
        }
    }

    // Bring e (and s, if stale) into the working copy used by direction `dir`,
    // or write the smoothed e back.
    // allocation-only counterpart of to_work (used by the dry run before graph capture)
    void prepare_work(Level<T>& L, int dir) {
        ensure_sflags(L, dir);          // (dry: allocation only)
        if (home_on(L) || home_lvl(L)) ensure_work(L, 1);
        if (split_on(L)) ensure_work(L, (dir == 0) ? 0 : 1);
        else if (plan(L, dir).xt) ensure_transposed_model(L);
    }
    void to_work(Level<T>& L, int dir) {
        ensure_sflags(L, dir);
        if (split_on(L)) {
            const int w = (dir == 0) ? 0 : 1;
            ensure_work(L, w);
            if (home_lvl(L)) {          // field and source live in the x-split copies
                if (w == 0) {
                    if (!L.sW_valid[0]) { convert_field(L, L.sW[0], L.sW[1], 2, true); L.sW_valid[0] = true; }
                    convert_field(L, L.eW[0], L.eW[1], 2, true);
                }
                return;
            }
            if (!L.sW_valid[w]) { convert_field(L, L.sW[w], L.s, w, true); L.sW_valid[w] = true; }
            if (!home_on(L)) convert_field(L, L.eW[w], L.e, w, true);
            else {      // every system's field into the x-split copy first (frozen systems keep theirs there)
                e_to_w1(L);
                if (w == 0) convert_field(L, L.eW[0], L.eW[1], 2, true);
            }
        } else if (plan(L, dir).xt) {
            if (!L.sT_valid) { convert_field(L, L.sT, L.s, -1, true); L.sT_valid = true; }
            convert_field(L, L.eT, L.e, -1, true);
        }
    }
    void from_work(Level<T>& L, int dir) {
        if (home_on(L) || home_lvl(L)) {       // the field stays in (x-lines: goes to) the x-split copy
            if (dir == 0) convert_field(L, L.eW[1], L.eW[0], 2, false);
        } else if (split_on(L)) convert_field(L, L.e, L.eW[(dir == 0) ? 0 : 1], (dir == 0) ? 0 : 1, false);
        else if (plan(L, dir).xt) convert_field(L, L.e, L.eT, -1, false);
    }
    int work_id(Level<T>& L, int dir) { return plan(L, dir).work_id; }

    // ---- placement of level 0's WRITTEN working copies (HISTORY R5.18, R6.1) -----------------------------------------------
    // A level-0 colour launch at 256^3 lasts 0.62 ... 0.73 ms depending on which piece of physical memory the working copy it
    // WRITES (eW[w]) got -- candidates fall into two classes 6-9 % apart, which one a hipMalloc returns differs from box to box and
    // from allocation to allocation; the blocks it only reads (factor, source) matter < 1 % (profiles/r06_placement.txt) -- and
    // hipMalloc does not expose it.  So the handle tries: right before the first launch sequence that sweeps on eW[w] is captured
    // (no graph holds the pointer yet) up to place_tries candidate blocks -- the one it has, then fresh ones, all held until the end so
    // that every candidate is another piece of memory -- are timed with one sweep each (4 ms per candidate at 256^3) until
    // one of the fast class is in hand; it stays, the others go back to the pool / driver.  The kept block is parked under its role
    // when the handle goes (DevicePool tags): later handles of the process take it without searching.  Only level 0, only working
    // copies of >= place_min_bytes (256 MiB); a candidate that cannot be allocated ends the search quietly.  The values a sweep
    // computes do not depend on the block it runs on (cycles bit-identical).  EMG3D_PLACE_TRIES=<n> (default 12; 0: off).
    int place_tries = getenv("EMG3D_PLACE_TRIES") ? atoi(getenv("EMG3D_PLACE_TRIES")) : 12;
    i64 place_min_bytes = LAB_ENV("EMG3D_PLACE_MIN_MB", 256) << 20;
    int place_reps = (int)LAB_ENV("EMG3D_PLACE_REPS", 1);
    double place_gap = 1.075;
    static const int PLACE_MAX = 16;
    struct PlaceRec { int tries = 0, kept = 0, reused = 0; float ms[PLACE_MAX] = {0}; };
    PlaceRec place_rec[2];
    bool placed[2] = {false, false};
    static bool lr_has(int lr, int dir) {
        return dir == 0 ? (lr == 1 || lr == 5 || lr == 6 || lr == 7) : dir == 1 ? (lr == 2 || lr == 4 || lr == 6 || lr == 7)
                                                                              : (lr == 3 || lr == 4 || lr == 5 || lr == 7);
    }
    bool place_applies(Level<T>& L) {
        return place_tries > 1 && order == 1 && !trace && split_on(L) &&
               (i64)nsys * L.nE * (i64)sizeof(T) >= place_min_bytes;
    }
    bool placement_pending(int lr_dir) {
        Level<T>& L = *lv0;
        if (!place_applies(L)) return false;
        const int lr = current_lr_dir(lr_dir, L.nC);
        return (lr_has(lr, 0) && !placed[0]) || ((lr_has(lr, 1) || lr_has(lr, 2)) && !placed[1]);
    }
    bool alloc_quiet = false;       // raw_alloc: a failing hipMalloc is the caller's business (no message, err untouched)
    template <class U>
    U* try_alloc(i64 n) {
        const int keep = err;
        const i64 keep_bytes = bytes;
        alloc_quiet = true;
        U* p = dalloc<U>(n);
        alloc_quiet = false;
        if (!p) { err = keep; bytes = keep_bytes; }
        return p;
    }
    float time_sweeps(Level<T>& L, int dir, int reps) {
        hipEvent_t t0 = nullptr, t1 = nullptr;
        float ms = -1.f;
        if (hipEventCreate(&t0) == hipSuccess && hipEventCreate(&t1) == hipSuccess && hipEventRecord(t0, stream) == hipSuccess) {
            for (int i = 0; i < reps; ++i) smooth_line(L, dir, 1, false, false);
            if (hipEventRecord(t1, stream) == hipSuccess && hipEventSynchronize(t1) == hipSuccess &&
                hipEventElapsedTime(&ms, t0, t1) == hipSuccess) ms /= (float)reps;
            else ms = -1.f;
        }
        if (ms < 0.f) (void)hipGetLastError();
        if (t0) hipEventDestroy(t0);
        if (t1) hipEventDestroy(t1);
        return ms;
    }
    void place_level0(int lr_dir) {
        Level<T>& L = *lv0;
        if (dry || !placement_pending(lr_dir)) return;
        const int lr = current_lr_dir(lr_dir, L.nC);
        bool moved = false;
        for (int w = 0; w < 2; ++w) {
            const int dir = (w == 0) ? (lr_has(lr, 0) ? 0 : -1) : lr_has(lr, 1) ? 1 : lr_has(lr, 2) ? 2 : -1;
            if (placed[w] || dir < 0 || !L.eW[w] || !L.sW[w] || !L.fac[dir]) continue;
            placed[w] = true;
            if (w == 1) e_to_ref(L);            // (the field may be at home in eW[1]: back to the reference layout first)
            if (!L.sW_valid[w]) { convert_field(L, L.sW[w], L.s, w, true); L.sW_valid[w] = true; }
            ensure_sflags(L, dir);
            const i64 n = (i64)nsys * L.nE;
            PlaceRec& R = place_rec[w];
            R = PlaceRec();
            T* cands[PLACE_MAX];
            cands[0] = L.eW[w];
            int best = 0;
            float worst = 0.f;
            const int nt = std::min<int>(place_tries, PLACE_MAX);
            for (int k = 0; k < nt; ++k) {
                T* c = (k == 0) ? cands[0] : try_alloc<T>(n);
                if (!c) break;
                cands[k] = c;
                hipMemsetAsync(c, 0, (size_t)n * sizeof(T), stream);
                L.eW[w] = c;
                if (k == 0) (void)time_sweeps(L, dir, 1);       // (the first launches of a kernel in a process: code upload)
                const float ms = time_sweeps(L, dir, place_reps);
                R.ms[k] = ms;
                R.tries = k + 1;
                if (ms < 0.f) break;
                if (ms < R.ms[best]) best = k;
                worst = std::max(worst, ms);
                // the candidates fall into classes (about 2.60 / 2.46 / 2.28 ms per 256^3 sweep): holding one that is place_gap faster than
                // the slowest seen -- fast against mid, or fast against slow -- ends the search; mid against slow (5 %) does not
                if ((double)R.ms[best] * place_gap < (double)worst) break;
            }
            if (R.ms[best] < 0.f) best = 0;
            R.kept = best;
            L.eW[w] = cands[best];
            block_tag[cands[best]] = 1 + w;
            for (int k = 0; k < R.tries; ++k) if (k != best) release(cands[k]);
            moved |= best != 0;
            if (getenv("EMG3D_LOG_SETUP")) {
                fprintf(stderr, "[place] working copy %d (%s-lines, %.0f MB): kept candidate %d of %d;", w, dir == 0 ? "x" : dir == 1 ? "y" : "z",
                        (double)n * sizeof(T) / 1048576.0, best, R.tries);
                for (int k = 0; k < R.tries; ++k) fprintf(stderr, " %.3f", R.ms[k]);
                fprintf(stderr, " ms per sweep\n");
            }
        }
        if (moved) drop_graphs();       // (none holds these pointers on the usual paths; a graph of an x-only cycle may)
        check_launch();
    }

    // The colours c = cP + 2 cQ of the passes of a call of nu sweeps in colour order -- THE list: the per-pass launches and the fused
    // launch both run it.  The first sweep runs backward (core.py:552, 569).  A line update is a projection: re-solving a colour
    // whose neighbours (all of other colours) have not changed since its last update reproduces the same values; a backward sweep
    // ends with the colour the next forward sweep starts with, so the repeated colour at each turn-around is skipped (identical
    // result up to rounding).  Colours without a line are left out.
    void colour_passes(Level<T>& L, int dir, int nu, std::vector<int>& seq) {
        int Pa, Qa;
        sweep_axes(dir, Pa, Qa);
        const i64 nP = L.nC[Pa], nQ = L.nC[Qa];
        int iback = 0, last_c = -1;
        seq.clear();
        for (int it = 0; it < nu; ++it) {
            iback = 1 - iback;
            for (int ch = 0; ch < 4; ++ch) {
                const int c = iback ? colour_perm_b[ch] : colour_perm[ch];
                if (skip_idempotent && c == last_c) continue;
                last_c = c;
                if (((nP - (c & 1)) / 2) * ((nQ - (c >> 1)) / 2) <= 0) continue;
                seq.push_back(c);
            }
        }
    }
    // How a call of nu sweeps along dir is issued (sweep_plan.hpp plan_fuse), decided once per (level, direction, nu): fused only with
    // the descriptor tables of its colours and the private copies in hand (optional memory, asked for here -- also in the dry run
    // before a capture; a refusal keeps the per-pass launches).  Level::passes[dir] holds the call's colours afterwards.
    const FusePlan& ensure_fuse(Level<T>& L, int dir, int nu) {
        const int key = nu * 256 + order + 2 * nsys;
        if (L.fuse_key[dir] == key) return L.fuse[dir];
        FusePlan& F = L.fuse[dir];
        F = FusePlan();
        L.fuse_key[dir] = key;
        L.passes[dir].clear();
        if (order != 1) return F;
        colour_passes(L, dir, nu, L.passes[dir]);
        const std::vector<int>& seq = L.passes[dir];
        plan(L, dir);
        F = plan_fuse(knobs, SweepShape{{L.nC[0], L.nC[1], L.nC[2]}, (int)sizeof(T)}, dir, (int)seq.size());
        if (!F.fused) return F;
        for (int c : seq) if (!L.qd[dir][c]) { F.fused = false; return F; }
        const i64 need = (i64)nsys * F.g.nslabs * L.nE;
        if (L.fz_n[dir] < need) {
            T* z = try_alloc<T>(need);
            if (!z) { F.fused = false; return F; }
            // (the systems of a handle change only before its first cycle, emg3d_mg_set_batch: no captured launch holds the smaller block)
            if (L.fz[dir]) release(L.fz[dir]);
            L.fz[dir] = z; L.fz_n[dir] = need;
        }
        return F;
    }
    // all colour passes of the call in one launch on private slab copies, then every edge from its owner's copy
    void smooth_fused(Level<T>& L, int dir, const SweepPlan& P, const FusePlan& F, const std::vector<int>& seq, const LineArgs<T>& a) {
        LineArgs<T> b = a;
        b.mode = 0; b.xcd = 0;
        b.fe = L.fz[dir]; b.fnE = L.nE; b.fax = F.axis;
        b.fnX = F.g.nX; b.fown = F.g.own; b.fns = F.g.nslabs; b.fnp = F.g.npass;
        b.fseq = 0;
        for (int p = 0; p < F.g.npass; ++p) b.fseq |= (unsigned long long)seq[(size_t)p] << (4 * p);
        for (int c = 0; c < 4; ++c) { b.fqd[c] = L.qd[dir][c]; b.fqdn[c] = L.qd[dir][c] ? L.qdn[dir][c] : 0u; }
        if (log_launches) fprintf(stderr, "[sweep] nC %lld %lld %lld L %d lines %lld kernel %s split %d fused passes %d slabs %d own %d\n", (long long)a.nC[0],
                                  (long long)a.nC[1], (long long)a.nC[2], a.L, (long long)a.nLinesTot, P.name, a.split, F.g.npass, F.g.nslabs, F.g.own);
        memcpy(sweep_name, P.name, sizeof sweep_name);
        if (broken) return;
        qpl_fused_launch<T>(P.family == SweepFamily::qpl_chain, bgrid((unsigned)F.g.nslabs), stream, b);
        ScatterArgs sa;
        sa.nE = L.nE; sa.g = F.g;
        int Pa, Qa;
        sweep_axes(dir, Pa, Qa);
        sa.ax = F.axis ? Qa : Pa;
        for (int c = 0; c < 3; ++c) {
            sa.off[c] = L.fl.off[c];
            sa.d0[c] = (unsigned)((c == 0) ? L.nC[0] : L.nC[0] + 1); sa.d1[c] = (unsigned)((c == 1) ? L.nC[1] : L.nC[1] + 1);
        }
        hipLaunchKernelGGL(k_scatter_slabs<T>, dim3((unsigned)((L.nE + EMG_BLOCK - 1) / EMG_BLOCK), (unsigned)nsys), dim3(EMG_BLOCK), 0, stream,
                           a.e, (const T*)L.fz[dir], sa, a.bt);
    }

    // nu sweeps along `dir`; conv_in / conv_out: convert e to / from the working copy
    void smooth_line(Level<T>& L, int dir, int nu, bool conv_in = true, bool conv_out = true) {
        if (nu <= 0) return;
        ensure_factor(L, dir);
        ensure_qdesc(L, dir);
        ensure_scantab(L, dir);
        const FusePlan& F = ensure_fuse(L, dir, nu);
        if (dry) { prepare_work(L, dir); return; }
        if (conv_in) to_work(L, dir);
        ensure_sflags(L, dir);          // (valid already inside a captured sequence: refresh_level0_source)
        LineArgs<T> a;
        line_args(L, dir, a, true);
        const SweepPlan& P = plan(L, dir);
        const i64 nP = L.nC[a.P], nQ = L.nC[a.Q];
        const i64 nB[2] = {(nQ - 0) / 2, (nQ - 1) / 2};
        if (order == 1) {
            if (F.fused) smooth_fused(L, dir, P, F, L.passes[dir], a);
            else for (int c : L.passes[dir]) {
                a.mode = 0; a.cP = c & 1; a.cQ = c >> 1;
                a.cntA = a.nA[a.cP]; a.cntB = nB[a.cQ];
                a.rs.slot0 = (unsigned)a.base[c];
                a.qd = L.qd[dir][c]; a.qdn = (L.qd[dir][c] ? L.qdn[dir][c] : 0u);
                a.sm = L.sm[dir][c]; a.smn = (L.sm[dir][c] ? L.smn[dir][c] : 0u);
                launch_sweep(P, a, a.cntA * a.cntB);
            }
            nu = 0;
        }
        int iback = 0;
        for (int it = 0; it < nu; ++it) {      // lexicographic order
            iback = 1 - iback;   // first sweep runs backward (core.py:552, 569)
            {
                const i64 tmin = 3, tmax = (nP - 1) + 2 * (nQ - 1);
                if (lex_loop && a.qpl && a.qM == 1 && a.seg <= 16) {
                    // short lines: ONE workgroup per system loops over the hyperplanes (k_line_sweep_qpl mode 2) --
                    // the same line solves in the same order as the launches below, without the launch boundaries
                    LineArgs<T> b = a;
                    b.mode = 2; b.t = tmin; b.jQ0 = tmax; b.cnt = iback; b.xcd = 0;
                    const i64 maxn = std::min<i64>(nQ - 1, (nP - 1) / 2 + 1), quads = maxn * a.seg;
                    const int lnw = quads <= 16 ? 1 : quads <= 32 ? 2 : quads <= 64 ? 4 : 8;
                    if (!broken) qpl_launch<T>(lnw, 1, true, 0, false, bgrid(1), stream, b);
                    sweep_kernel_name(sweep_name, sizeof sweep_name, SweepFamily::qpl, (int)sizeof(T), lnw, 1);
                    continue;
                }
                for (i64 th = tmin; th <= tmax; ++th) {
                    const i64 tt = iback ? tmax - (th - tmin) : th;
                    i64 lo = tt - (nP - 1);                 // jQ >= ceil(lo/2)
                    i64 jQ0 = lo <= 0 ? 1 : (lo + 1) / 2;
                    if (jQ0 < 1) jQ0 = 1;
                    i64 jQ1 = (tt - 1) / 2;
                    if (jQ1 > nQ - 1) jQ1 = nQ - 1;
                    const i64 n = jQ1 - jQ0 + 1;
                    if (n <= 0) continue;
                    a.mode = 1; a.t = tt; a.jQ0 = jQ0; a.cnt = n;
                    launch_sweep(P, a, n);
                }
            }
        }
        if (conv_out) from_work(L, dir);
        check_launch();
    }

    void smooth_point(Level<T>& L, int nu) {
        if (dry) return;
        if (&L == lv0.get()) e_to_ref(L);
        const bool hl = home_lvl(L) && L.e_home == 1;        // point smoothing of a level that lives in the x-split copies: through e, s
        if (hl) { convert_field(L, L.e, L.eW[1], 1, false); convert_field(L, L.s, L.sW[1], 1, false); }
        PointArgs<T> a;
        for (int q = 0; q < 3; ++q) { a.nC[q] = L.nC[q]; a.eta[q] = L.eta[q]; a.h[q] = L.h[q]; a.ih[q] = L.ih[q]; }
        a.fl = L.fl; a.e = L.e; a.s = L.s; a.zeta = L.zeta; a.bt = batch(L);
        a.col = 0; a.t = 0; a.cnt[0] = a.cnt[1] = a.cnt[2] = 0;
        int iback = 0;
        int last_c = -1;
        for (int it = 0; it < nu; ++it) {
            iback = 1 - iback;
            if (order == 1) {
                for (int ch = 0; ch < 8; ++ch) {
                    const int c = iback ? point_perm_b[ch] : point_perm[ch];
                    if (skip_idempotent && c == last_c) continue;   // see smooth_line
                    last_c = c;
                    a.mode = 0; a.col = c;
                    for (int q = 0; q < 3; ++q) a.cnt[q] = (L.nC[q] - ((c >> q) & 1)) / 2;
                    const i64 n = a.cnt[0] * a.cnt[1] * a.cnt[2];
                    if (n <= 0) continue;
                    MG_LAUNCH(k_point_sweep<T>, bgrid_y((unsigned)((n + EMG_LINE_BLOCK - 1) / EMG_LINE_BLOCK)),
                                       dim3(EMG_LINE_BLOCK), 0, stream, a);
                }
            } else {
                const i64 tmin = 7, tmax = (L.nC[0] - 1) + 2 * (L.nC[1] - 1) + 4 * (L.nC[2] - 1);
                const i64 n = (L.nC[1] - 1) * (L.nC[2] - 1);
                for (i64 th = tmin; th <= tmax; ++th) {
                    a.mode = 1; a.t = iback ? tmax - (th - tmin) : th;
                    MG_LAUNCH(k_point_sweep<T>, bgrid_y((unsigned)((n + EMG_LINE_BLOCK - 1) / EMG_LINE_BLOCK)),
                                       dim3(EMG_LINE_BLOCK), 0, stream, a);
                }
            }
        }
        if (hl) convert_field(L, L.eW[1], L.e, 1, true);
        check_launch();
    }

    // solver.smoothing, solver.py:738-799
    void smoothing(Level<T>& L, int nu, int lr_dir) {
        const int lr = current_lr_dir(lr_dir, L.nC);
        if (lr == 0) smooth_point(L, nu);
        int dirs[3], nd = 0;
        if (lr == 1 || lr == 5 || lr == 6 || lr == 7) dirs[nd++] = 0;
        if (lr == 2 || lr == 4 || lr == 6 || lr == 7) dirs[nd++] = 1;
        if (lr == 3 || lr == 4 || lr == 5 || lr == 7) dirs[nd++] = 2;
        // consecutive directions that share a working copy (y and z) convert once
        for (int k = 0; k < nd; ++k) {
            const bool in = (k == 0) || work_id(L, dirs[k - 1]) != work_id(L, dirs[k]);
            const bool out = (k == nd - 1) || work_id(L, dirs[k + 1]) != work_id(L, dirs[k]);
            smooth_line(L, dirs[k], nu, in, out);
        }
    }

    // ------------------------------------------------- residual / transfer
    // mode 1: L.r = s - A e ; mode 2: norm only -> norms[slot]
    void residual(Level<T>& L, int mode, int slot) {
        ResidualArgs<T> a;
        for (int q = 0; q < 3; ++q) { a.nC[q] = L.nC[q]; a.eta[q] = L.eta[q]; a.h[q] = L.h[q]; a.ih[q] = L.ih[q]; }
        a.fl = L.fl; a.r = L.r; a.s = L.s; a.e = L.e; a.zeta = L.zeta; a.bt = batch(L);
        if (!dry && L.e_home == 1) {        // level 0, field and source in the x-split copies (home_on)
            if (!L.sW_valid[1]) { convert_field(L, L.sW[1], L.s, 1, true); L.sW_valid[1] = true; }
            a.e = L.eW[1]; a.s = L.sW[1]; a.xs = 1;
        }
        const i64 plane = (L.nC[0] + 1) * (L.nC[1] + 1);
        // levels with millions of cells: KZ node planes per thread (k_residual_zm, same results); below, a plane each
        const i64 cells = L.nC[0] * L.nC[1] * L.nC[2];
        const int kz = cells < res_zm_min ? 1 : res_kz ? res_kz : (cells * nsys >= ((i64)8 << 20) ? 8 : 4);
        const i64 nNz = L.nC[2] + 1;
        dim3 grid((unsigned)((plane + EMG_BLOCK - 1) / EMG_BLOCK), (unsigned)((nNz + kz - 1) / kz), (unsigned)nsys);
        a.nbx = grid.x;
        a.xcd = ((int)grid.x < res_xcd_min) ? 0 : res_xcd >= 0 ? res_xcd : (kz > 1 ? 2 : 1);
        if (a.xcd == 2) grid.x = 8 * ((grid.x + 7) / 8);       // strips: surplus workgroups exit
        const i64 np = (i64)a.nbx * nNz;                       // one partial per block and plane, whatever kz
        if (mode == 2 && np * nsys > n_partials) { partials = dalloc<double>(np * nsys); n_partials = np * nsys; }
        if (dry) return;
        {
            const char* tn = sizeof(T) == 16 ? "c128" : "f64";
            if (kz > 1) snprintf(res_name, sizeof res_name, "k_residual_zm<%s,%d,%d>", tn, mode, kz);
            else snprintf(res_name, sizeof res_name, "k_residual<%s,%d>", tn, mode);
        }
        if (mode == 2) {
            // a frozen system writes no partials: its norm slot keeps... nothing meaningful -- the host ignores
            // the norms of frozen systems (the partials are zeroed so that the sum stays finite)
            a.partials = partials;
            if (nsys > 1 && bmask) hipMemsetAsync(partials, 0, (size_t)(np * nsys) * sizeof(double), stream);
            if (!broken) residual_launch<T>(2, kz, grid, stream, a);
            MG_LAUNCH(k_sum_sqrt, dim3(nsys), dim3(EMG_BLOCK), 0, stream, (const double*)partials, np,
                               norm_out ? norm_out : norms, slot);
        } else {
            a.partials = nullptr;
            if (!broken) residual_launch<T>(1, kz, grid, stream, a);
        }
        check_launch();
    }

    void restrict_to(Level<T>& L, const Transfer& X, Level<T>& C) {   // solver.py:886-899
        const bool hl = home_lvl(C);
        if (hl) { ensure_work(C, 1); C.e_home = 1; }
        if (dry) return;
        RestrictArgs<T> a;
        for (int q = 0; q < 3; ++q) { a.cnC[q] = C.nC[q]; a.fnC[q] = L.nC[q]; a.co[q] = X.co[q]; }
        a.cfl = C.fl; a.ffl = L.fl; a.cr = C.s; a.r = L.r; a.pec = 1;
        C.sT_valid = false; C.sW_valid[0] = C.sW_valid[1] = false;
        for (int ax = 0; ax < 3; ++ax) for (int q = 0; q < 3; ++q) a.w[ax][q] = X.w[ax][q];
        a.ce = C.e; a.bt = batch(L); a.cbst = C.nE;
        if (hl) { a.cr = C.sW[1]; a.ce = C.eW[1]; a.cxs = 1; C.sW_valid[1] = true; }
        i64 nmax = 0;       // one launch: blockIdx.y = component
        for (int c = 0; c < 3; ++c) {
            i64 n = 1;
            for (int q = 0; q < 3; ++q) n *= (q == c) ? C.nC[q] : C.nC[q] + 1;
            nmax = std::max(nmax, n);
        }
        MG_LAUNCH(k_restrict<T>, dim3((unsigned)((nmax + EMG_BLOCK - 1) / EMG_BLOCK), 3, (unsigned)nsys), dim3(EMG_BLOCK), 0, stream, a);
        check_launch();
    }

    void prolong_from(Level<T>& L, const Transfer& X, Level<T>& C) {  // solver.py:904-977
        if (dry) return;
        ProlongArgs<T> a;
        for (int q = 0; q < 3; ++q) { a.fnC[q] = L.nC[q]; a.cnC[q] = C.nC[q]; a.co[q] = X.co[q]; a.idx[q] = X.pidx[q]; a.wt[q] = X.pwt[q]; }
        a.ffl = L.fl; a.cfl = C.fl; a.e = L.e; a.ce = C.e; a.bt = batch(L); a.cbst = C.nE;
        if (L.e_home == 1) { a.e = L.eW[1]; a.fxs = 1; }
        if (C.e_home == 1) { a.ce = C.eW[1]; a.cxs = 1; }
        i64 nmax = 0;       // one launch: blockIdx.y = component
        for (int c = 0; c < 3; ++c) {
            i64 n = 1;
            for (int q = 0; q < 3; ++q) n *= (q == c) ? L.nC[q] : L.nC[q] + 1;
            nmax = std::max(nmax, n);
        }
        MG_LAUNCH(k_prolong<T>, dim3((unsigned)((nmax + EMG_BLOCK - 1) / EMG_BLOCK), 3, (unsigned)nsys), dim3(EMG_BLOCK), 0, stream, a);
        check_launch();
    }

    // ----------------------------------------------------------- recursion
    // One visit of solver.multigrid for level > 0 (solver.py:471-586).
    void mg_level(int g, int lr_dir, int level, int new_cycmax) {
        int cm;
        if (level == clevel[g]) cm = 1;
        else if (new_cycmax == 0 || cycle != 'F') cm = cycmax;
        else cm = new_cycmax;
        int cyc = 0, it = 0;
        while (it < cm) {
            iterate(g, lr_dir, level, cm - cyc, it, cm);
            ++it; ++cyc;
        }
    }

    // Body of the while loop (solver.py:524-577) for any level.
    void trace_point(Level<T>& L, int it, int level, int cm, int kind) {
        if (!trace || dry || nsys != 1) return;
        if ((int)trace_recs.size() >= TRACE_MAX) { ++trace_dropped; return; }
        if (!trace_norms) trace_norms = dalloc<double>(TRACE_MAX);
        if (!trace_norms) return;
        double* const keep = norm_out;
        norm_out = trace_norms;
        residual(L, 2, (int)trace_recs.size());
        norm_out = keep;
        trace_recs.push_back(TraceRec{it, level, cm, kind, {L.nC[0], L.nC[1], L.nC[2]}});
    }
    // it, cm: iteration count and cycmax of this level's loop (the trace reports them; level 0: it = -1, the host counts)
    void iterate(int g, int lr_dir, int level, int child_cycmax, int it = -1, int cm = 0) {
        Hierarchy<T>& H = hierarchy(g);
        Level<T>& L = *H.lv[level];
        if (level == clevel[g]) {
            smoothing(L, nu_coarse, lr_dir);
            trace_point(L, it, level, cm, 0);
        } else {
            if (nu_pre > 0) { smoothing(L, nu_pre, lr_dir); trace_point(L, it, level, cm, 1); }
            Level<T>& C = *H.lv[level + 1];
            residual(L, 1, 0);
            restrict_to(L, H.tr[level], C);
            mg_level(g, lr_dir, level + 1, child_cycmax);
            prolong_from(L, H.tr[level], C);
            if (nu_post > 0) { smoothing(L, nu_post, lr_dir); trace_point(L, it, level, cm, 2); }
        }
    }

    // One level-0 iteration + end-of-cycle residual norm into norms[slot].
    // cycmax of LEVEL 0.  solver.multigrid evaluates it ONCE, on entry, with the sc_dir of that moment
    // (solver.py:480-485), and keeps it while sc_dir rotates from cycle to cycle: a solve that starts with a direction
    // whose clevel is 0 (level 0 is its coarsest grid, e.g. 8 x 3 x 3 with sc_dir 1) hands new_cycmax = 1 to the
    // children of ALL its later cycles -- its F-cycles then visit the coarse levels once, like V-cycles.
    // emg3d_mg_begin(sc_dir) records that moment; 0: not recorded, every cycle uses its own sc_dir.
    int entry_cm = 0;
    void cycle0_eager(int g, int lr_dir, int slot) {
        int cm = entry_cm ? entry_cm : ((0 == clevel[g]) ? 1 : cycmax);   // level 0: new_cycmax == 0
        iterate(g, lr_dir, 0, cm, -1, cm);        // cyc == 0 on level 0 (solver.py:585-586)
        residual(*lv0, 2, slot);
    }

    // A cycle is ~10^3 dependent kernel launches, many of them a few
    // microseconds long: issued one by one the host cannot keep the queue full.
    // The launch sequence of a (sc_dir, lr_dir) pair is fixed once its hierarchy
    // and factor caches exist, so it is captured into a hipGraph on its second
    // use and replayed afterwards (the first use runs eagerly and allocates).
    // The level-0 source changes only through set_sfield; its working copies are
    // refreshed here, OUTSIDE the captured graphs (a graph captured while a copy
    // was still valid would otherwise replay without the conversion).
    void refresh_level0_source() {
        Level<T>& L = *lv0;
        if (L.sT && !L.sT_valid) { convert_field(L, L.sT, L.s, -1, true); L.sT_valid = true; }
        for (int w = 0; w < 2; ++w)
            if (L.sW[w] && !L.sW_valid[w]) { convert_field(L, L.sW[w], L.s, w, true); L.sW_valid[w] = true; }
        for (int d = 0; d < 3; ++d)
            if (L.sflag[d]) ensure_sflags(L, d);
    }

    // Everything a cycle with (sc_dir g, lr_dir) needs that is loop invariant: grid hierarchy, transfer
    // weights, coarse models, factor caches, work buffers and the captured launch sequence.  Launches no
    // cycle; the fields are untouched.
    void prepare(int g, int lr_dir) {
        if (!use_graph) { dry = true; cycle0_eager(g, lr_dir, 0); dry = false; place_level0(lr_dir); return; }
        cycle0(g, lr_dir, -1);
    }

    // slot < 0: prepare only (see above)
    void cycle0(int g, int lr_dir, int slot) {
        if (!use_graph || trace) {      // (tracing: eager launches)
            if (slot >= 0) {
                if (placement_pending(lr_dir)) prepare(g, lr_dir);      // (eager cycles place their working copies too)
                cycle0_eager(g, lr_dir, slot);
            }
            return;
        }
        const int key = (g * 8 + lr_dir) * 4 + entry_cm;       // the captured launch sequence depends on level 0's cycmax
        auto it = graphs.find(key);
        if (it != graphs.end() && slot < 0) return;
        // a cycle that line-smooths level 0 starts (and ends) with the field in the x-split copy
        const int home_in = (home_on(*lv0) && current_lr_dir(lr_dir, lv0->nC) != 0) ? 1 : 0;
        if (it == graphs.end()) {
            // dry run: build hierarchy, factor caches and work buffers (the only
            // steps that allocate), then capture the launch sequence
            const bool tlog = getenv("EMG3D_LOG_SETUP") != nullptr;
            auto now = [] { return std::chrono::steady_clock::now(); };
            auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            auto t0 = now();
            const size_t nalloc0 = allocs.size();
            dry = true;
            cycle0_eager(g, lr_dir, 0);
            dry = false;
            place_level0(lr_dir);           // (large level 0: choose the blocks its sweeps write to, before any graph holds them)
            // where the captured sequence finds the field.  Launch path: move it there now.  Prepare-only path (it may run
            // on the side stream beside a cycle that is using the field): nothing is moved, the branch decisions of the
            // capture are taken as if, and the real state comes back afterwards -- the launch converts when it is due.
            const int home_keep = (slot >= 0) ? home_in : lv0->e_home;
            if (slot >= 0) { if (home_in) e_to_w1(*lv0); else e_to_ref(*lv0); }
            else if (home_in) ensure_work(*lv0, 1);
            lv0->e_home = home_in;
            refresh_level0_source();
            if (tlog) hipStreamSynchronize(stream);
            auto t1 = now();
            hipGraph_t graph = nullptr;
            hipGraphExec_t exec = nullptr;
            hipError_t st = hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal);
            if (st == hipSuccess) {
                cycle0_eager(g, lr_dir, 0);
                st = hipStreamEndCapture(stream, &graph);
            }
            const int home_out = lv0->e_home;
            lv0->e_home = home_keep;        // nothing has run yet
            auto t2 = now();
            if (st == hipSuccess) st = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            if (graph) hipGraphDestroy(graph);
            if (tlog) fprintf(stderr, "[setup] key %d: hierarchy+factors %.2f ms (%zu allocations), capture %.2f ms, instantiate %.2f ms\n",
                              key, ms(t0, t1), allocs.size() - nalloc0, ms(t1, t2), ms(t2, now()));
            if (st != hipSuccess || err != 0) {
                // capture not possible: fall back to eager launches for good
                (void)hipGetLastError();
                fprintf(stderr, "[emg3d_hip] hipGraph capture failed (%s); using eager launches\n", hipGetErrorString(st));
                use_graph = false;
                err = 0;
                if (slot >= 0) cycle0_eager(g, lr_dir, slot);
                return;
            }
            (void)hipGraphUpload(exec, stream);     // move the first-launch upload out of the first cycle
            graphs[key] = exec;
            graph_home[key] = std::make_pair(home_in, home_out);
            it = graphs.find(key);
            if (slot < 0) return;
        }
        const std::pair<int, int> hm = graph_home[key];
        if (hm.first) e_to_w1(*lv0); else e_to_ref(*lv0);
        refresh_level0_source();
        hipError_t st = hipGraphLaunch(it->second, stream);
        if (st != hipSuccess && err == 0) err = (int)st;
        lv0->e_home = hm.second;
        if (slot != 0) hipMemcpyAsync(norms + (i64)slot * nsys, norms, (size_t)nsys * sizeof(double), hipMemcpyDeviceToDevice, stream);
    }

    void forget_factors() {
        // (the launch descriptors carry factor offsets of the layout they were generated for: they go with the factor)
        auto clear = [](Level<T>& L) {
            for (int d = 0; d < 3; ++d) {
                L.fac[d] = nullptr; L.fac_kind[d] = 0; L.plan_key[d] = -1; L.fuse_key[d] = -1;
                for (int c = 0; c < 4; ++c) { L.qd[d][c] = nullptr; L.qdn[d][c] = 0; L.sm[d][c] = nullptr; L.smn[d][c] = 0; }
            }
        };
        if (lv0) clear(*lv0);
        for (auto& kv : hier) for (auto& l : kv.second.lv) if (l) clear(*l);
    }

    void drop_graphs() {
        for (auto& kv : graphs) hipGraphExecDestroy(kv.second);
        graphs.clear();
        graph_home.clear();
        graph_seen.clear();
    }
};
