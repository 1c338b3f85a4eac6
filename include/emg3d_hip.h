/*
 * emg3d_hip.h -- C ABI of the MI355X (gfx950) multigrid hot path for emg3d.
 *
 * This shared library (libemg3d_hip.so) stands where the numba module
 * `emg3d/core.py` and the cycle sub-routines of `emg3d/solver.py` stand in the
 * reference (emg3d v0.17.0).  Plain pointers and sizes only; no torch types.
 *
 * Conventions (identical to the reference):
 *   dtype   0 = float64 (Laplace domain), 1 = complex128 (frequency domain;
 *           interleaved re,im doubles)                     fields.py:417-420
 *   field   ONE 1-D buffer [fx | fy | fz]; fx F-ordered (nCx,nNy,nNz),
 *           fy (nNx,nCy,nNz), fz (nNx,nNy,nCz)              fields.py:253-281
 *   eta_*   F-ordered (nCx,nCy,nCz) of `dtype`; eta_y/eta_z may alias eta_x
 *   zeta,h  float64                                         models.py:631-658
 *   order   0 = lexicographic (the reference's update order, executed as
 *               hyperplane wavefronts; same result as the sequential sweep)
 *           1 = multi-colour (4 colours for line smoothers, 8 for the point
 *               smoother): the throughput mode
 * Every function returns 0 on success, a HIP error code (>0) on a device
 * error, or a negative value for invalid arguments; numerical blow-ups surface
 * as NaN/Inf in the data exactly as in the reference (solver.py:1715).
 *
 * Tier 1: stateless host-pointer kernels, one per `emg3d.core` function
 * (H2D, kernel, D2H inside the call) -- used by the drop-in `core` module and
 * the parity tests.  Tier 2: a handle that keeps grids, model, fields and the
 * cached line factorisations device-resident across a whole solve.
 */
#ifndef EMG3D_HIP_H
#define EMG3D_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library / device ------------------------------------------------- */
/* ABI version: bumped whenever an entry point is added or a signature changes; emg3d_hip_version() returns the value the
 * library was built with, and the Python binding (emg3d_amd/_lib.py: ABI_VERSION) refuses a library of another version. */
#define EMG3D_HIP_ABI_VERSION 121
int emg3d_hip_version(void);
int emg3d_hip_device_count(int* count);
int emg3d_hip_set_device(int device);
/* name must hold >= 256 bytes */
int emg3d_hip_device_info(int device, char* name, int64_t* total_mem, int* cu_count);
/* bytes the driver reports free / in total on `device` right now (hipMemGetInfo); blocks parked in this process's own
 * pool (emg3d_hip_cached_bytes) count as used there although the next handle may take them                          */
int emg3d_hip_mem_info(int device, int64_t* free_bytes, int64_t* total_bytes);

/* Device blocks of destroyed handles are kept for the next handle of the process (exact-size reuse, bounded by
 * EMG3D_POOL_GB, default 96; 0 disables): release them to the driver / ask how much is parked.            */
int64_t emg3d_hip_release_cached(void);
int64_t emg3d_hip_cached_bytes(void);
/* ... of which DEVICE memory parked for `device` (the pool also holds blocks of other devices of the process and pinned host
 * staging buffers, neither of which an allocation on `device` can take)                                              */
int64_t emg3d_hip_cached_bytes_on(int device);

/* ---- Tier 1: `emg3d.core` equivalents on host pointers ----------------- */

/* core.amat_x(rx,ry,rz, ex,ey,ez, eta_x,eta_y,eta_z, zeta, hx,hy,hz)
 * reference emg3d/core.py:29-177.  r -= A e, in place in r.               */
int emg3d_amat_x(int dtype, int64_t nx, int64_t ny, int64_t nz, void* r, const void* e,
                 const void* eta_x, const void* eta_y, const void* eta_z, const double* zeta,
                 const double* hx, const double* hy, const double* hz);

/* fields.get_h_field(grid, model, field), reference emg3d/fields.py:819-911: H = -curl E / (s mu_0) on the
 * faces, [hx|hy|hz] F-ordered (nNx,nCy,nCz), (nCx,nNy,nCz), (nCx,nCy,nNz).  zeta = V/mu_r when the model has
 * mu_r (fields.py:878-906), NULL otherwise.  (smu0_re, smu0_im) = field.smu0; real dtype: smu0_im = 0.   */
int emg3d_get_h_field(int dtype, int64_t nx, int64_t ny, int64_t nz, void* hfield, const void* efield,
                      const double* zeta, const double* hx, const double* hy, const double* hz,
                      double smu0_re, double smu0_im);

/* core.gauss_seidel (dir=0, core.py:181-474), core.gauss_seidel_x/_y/_z
 * (dir=1/2/3, core.py:477-753, 756-1037, 1040-1316): nu sweeps, in place. */
int emg3d_gauss_seidel(int dtype, int dir, int64_t nx, int64_t ny, int64_t nz, void* e,
                       const void* s, const void* eta_x, const void* eta_y, const void* eta_z,
                       const double* zeta, const double* hx, const double* hy, const double* hz,
                       int nu, int order);

/* core.restrict(crx,cry,crz, rx,ry,rz, wx,wy,wz, sc_dir), core.py:1586-1967.
 * w = [wxl,wx0,wxr, wyl,wy0,wyr, wzl,wz0,wzr] (host pointers).             */
int emg3d_restrict(int dtype, int64_t nx, int64_t ny, int64_t nz, int64_t cnx, int64_t cny,
                   int64_t cnz, void* cr, const void* r, const double* const* w, int sc_dir);

/* core.restrict_weights(vectorN, vectorCC, h, cvectorN, cvectorCC, ch),
 * core.py:1970-2041.  nh = len(h), n = len(cvectorN); O(n) host work.      */
int emg3d_restrict_weights(const double* vectorN, const double* vectorCC, const double* h,
                           int64_t nh, const double* cvectorN, const double* cvectorCC,
                           const double* ch, int64_t n, double* wl, double* w0, double* wr);

/* core.solve(amat, bvec), core.py:1447-1582: banded LDL^T, n unknowns.     */
int emg3d_solve(int dtype, void* amat, void* bvec, int64_t n);

/* core.blocks_to_amat(amat,bvec,middle,left,rhs,im,nC), core.py:1319-1444.
 * n = number of unknowns (len(bvec)); left is float64 as in the reference. */
int emg3d_blocks_to_amat(int dtype, void* amat, void* bvec, int64_t n, const void* middle,
                         const double* left, const void* rhs, int64_t im, int64_t nC);

/* solver.prolongation(grid, efield, cgrid, cefield, sc_dir),
 * solver.py:904-977 (+ RegularGridProlongator 1368-1463): e += P ce, then
 * ensure_pec.  Fine grid (nx,ny,nz; hx,hy,hz); sc_dir in 0..6.             */
int emg3d_prolongation(int dtype, int64_t nx, int64_t ny, int64_t nz, const double* hx,
                       const double* hy, const double* hz, const double* origin, void* e,
                       const void* ce, int sc_dir);

/* solver._restrict_model_parameters(param, sc_dir), solver.py:1747-1784.
 * is_complex selects the scalar type of param (eta: dtype, zeta: 0).       */
int emg3d_restrict_model(int is_complex, int64_t nx, int64_t ny, int64_t nz, void* cparam,
                         const void* param, int sc_dir);

/* Which line-sweep kernel the library selects for the colour launches (order 1; order 0: the hyperplane launches) of a level of
 * nx x ny x nz cells along dir (1, 2, 3 = x, y, z) on a device of cu_count compute units (<= 0: the current device) with nsys
 * batched systems -- the launch selection of the handle (reference: the one loop of core.gauss_seidel_x/_y/_z, emg3d/core.py:477-1316,
 * has no such choice) evaluated on the shape alone: no device memory, no launch, callable without a GPU when cu_count > 0.  The
 * selection lives in csrc/sweep_plan.hpp (plan_sweep): this call and the handle's launches read the same SweepPlan.
 * name (>= 64 bytes): the instantiation as emg3d_mg_last_sweep_kernel reports it; info[6]: lines of the largest colour, lines per
 * wave (thm: per pair of waves, tha / qpl: per workgroup), rounds of waves of that colour's launch, factor layout (0 one-sided 15
 * numbers per block, 3 mirrored two-sided, 4 compact 11 numbers), parity-split working copies (0 / 1), 64-bit field offsets (0 / 1). */
int emg3d_sweep_plan(int dtype, int64_t nx, int64_t ny, int64_t nz, int dir, int order, int nsys, int cu_count, char* name,
                     int64_t* info);

/* The same plan's answer on the scan tables of the scan kernel (csrc/sweep_plan.hpp, sweep_scantab; the arguments of
 * emg3d_sweep_plan, shape logic only, callable without a GPU when cu_count > 0): do the colour launches load the scanned map
 * matrices of every scan step from a table written when the factor is built?  A call of its own, so that callers of
 * emg3d_sweep_plan keep their six-entry buffers.  info[4]: table on (0 / 1), bytes of the four colours' tables (0: the kernel form
 * has none), quads per line (0: not the scan kernel), the threads of a colour launch up to which a table is admitted. */
int emg3d_sweep_scantab(int dtype, int64_t nx, int64_t ny, int64_t nz, int dir, int order, int nsys, int cu_count, int64_t* info);

/* How many forward steps of a half of a line keep their intermediate result z in LDS where the two-sided chain kernel
 * (k_line_sweep_thm) serves such a level -- csrc/sweep_plan.hpp, sweep_thm_zkeep; the arguments of emg3d_sweep_plan, shape logic only,
 * callable without a GPU when cu_count > 0 (a device with 160 KB of LDS per workgroup).  The kept steps neither write z to the field
 * nor read it back; results are bit-identical for every depth.
 * info[6]: steps a half may keep (0: another kernel serves, or the device refused the LDS), dynamic LDS bytes of a launch, static LDS
 * bytes of the instantiation, steps of the longest half, steps of that half actually kept (the first kept step is a multiple of the
 * prefetch depth), lines per pair of waves.                                                                                        */
int emg3d_sweep_thm_zkeep(int dtype, int64_t nx, int64_t ny, int64_t nz, int dir, int order, int nsys, int cu_count, int64_t* info);

/* How a smoothing call of npass colour passes along dir is ISSUED on such a level (csrc/sweep_plan.hpp, plan_fuse): one launch per
 * pass, or -- levels of short lines that the scan kernel serves -- all passes in one launch of that kernel, a workgroup per slab of
 * line nodes along the longer transverse axis working on a private copy, plus one launch that writes every edge from its owner's copy.
 * The kernel selection (emg3d_sweep_plan) is the same either way.  own > 0: own line nodes per slab instead of the default;
 * max_seg > 0: fused up to lines of that many blocks (a power of two) instead of the default (8-block lines: lab build only); budget > 0: bytes the private copies may take instead of the default.  Shape logic only, callable without a GPU when cu_count > 0.
 * info[8]: fused (0 / 1), slab axis (0, 1, 2 = x, y, z), cells nX along it (lines at the nodes 1 .. nX - 1), own nodes per slab, slabs,
 * passes, waves per workgroup, bytes of private copies.  ranges (may be NULL; nranges = its capacity, >= slabs * (4 + 2 npass)), per
 * slab: own nodes [x0, x1), owned edge indices [a, b) along the axis (nodes 0 .. nX and cells 0 .. nX - 1 alike), then per pass the
 * live nodes lo, hi (inclusive).  Written only when fused.                                                                        */
int emg3d_sweep_fuse_plan(int dtype, int64_t nx, int64_t ny, int64_t nz, int dir, int order, int nsys, int cu_count, int npass, int own,
                          int max_seg, int64_t budget, int64_t* info, int64_t* ranges, int64_t nranges);

/* ---- Tier 2: device-resident multigrid handle --------------------------- */
typedef struct emg3d_mg emg3d_mg_t;

/* Builds the level-0 state on `device`: uploads h, eta, zeta; origin[3]
 * (or NULL = 0) is the grid origin (node coordinates enter the transfer
 * weights exactly as in the reference, solver.py:859-864).
 * (VolumeModel outputs, models.py:554-658, are inputs here.)               */
int emg3d_mg_create(emg3d_mg_t** out, int dtype, int64_t nx, int64_t ny, int64_t nz,
                    const double* hx, const double* hy, const double* hz, const double* origin,
                    const void* eta_x, const void* eta_y, const void* eta_z, const double* zeta,
                    int device);
/* Same handle from the FREQUENCY-INDEPENDENT model: sv_* = conductivity * cell volume (real,
 * F-ordered (nCx,nCy,nCz); sv_y / sv_z may alias sv_x or be NULL) and the scalar
 * smu0 = s*mu_0 (= -2 pi i f mu_0, or f mu_0 in the Laplace domain; imaginary part ignored for
 * dtype 0): eta = smu0 * sv is formed on the device (models.py:631-658 without epsilon_r).  The
 * ranks of a frequency shard (simulations.py:840-867) share sv and differ in one scalar.      */
int emg3d_mg_create_sv(emg3d_mg_t** out, int dtype, int64_t nx, int64_t ny, int64_t nz, const double* hx,
                       const double* hy, const double* hz, const double* origin, const double* sv_x,
                       const double* sv_y, const double* sv_z, const double* zeta, double smu0_re,
                       double smu0_im, int device);

/* The same with the conductivities and the cell volumes as separate arrays: eta = (s mu_0 V) sigma is formed on the device
 * exactly as VolumeModel rounds it (reference models.py:631-658, `(smu0 * vol) * sigma`), so that a handle -- also one
 * re-targeted with emg3d_mg_set_smu0 -- holds bit for bit the eta of the reference at every frequency.  s mu_0 must be
 * purely imaginary (dtype 1) or real (dtype 0): -2 otherwise.
 * `map`: the property map of the three arrays, which hold the model's own parameter p; the device forms sigma = backward(p)
 * (k_sigma_of_map, reference emg3d/maps.py:319-448):
 *     0 conductivity        sigma = p          (the arrays are taken as they are)
 *     1 resistivity         sigma = 1 / p      (an IEEE division: Model.conductivity's bits)
 *     2 log10 conductivity  sigma = 10^p
 *     3 ln conductivity     sigma = e^p
 *     4 log10 resistivity   sigma = 10^-p
 *     5 ln resistivity      sigma = e^-p
 * 2-5 use the device's exp10 / exp, within a few ulp of NumPy's; emg3d_mg_get_sigma returns what the device
 * holds.  Any other code: -2.                                                                                            */
int emg3d_mg_create_vs(emg3d_mg_t** out, int dtype, int64_t nx, int64_t ny, int64_t nz, const double* hx,
                       const double* hy, const double* hz, const double* origin, const double* sigma_x,
                       const double* sigma_y, const double* sigma_z, const double* vol, const double* zeta,
                       double smu0_re, double smu0_im, int map, int device);
/* ... and with displacement currents (Model.epsilon_r): eta = s mu_0 V (sigma - s eps_0 eps_r), reference
 * models.py:639-647, formed on the device as NumPy rounds it.  seps0 = s eps_0 (dtype 0) resp. Im(s) eps_0 (dtype 1: s is
 * purely imaginary, and so is s mu_0 = i smu0_im).  Another frequency: emg3d_mg_set_smu0_eps.                        */
int emg3d_mg_create_vse(emg3d_mg_t** out, int dtype, int64_t nx, int64_t ny, int64_t nz, const double* hx,
                        const double* hy, const double* hz, const double* origin, const double* sigma_x,
                        const double* sigma_y, const double* sigma_z, const double* vol, const double* zeta,
                        const double* epsilon_r, double smu0_re, double smu0_im, double seps0, int map, int device);
void emg3d_mg_destroy(emg3d_mg_t* mg);

/* Cycle parameters = the MGParameters fields used inside solver.multigrid
 * (solver.py:1043-1113): cycle 'V'/'W'/'F' as char code, nu_*, clevel[4] =
 * MGParameters.clevel after max_level (solver.py:1142-1173), order as above. */
int emg3d_mg_set_params(emg3d_mg_t* mg, int cycle, int nu_init, int nu_pre, int nu_coarse,
                        int nu_post, const int* clevel, int order);

int emg3d_mg_set_sfield(emg3d_mg_t* mg, const void* sfield_host);
/* Source from the real, frequency-independent source vector: s = smu0 * vector (fields.py:624,
 * `SourceField.vector`); uploads 8 instead of 16 bytes per edge.  Overwrites the residual buffer. */
int emg3d_mg_set_sfield_vector(emg3d_mg_t* mg, const double* vector, double smu0_re, double smu0_im);
/* Source of ONE finite electric dipole src6 = (x0, x1, y0, y1, z0, z1) built in HBM (fields.get_source_field for
 * a finite dipole, reference fields.py:586-629; the edge distribution _finite_source_xyz, fields.py:914-1010, runs
 * on the device): s (+)= scale_c * weights_c per component, scale6 = (re, im) x 3 = moment_c * s mu_0 (fields.py:624;
 * imaginary parts ignored by float64 handles); coordinates and nodes are rounded to `decimals` as in the reference;
 * accumulate != 0 adds to the present source (arbitrarily shaped dipoles, fields.py:575-580).  sums3 (may be NULL)
 * receives the three weight sums (1 for a source inside the grid; |sum - 1| > 1e-6 triggers the reference's
 * normalisation).  Returns -4 when the source lies outside the grid (the reference raises ValueError).
 * A point dipole [x, y, z, azimuth, dip] is turned into a finite one by the caller (fields.py:1037-1040).     */
int emg3d_mg_set_sfield_dipole(emg3d_mg_t* mg, const double* src6, const double* scale6, int decimals,
                               int accumulate, double* sums3);
/* The same as a stateless call that returns the source field on the host ([fx|fy|fz], nE entries of dtype). */
int emg3d_source_field(int dtype, int64_t nx, int64_t ny, int64_t nz, const double* hx, const double* hy,
                       const double* hz, const double* origin, const double* src6, const double* scale6,
                       int decimals, void* sfield, double* sums3);
int emg3d_mg_set_efield(emg3d_mg_t* mg, const void* efield_host); /* NULL -> zeros */
int emg3d_mg_get_efield(emg3d_mg_t* mg, void* efield_host);
int emg3d_mg_get_residual(emg3d_mg_t* mg, void* rfield_host);     /* r = s - A e */
/* fields.get_h_field (fields.py:819-911) of the device-resident level-0 electric field; use_zeta != 0 when
 * the model has mu_r.  48 instead of 96+ bytes per cell over PCIe.  Overwrites the residual buffer.      */
int emg3d_mg_get_hfield(emg3d_mg_t* mg, int use_zeta, double smu0_re, double smu0_im, void* hfield_host);

/* ---- receivers ----------------------------------------------------------------------
 * maps.interp3d(points, values, new_points, method, fill_value, mode='constant', cval), reference
 * emg3d/maps.py:179-276, on the device: values F-ordered (nx,ny,nz) of dtype on the regular grid px,py,pz;
 * xi = [x[n] | y[n] | z[n]]; method 0 = 'linear' (RegularGridInterpolator, bounds_error=False; has_fill = 0 means
 * fill_value=None: extrapolate), 1 = 'cubic' (the SciPy arithmetic the reference calls: not-a-knot index spline +
 * cubic B-spline prefilter + 4x4x4 evaluation; points outside get cval, complex: cval + cval j); fewer than 4 points
 * along an axis force 'linear' (maps.py:238-240); 2 / 3 / 4 = 'cubic' with xi already in INDEX coordinates of `values`
 * (px, py, pz unused): how the binding serves map_coordinates' boundary modes 'mirror' (2: stencil indices mirrored;
 * also 'wrap', whose coordinates the caller wraps with period n - 1 first: SciPy's legacy rule), 'nearest' (3: values
 * edge-padded by 12 samples by the caller; "reflect" prefilter initialisation, stencil indices clamped to the array) and
 * 'reflect' (4: "reflect" prefilter initialisation, stencil indices reflected); no point is outside in any of them -- the
 * O(n) index spline on the host, prefilter and evaluation over the whole array here.  The stateless entry points run on
 * the calling thread's current device.                                                                                    */
int emg3d_interp3d(int dtype, int64_t nx, int64_t ny, int64_t nz, const double* px, const double* py,
                   const double* pz, const void* values, int64_t n, const double* xi, int method, int has_fill,
                   double fill_value, double cval, void* out);
/* fields.get_receiver_response(grid, field, rec), reference emg3d/fields.py:733-817: the field at n point
 * receivers, resp[r] = sum_c factors[c][r] * interp3d(points_c[1:-1], field_c[1:-1,1:-1,1:-1], (x,y,z)[r], 'cubic',
 * 0.0, 'constant', nan).  xyz = [x[n] | y[n] | z[n]]; factors = [fx[n] | fy[n] | fz[n]] = fields._rotation(azimuth,
 * dip) (fields.py:1013-1034, evaluated by the caller); a component whose factors are all <= 1e-10 is skipped
 * (fields.py:810).  field: [fx|fy|fz] of an electric (is_electric != 0) or magnetic field on the host.        */
int emg3d_get_receiver_response(int dtype, int64_t nx, int64_t ny, int64_t nz, const double* hx, const double* hy,
                                const double* hz, const double* origin, const void* field, int is_electric,
                                int64_t n, const double* xyz, const double* factors, void* resp);
/* Same on the device-resident level-0 electric field of a handle (magnetic != 0: on H = get_h_field(E),
 * fields.py:819-911, formed on the device; use_zeta / smu0 as in emg3d_mg_get_hfield): 16 bytes per receiver
 * cross PCIe instead of the field.  Overwrites the residual buffer when magnetic != 0.                      */
int emg3d_mg_get_receiver_response(emg3d_mg_t* mg, int magnetic, int use_zeta, double smu0_re, double smu0_im,
                                   int64_t n, const double* xyz, const double* factors, void* resp);

/* ---- adjoint-state gradient ------------------------------------------------------------
 * maps.edges2cellaverages(ex, ey, ez, vol, out_x, out_y, out_z), reference emg3d/maps.py:578-630: edge values to
 * volume-weighted cell averages, ADDED into out_x/y/z (F-ordered (nx,ny,nz) of dtype, host); field = [fx|fy|fz].  */
int emg3d_edges2cellaverages(int dtype, int64_t nx, int64_t ny, int64_t nz, const void* field, const double* vol,
                             void* out_x, void* out_y, void* out_z);
/* optimize.gradient for ONE (source, frequency) pair on its computational grid, reference
 * emg3d/optimize.py:176-199: grad = sum_c edges2cellaverages_c(-Re(bfield * efield * smu0)) with the cell volumes
 * of the handle's grid.  bfield = the handle's level-0 field (the back-propagated solution, simulations.py:1131-1143),
 * efield = workspace vector `efield_vec` (the forward solution, saved with emg3d_mg_vec_copy(id, -2)).  grad: nC
 * doubles, F-ordered.  (The reference then maps -grad to the model grid: emg3d_interp3d_grid, optimize.model_gradient.)
 * Overwrites the residual buffer.                                                                                */
int emg3d_mg_gradient(emg3d_mg_t* mg, int efield_vec, double smu0_re, double smu0_im, double* grad);
/* The same with the three components kept apart: grad_x, grad_y, grad_z (nC doubles each); (grad_x + grad_y) + grad_z is
 * emg3d_mg_gradient's result bit for bit.                                                                               */
int emg3d_mg_gradient3(emg3d_mg_t* mg, int efield_vec, double smu0_re, double smu0_im, double* grad_x, double* grad_y,
                       double* grad_z);

/* Survey gradient (optimize.survey_gradient): the gradients of ALL systems of a batched handle, summed on the device.  The
 * accumulator is a buffer of nC doubles of the handle's own (NOT the residual buffer emg3d_mg_gradient stages in): allocated on
 * first use, counted by emg3d_mg_device_bytes, freed with the handle; cycles, emg3d_mg_set_smu0 and emg3d_mg_set_mask leave it alone.
 *   grad_acc_reset: allocates the accumulator if need be and zeroes it.
 *   grad_acc_add  : acc = (((acc + g_0) + g_1) + ...) over the systems b = 0 .. nsys-1 in ascending order with use[b] != 0
 *                   (use: nsys flags), in ONE launch, one read and one write of acc per cell, no atomics; g_b is bit for bit what
 *                   emg3d_mg_gradient returns for system b -- forward field = slice b of the batched vector `fwd_bvec` (saved with
 *                   emg3d_mg_bvec_copy(id, -2); -2 for a bad id or fwd_bvec < 0: a saved copy, not the live field, as
 *                   emg3d_mg_gradient asks), back-propagated field = slice b of the level-0 field array.  Works on handles
 *                   with one system too.
 *   grad_acc_get  : the accumulator, nC doubles, F-ordered.                                                             */
int emg3d_mg_grad_acc_reset(emg3d_mg_t* mg);
int emg3d_mg_grad_acc_add(emg3d_mg_t* mg, int fwd_bvec, double smu0_re, double smu0_im, const int32_t* use);
int emg3d_mg_grad_acc_get(emg3d_mg_t* mg, double* out);
/* The same per direction (optimize.SurveyJacobian, components=True): three accumulators of nC doubles each, of the handle's own like
 * the one above and independent of it (allocated on first use, counted by emg3d_mg_device_bytes, freed with the handle).
 *   grad_acc3_add: acc_c = (((acc_c + g_c,0) + g_c,1) + ...) for c = x, y, z over the used systems in ascending order, ONE launch;
 *                  g_c,b is bit for bit what emg3d_mg_gradient3 returns for system b (fields as for grad_acc_add, -2 likewise).
 *   grad_acc3_get: the three accumulators, nC doubles each, F-ordered.                                                      */
int emg3d_mg_grad_acc3_reset(emg3d_mg_t* mg);
int emg3d_mg_grad_acc3_add(emg3d_mg_t* mg, int fwd_bvec, double smu0_re, double smu0_im, const int32_t* use);
int emg3d_mg_grad_acc3_get(emg3d_mg_t* mg, double* out_x, double* out_y, double* out_z);
/* Survey sensitivity diagonal (optimize.SurveyJacobian.sensitivity_diagonal): diag(J^H W J) = sum over the data d of W_d |J_dj|^2.
 * The operator is complex symmetric, so row (source s, receiver r) of J at a cell is c = c_x + c_y + c_z with
 * c_c = edges2cellaverages_c(s mu_0 lambda_r E_s), lambda_r the solution for receiver r's adjoint source alone (it serves every
 * source) and E_s the forward field: an all-pairs product of two sets of fields, complex before it is squared.
 *   sens_acc_add: acc += weights[b_adj * nsys + b_fwd] * |(c_x + c_y) + c_z|^2 over the pairs, in ONE launch, one read and one write
 *                 of acc per cell, no atomics -- adjoint systems b_adj with use_adj[b_adj] != 0 in ascending order (outer loop;
 *                 lambda = slice b_adj of the level-0 field array), forward systems b_fwd with use_fwd[b_fwd] != 0 in ascending order
 *                 (inner loop; E = slice b_fwd of the batched vector `fwd_bvec`, a saved copy as for grad_acc_add); a pair whose
 *                 weight is 0 is skipped and contributes exactly nothing.  split = 0: into the accumulator of grad_acc_*;
 *                 split != 0: W |c_x|^2, W |c_y|^2, W |c_z|^2 into the three of grad_acc3_*.  grad_acc(3)_reset and _get serve
 *                 unchanged.  use_fwd, use_adj: nsys flags each; weights: nsys * nsys doubles, uploaded by the call into a table of
 *                 the handle's own (allocated at the first call, counted by emg3d_mg_device_bytes).  -2: a bad fwd_bvec, an
 *                 accumulator that was never reset, a weight that is not finite.                                           */
int emg3d_mg_sens_acc_add(emg3d_mg_t* mg, int fwd_bvec, double smu0_re, double smu0_im, const int32_t* use_fwd,
                          const int32_t* use_adj, const double* weights, int split);
/* Explicit rows of J (optimize.SurveyJacobian.sensitivity_rows): what sens_acc_add squares, kept.  Every pair of an adjoint system
 * (use_adj[b_adj] != 0) and a forward system (use_fwd[b_fwd] != 0) is a row; pair number p is its rank in sens_acc_add's loop order
 * (adjoint systems ascending, outer; forward systems ascending, inner); there is no weight table.  Fields as for sens_acc_add:
 * lambda = slice b_adj of the level-0 field array, E = slice b_fwd of the batched vector `fwd_bvec` (a saved copy).
 *   sens_rows_count: the number of pairs of two masks of nsys flags (1 <= nsys <= 64), pure host arithmetic; -2 for bad arguments.
 *   sens_rows      : out (host) <- [p][dir][part][cell] doubles, planar: dir = one plane (c_x + c_y) + c_z, split != 0: the three
 *                    c_x, c_y, c_z; part = re, im for a complex128 handle, one plane for a float64 handle; cells F-ordered.  `out`
 *                    holds sens_rows_count * (split ? 3 : 1) * (complex ? 2 : 1) * cells doubles.  ONE launch writes all rows into
 *                    a buffer of the handle's own, every element once, no atomics; entry for entry the value whose square
 *                    sens_acc_add adds.  on_model_grid != 0 (needs emg3d_mg_set_model_grid and emg3d_mg_set_regrid_factors, -7
 *                    otherwise): every plane y becomes Q_dir (.) A^T (F_dir (.) y) on the model grid (cells = nM) with the launch
 *                    of grad_acc(3)_get_model, one plane after the other, into a second buffer; without split the factors of
 *                    direction x are used, which is the row only if the three directions share their factors (-2 otherwise).
 *                    Then ONE copy to the host.  The two buffers are optional memory like the batched vectors: each grows to the
 *                    largest call so far, is counted by emg3d_mg_device_bytes and freed with the handle; one that does not fit
 *                    answers hipErrorOutOfMemory (2) and the handle stays usable.  -2: a bad fwd_bvec (fwd_bvec < 0 included: a
 *                    saved copy, not the live field), a mask without a used system.                                            */
int64_t emg3d_mg_sens_rows_count(const int32_t* use_fwd, const int32_t* use_adj, int nsys);
int emg3d_mg_sens_rows(emg3d_mg_t* mg, int fwd_bvec, double smu0_re, double smu0_im, const int32_t* use_fwd, const int32_t* use_adj,
                       int split, int on_model_grid, double* out);

/* ---- row store (solver.DeviceRows, optimize.SurveyJacobian.park_rows) ----------------------------------------------
 * n_rows x n_cols doubles, row-major, on one device, in ONE block of its own (a quiet allocation, never a piece of a handle's
 * arena), and the dense products a data-space method takes from rows of J that stay in HBM.  A store belongs to no handle: the
 * handles of a survey (complex128 for its frequencies, float64 for its Laplace-domain entries) park into the same store.
 *   rows_create   : checks n_rows * n_cols * 8 bytes (rounded up to 256) against emg3d_hip_mem_info (free + what the handles' pool
 *                   holds on that device) BEFORE it allocates: a store that cannot fit answers hipErrorOutOfMemory (2) without an
 *                   attempt.  -2: n_rows < 1, n_cols < 1, out NULL.
 *   rows_bytes    : the block's bytes; plus those of the chain factors once set, and of the products' workspace (operands, slab
 *                   partials, results: one more block, at most 256 MiB of partials, that grows to the largest product so far and is
 *                   kept, because allocating it per call costs more than the kernels).
 *   rows_set / rows_get: row i <- / -> n_cols doubles of the host.  -2: i outside 0 .. n_rows - 1, a NULL pointer.
 *   rows_set_chain: three arrays of n doubles (host), kept on the device for sens_rows_park(chain != 0); n = 0 frees them.
 *   sens_rows_park: emg3d_mg_sens_rows up to its copy to the host -- the same checks (-2, -7, 2), the same launch into the handle's
 *                   row buffer, the same model-grid launches --, then ONE launch (k_rows_park) writes plane part = 0 (the real part)
 *                   of pair p into store row dest[p]; dest[p] < 0 skips the pair; no two pairs may name the same row.  A store row's
 *                   columns are [dir][cell], cells F-ordered: n_cols = cells (split = 0, or sum3) or 3 * cells.  chain != 0:
 *                   direction q is written as chain_q[cell] * value; sum3 != 0 (needs split): one plane (p0 + p1) + p2 of the (scaled)
 *                   directions.  No contraction: with the operations of SurveyJacobian.sensitivity_rows in their order, a parked
 *                   row equals the row that returns, bit for bit.  The handle's stream is synchronised before the call returns, so
 *                   every later operation of the store sees the rows.  -2 also: a store on another device or of another n_cols, a
 *                   dest[p] >= n_rows, chain without factors of `cells` entries.
 *   sens_rows_fill: BOTH parts of the same rows into the store: the real part of pair p into row dest_re[p], the imaginary part into
 *                   row dest_im[p] (dest_im NULL: real parts only), a negative entry skips that part, and a pair with both
 *                   negative is not computed.  Columns, chain and sum3 as for sens_rows_park, the same operations in the same
 *                   order: part 0 is what sens_rows_park parks bit for bit, part 1 the imaginary plane of emg3d_mg_sens_rows
 *                   through the same real operations.  on_model_grid = 0: ONE launch (k_sens_rows_fill) from the fields into the
 *                   store -- the handle's row buffer is neither allocated nor grown.  on_model_grid != 0: the launches of
 *                   emg3d_mg_sens_rows, then k_rows_park once per part.  The handle's stream is synchronised before the call
 *                   returns.  The codes of sens_rows_park (-2, -7; 2 on the model-grid path); -2 also: dest_re NULL, a dest_im
 *                   on a float64 handle, a row named twice (in one table or across the two), every entry negative.  A
 *                   refused call writes nothing.
 *   rows_gram     : G (host, n_rows^2 doubles) <- R diag(cm) R^T, G[a][b] = sum_j R[a][j] cm[j] R[b][j]; cm: n_cols doubles (host) or
 *                   NULL (= 1).  k_rows_gram: v_mfma_f64_16x16x4_f64, one workgroup per K-slab of columns and pair of row blocks
 *                   (rows_gram_plan), cm multiplied into one operand while staging; the slab partials are summed in ascending slab
 *                   order by k_rows_gram_reduce, which writes the lower triangle and its mirror.  No atomics: G is the same bits
 *                   at every call, G == G^T exactly, and the slab partition follows from n_cols alone, so that without cm (or with a
 *                   cm whose products cm[j] R[b][j] are exact) a store with its rows permuted gives the permuted G bit for bit; with
 *                   a general cm the factor sits on the row of the smaller index, and a permuted pair agrees to rounding only.
 *   rows_matvec   : out (host, n_rows) <- R v, v: n_cols doubles (host); per row and slab a fixed tree, the slab partials summed in
 *                   ascending order: deterministic.
 *   rows_rmatvec  : out (host, n_cols) <- cm (.) R^T y: per column acc = acc + y[i] * R[i][j] over the rows ascending, then
 *                   cm[j] * acc (cm NULL: acc), every operation rounded once -- bit for bit that loop on the host.
 *   rows_gram_plan: host arithmetic, needs no GPU.  out[8] <- rows per block, columns staged per step, columns per K-slab, slabs,
 *                   row blocks, jobs (pairs of row blocks ba >= bb), workgroups (jobs * slabs), LDS bytes per workgroup.  The slab
 *                   length is a function of n_cols alone.  rows_gram_job: out[4] <- the rows [a0, a1) x [b0, b1) of job `job`; a
 *                   diagonal job (a0 == b0) computes the 16 x 16 tile pairs ta >= tb of its block only.  -2: bad arguments.
 *   rows_gram_batch: host arithmetic, needs no GPU; what rows_gram itself runs.  out[4] <- jobs per launch, launches, bytes of one
 *                   job's slab partials (64 tile pairs x slabs x 256 doubles), bytes of partials held at a time.  The jobs run in
 *                   their order, as many per launch as fit the partials' bytes and at least one; jobs per launch depends on
 *                   n_rows through the number of jobs only.  -2: bad arguments.   */
typedef struct emg3d_rows emg3d_rows_t;
int emg3d_rows_create(int device, int64_t n_rows, int64_t n_cols, emg3d_rows_t** out);
void emg3d_rows_destroy(emg3d_rows_t* rows);
int64_t emg3d_rows_bytes(const emg3d_rows_t* rows);
int emg3d_rows_set(emg3d_rows_t* rows, int64_t i, const double* host);
int emg3d_rows_get(emg3d_rows_t* rows, int64_t i, double* host);
int emg3d_rows_set_chain(emg3d_rows_t* rows, int64_t n, const double* cx, const double* cy, const double* cz);
int emg3d_mg_sens_rows_park(emg3d_mg_t* mg, int fwd_bvec, double smu0_re, double smu0_im, const int32_t* use_fwd, const int32_t* use_adj,
                            int split, int on_model_grid, emg3d_rows_t* rows, const int32_t* dest, int chain, int sum3);
int emg3d_mg_sens_rows_fill(emg3d_mg_t* mg, int fwd_bvec, double smu0_re, double smu0_im, const int32_t* use_fwd, const int32_t* use_adj,
                            int split, int on_model_grid, emg3d_rows_t* rows, const int32_t* dest_re, const int32_t* dest_im, int chain,
                            int sum3);
int emg3d_rows_gram(emg3d_rows_t* rows, const double* cm, double* G);
int emg3d_rows_matvec(emg3d_rows_t* rows, const double* v, double* out);
int emg3d_rows_rmatvec(emg3d_rows_t* rows, const double* y, const double* cm, double* out);
int emg3d_rows_gram_plan(int64_t n_rows, int64_t n_cols, int64_t* out);
int emg3d_rows_gram_job(int64_t n_rows, int64_t job, int64_t* out);
int emg3d_rows_gram_batch(int64_t n_rows, int64_t n_cols, int64_t* out);

/* ---- a small dense matrix times the store (solver.DeviceRows.project / colsumsq; optimize.RowStore.project,
 *      resolution_diagonal, posterior_variance) -----------------------------------------------------------------------
 * rows_gram contracts over the columns; rows_project contracts over the ROWS: Y[m x n_cols] = M[m x n_rows] R, every column on its
 * own, no split over k, no partials, no second pass; the result is a store.
 *   rows_project     : dst <- M src.  M: m x src.n_rows doubles of the host, row-major; dst: another store on the same device with
 *                      n_rows == m and n_cols == src.n_cols -- anything else (dst == src included: there is no in-place mode)
 *                      answers -2.  M goes through src's workspace; runs on src's stream, synchronised before it returns; src is
 *                      not modified.  k_rows_project: v_mfma_f64_16x16x4_f64, one workgroup per panel of columns and block of
 *                      output rows (rows_project_plan), which walks ALL rows of src in ascending steps with its accumulators in
 *                      registers and writes every element once; each block of output rows is one pass over src.  The contract:
 *                        deterministic -- the same bits at every call (no atomics);
 *                        local -- Y[i][j] depends on row i of M and column j of src and on nothing else: it is one accumulation
 *                          chain over k = 0 .. n_rows - 1 in groups of four (one MFMA each), padded with zeros, whatever m and
 *                          n_cols are and wherever the row sits in M and the column in the store.  Rows of M permuted give the
 *                          rows of Y permuted, a store of some of the columns gives those columns of Y, a NaN in one column of src
 *                          stays in that column of Y;
 *                        the order of the four products inside one instruction is the hardware's, so Y is NOT bit for bit a loop
 *                          on the host; against exact arithmetic |Y - M R| <= gamma_(n_rows + 2) |M| |R| per element.
 *   rows_colsumsq    : out (host, n_cols) <- sum_i s[i] R[i][j]^2; s: n_rows doubles (host) or NULL (= 1).  One thread per column:
 *                      acc = acc + s[i] * (R[i][j] * R[i][j]) over the rows ascending (s NULL: acc + R[i][j] * R[i][j]), every
 *                      operation rounded once -- bit for bit that loop on the host.
 *   rows_project_plan: host arithmetic, needs no GPU; the launch calls the same function.  out[8] <- output rows per block, columns
 *                      per workgroup, source rows (k) per step, passes over the source = ceil(m / rows per block), workgroups
 *                      (passes * panels), LDS bytes of the largest workgroup, panels = ceil(n_cols / columns per workgroup), the
 *                      rows the last block's kernel covers (32, 64, 128 or a whole block: a block with fewer live rows stages and
 *                      multiplies fewer).  The panels are a function of n_cols alone.  -2: a size < 1, out NULL.           */
int emg3d_rows_project_plan(int64_t n_rows, int64_t m, int64_t n_cols, int64_t* out);
int emg3d_rows_project(emg3d_rows_t* src, const double* M, int64_t m, emg3d_rows_t* dst);
int emg3d_rows_colsumsq(emg3d_rows_t* rows, const double* s, double* out);

/* ---- smoothing model covariance (maps.SmoothingCovariance, optimize.RowStore.with_covariance) ----------------------
 * C = L L^T with L = diag(w) S^p, S = S_z S_y S_x, S_axis = T^-1 one implicit diffusion step along an axis: T the symmetric
 * tridiagonal matrix I + ell^2 H^-1/2 D^T diag(1/d) D H^-1/2 of the axis' cell widths h, centre distances d and correlation
 * length ell (Neumann ends; smallest eigenvalue 1).  The caller factorises T once on the host (maps.SmoothingCovariance: lo, cp,
 * inv, n doubles per axis) and the library solves one line a[0 .. n-1] by sequential Thomas, every operation rounded once:
 *     a[0] = a[0] * inv[0];   a[i] = (a[i] - lo[i] * a[i-1]) * inv[i], i = 1 .. n-1;   a[i] = a[i] - cp[i] * a[i+1], i = n-2 .. 0.
 * L^T on an array of nx x ny x nz doubles (x fastest): a = w * a if a scale is given; then for x, y, z in this order the solve
 * `passes` times in a row on every line of the axis.  L runs the same sweeps and multiplies by w last.  An axis whose three
 * factor pointers are NULL, or of length 1, is skipped.  The result equals that loop in numpy BIT FOR BIT whichever kernel runs
 * it (k_rows_smooth_*: a line stays in LDS between its sweeps and passes, so that an axis reads and writes the data once; a line
 * that no LDS holds goes one thread per line through HBM).
 *   rows_smooth_plan: host arithmetic, needs no GPU.  out[6] <- path of `axis` (0, 1, 2 = x, y, z) on arrays of nx x ny x nz: 0 the
 *                     line is resident in LDS, 1 through HBM; lines per workgroup; LDS bytes per workgroup; workgroups PER ARRAY
 *                     (a launch has that many times the number of arrays); the least lines a workgroup of path 0 takes (path 1
 *                     is chosen exactly when the LDS cannot hold that many); lines per array.  -2: bad arguments.
 *   smooth3d        : stateless: data (host, n_arrays arrays back to back) is uploaded, smoothed by the same kernels and
 *                     downloaded.  scale: nx * ny * nz doubles (host) for every array, or NULL; scale_after = 0: L^T, 1: L.
 *                     -2: a size < 1, passes < 1, data NULL, an axis with some but not all of its factors.
 *   rows_smooth     : L^T on every row of a store in place; a row is `planes` arrays of nx x ny x nz, each smoothed on its own;
 *                     scale: n_cols doubles (host) or NULL.  Factors and scale go through the store's workspace; runs on the
 *                     store's stream, synchronised before it returns.  -2: nx * ny * nz * planes != n_cols, passes < 1, ...
 *   rows_smooth_l   : the same arguments and answers; L instead of L^T on every row: the same sweeps, then the scale multiplied in
 *                     on the way out of the last active axis (k_rows_smooth_*'s w_post; the scale kernel where no axis is active).
 *                     Bit for bit SmoothingCovariance.sqrt(row, host=True).
 *   rows_clone      : *out <- a second store of the same size on the same device with the same rows (device to device; the chain
 *                     factors are not copied).  The memory check and the answers of rows_create.                             */
int emg3d_rows_smooth_plan(int64_t nx, int64_t ny, int64_t nz, int axis, int64_t* out);
int emg3d_smooth3d(int device, int64_t n_arrays, int64_t nx, int64_t ny, int64_t nz, const double* scale, const double* lo_x,
                   const double* cp_x, const double* inv_x, const double* lo_y, const double* cp_y, const double* inv_y,
                   const double* lo_z, const double* cp_z, const double* inv_z, int passes, int scale_after, double* data);
int emg3d_rows_smooth(emg3d_rows_t* rows, int64_t nx, int64_t ny, int64_t nz, int planes, const double* scale, const double* lo_x,
                      const double* cp_x, const double* inv_x, const double* lo_y, const double* cp_y, const double* inv_y,
                      const double* lo_z, const double* cp_z, const double* inv_z, int passes);
int emg3d_rows_smooth_l(emg3d_rows_t* rows, int64_t nx, int64_t ny, int64_t nz, int planes, const double* scale, const double* lo_x,
                        const double* cp_x, const double* inv_x, const double* lo_y, const double* cp_y, const double* inv_y,
                        const double* lo_z, const double* cp_z, const double* inv_z, int passes);
int emg3d_rows_clone(emg3d_rows_t* rows, emg3d_rows_t** out);

/* ---- sensitivity products (optimize.Jacobian) --------------------------------------------------------------------
 * The reference (v0.17.0) has the gradient only; these are the pieces of J v and J^T w with J = d(data) / d(conductivity) for
 * one (source, frequency) pair.  With A e = s the system of core.amat_x (the sigma-term of an edge is -1/4 (eta of its four
 * cells) e, eta = s mu_0 sigma V; reference emg3d/core.py:149-177) and E the forward field:
 *   J v   = P de,   A de = s mu_0 C(v) o E,   C(v)[edge] = 1/4 sum of V_c v_c over the four cells around the edge;
 *   J^T w = -sum_c edges2cellaverages_c(-Re(s mu_0 lambda E)) = -emg3d_mg_gradient,   A lambda = P^T conj(w).
 * maps.cellaverages2edges: the exact transpose of emg3d_edges2cellaverages (boundary edges count their cell two or four times,
 * as there): out_c[edge] += sum vol v_c / 4; v_* F-ordered (nx,ny,nz) of dtype, out_* the components of a field of dtype (host);
 * a NULL v_c leaves out_c alone.                                                                                       */
int emg3d_cells2edges(int dtype, int64_t nx, int64_t ny, int64_t nz, const void* vx, const void* vy, const void* vz,
                      const double* vol, void* out_x, void* out_y, void* out_z);
/* Source of the selected system <- s mu_0 C(v) o E, E = workspace vector `efield_vec` (>= 0), per component with that
 * component's perturbation vx / vy / vz (host, nC doubles, F-ordered; NULL: the component's source is zero; the same pointer
 * for several directions is uploaded once); PEC boundary edges are written as exact zeros.  One thread per edge gathers its
 * four cells: deterministic.  Overwrites the residual buffer.                                                          */
int emg3d_mg_jvec_source(emg3d_mg_t* mg, int efield_vec, double smu0_re, double smu0_im, const double* vx, const double* vy,
                         const double* vz);
/* The same for the systems of a batched handle that share ONE perturbation and have a forward field each (optimize.SurveyJacobian):
 * source of every system b with use[b] != 0 (use: nsys flags) <- s mu_0 C(v) o E_b, E_b = slice b of the batched vector `fwd_bvec`
 * (saved with emg3d_mg_bvec_copy(id, -2); -2 for a bad id or fwd_bvec < 0: a saved copy, not the live field), in ONE launch: a thread
 * forms C(v) of its edge once and loops over the used systems.  Slice b of the source array is bit for bit what emg3d_mg_jvec_source
 * writes for the selected system b with the same field; PEC boundary edges of the used systems are exact zeros; the sources of the
 * other systems are not touched.  v is uploaded once per call.  Per edge and used system sizeof(dtype) bytes are read and
 * sizeof(dtype) written.  Overwrites the residual buffer.                                                                    */
int emg3d_mg_jvec_source_b(emg3d_mg_t* mg, int fwd_bvec, double smu0_re, double smu0_im, const double* vx, const double* vy,
                           const double* vz, const int32_t* use);
/* Linear receivers: resp[r] = sum_c factors[c][r] * (trilinear interpolation of component c of the selected system's field on
 * the trimmed points of emg3d_get_receiver_response), NaN outside them; xyz / factors as there.  This is the receiver
 * operator P whose transpose the next call applies.                                                                    */
int emg3d_mg_get_receiver_response_linear(emg3d_mg_t* mg, int64_t n, const double* xyz, const double* factors, void* resp);
/* Source of the selected system (+)= P^T w: w[n] of the handle's dtype (host); the buffer is zeroed first unless
 * accumulate != 0.  Receivers whose datum is NaN (outside the trimmed points) contribute nothing.  Receivers may share
 * edges: the host builds the edge -> contributions table (O(n log n)), the device gathers per touched edge in a fixed
 * order -- results repeat bit for bit.                                                                                 */
int emg3d_mg_set_receiver_adjoint(emg3d_mg_t* mg, int64_t n, const double* xyz, const double* factors, const void* w,
                                  int accumulate);
/* The linear receivers on H = get_h_field(E) of the selected system's field (without mu_r; formed on the device in the residual
 * buffer, which is overwritten): resp[r] = sum_c factors[c][r] * (trilinear interpolation of H_c on its trimmed face points).    */
int emg3d_mg_get_receiver_response_linear_h(emg3d_mg_t* mg, double smu0_re, double smu0_im, int64_t n, const double* xyz,
                                            const double* factors, void* resp);
/* Source of the selected system (+)= P^T w for every receiver operator of this library.  method 0: the linear receivers
 * (emg3d_mg_set_receiver_adjoint is method 0, magnetic 0); method 1: the cubic-spline receivers of
 * emg3d_mg_get_receiver_response, P = R Eval F_2 F_1 F_0 Trim per component, transposed factor by factor: the 64 stencil weights
 * per receiver are gathered per touched coefficient of a zeroed trimmed array (host-built table, fixed order), the transposed
 * B-spline prefilter runs along the three axes (F^T = D F D^-1, D = diag(1/2, 1, ..., 1, 1/2): the forward filter between two
 * scalings of the line ends), the result is added to the interior of the source.  A component with fewer than four trimmed
 * points along an axis is linear, as in the forward operator; receivers with a NaN datum contribute nothing.  magnetic != 0: the
 * receivers act on H = -curl E / (s mu_0) (no mu_r): P^T w is formed on the faces (in the residual buffer, which is overwritten)
 * and every interior edge gathers its four faces (the transposed curl) times -1 / (s mu_0); smu0 is not used otherwise.  No
 * atomics: results repeat bit for bit; PEC boundary edges stay exact zeros.                                                  */
int emg3d_mg_set_receiver_adjoint_ex(emg3d_mg_t* mg, int method, int magnetic, double smu0_re, double smu0_im, int64_t n,
                                     const double* xyz, const double* factors, const void* w, int accumulate);
/* The same for all systems of a batched handle in one call: source of every system b with use[b] != 0 (+)= P^T w_b, w = [nsys][n]
 * values of dtype (row b belongs to system b; the rows of unused systems are not read as data).  The tables that depend on the grid
 * and the receivers only (edge -> contributions, coefficient -> contributions, with the fractional indices and stencil weights) are
 * built and uploaded ONCE, w is uploaded once; per system only kernels are issued (gather with that system's row, transposed
 * prefilter, trim-add, transposed curl for magnetic receivers).  Slice b of the source array is bit for bit what
 * emg3d_mg_set_receiver_adjoint_ex gives on the selected system b with row b; a used system whose row is all zero gets a zero source
 * (accumulate == 0); the sources of the other systems are not touched.                                                        */
int emg3d_mg_set_receiver_adjoint_b(emg3d_mg_t* mg, int method, int magnetic, double smu0_re, double smu0_im, int64_t n,
                                    const double* xyz, const double* factors, const void* w, const int32_t* use, int accumulate);
/* The same without a handle (mirrors emg3d_get_receiver_response): field (host, nE values of dtype, [fx|fy|fz]) = P^T w for the
 * electric (is_electric != 0) or magnetic (needs smu0) component set on the grid (hx, hy, hz, origin).                       */
int emg3d_receiver_adjoint(int dtype, int64_t nx, int64_t ny, int64_t nz, const double* hx, const double* hy, const double* hz,
                           const double* origin, int is_electric, int method, double smu0_re, double smu0_im, int64_t n,
                           const double* xyz, const double* factors, const void* w, void* field);

/* ---- regridding ---------------------------------------------------------------------------------------------------
 * maps._volume_average_weights(x1, x2), reference emg3d/maps.py:526-576, for one axis: x1 (n1 >= 2 edges, old grid) and
 * x2 (n2 >= 2 edges, new grid), ascending.  Every interval of the sorted union of the edges whose centre lies in
 * [x2[0], x2[n2-1]] is a segment: w = its length, idx_in = the x1 cell holding the centre (clipped to the first / last
 * cell), idx_out = the x2 cell holding it; *nseg segments (at most n1 + n2 - 1: the capacity of w / idx_in / idx_out),
 * sorted by idx_out.  ptr (n2 entries): new cell o owns segments [ptr[o], ptr[o+1]).  O(n) host work, no device.      */
int emg3d_volume_average_weights(const double* x1, int64_t n1, const double* x2, int64_t n2, double* w, int64_t* idx_in,
                                 int64_t* idx_out, int64_t* ptr, int64_t* nseg);
/* maps.volume_average(edges_x, edges_y, edges_z, values, new_edges_x, new_edges_y, new_edges_z, new_values, new_vol),
 * reference emg3d/maps.py:453-523, on the device: values F-ordered (nx,ny,nz) of dtype on the grid of the edges (nx+1,
 * ny+1, nz+1 of them), new_values F-ordered (mx,my,mz) of dtype: the volume-weighted sums are ADDED into it, then it is
 * divided by new_vol (F-ordered (mx,my,mz) doubles), in the reference's order of operations (bit for bit).             */
int emg3d_volume_average(int dtype, int64_t nx, int64_t ny, int64_t nz, const double* edges_x, const double* edges_y,
                         const double* edges_z, const void* values, int64_t mx, int64_t my, int64_t mz,
                         const double* new_edges_x, const double* new_edges_y, const double* new_edges_z, void* new_values,
                         const double* new_vol);
/* The segments of emg3d_volume_average_weights come out in ascending coordinate order, so they are sorted by OLD cell too:
 * iptr (n + 1 entries, n = n1 - 1 old cells): old cell i owns segments [iptr[i], iptr[i+1]) -- the offsets the transpose below
 * gathers with.  -2 if idx_in is not ascending or leaves [0, n).  O(n) host work, no device.                             */
int emg3d_volume_average_old_offsets(const int64_t* idx_in, int64_t nseg, int64_t n, int64_t* iptr);
/* The transpose of emg3d_volume_average, double only (optimize.model_gradient(method='transpose')): with A the matrix that
 * emg3d_volume_average applies to a zero new array -- A[o, i] = (sum of the segment weights (w_z w_y) w_x of new cell o that lie
 * in old cell i) / new_vol[o] --, out = A^T y: y and new_vol F-ordered (mx,my,mz) on the NEW grid, out F-ordered (nx,ny,nz) on
 * the OLD grid (overwritten).  One thread per old cell gathers t[o] = y[o] / new_vol[o] over the tensor product of its segments:
 * out[i] = sum_z sum_y sum_x ((w_z w_y) w_x) t[o], z outermost, segments ascending, from 0, nothing fused -- no atomics, results
 * repeat bit for bit.  An old cell without a segment (the old grid reaches beyond the new one) gets an exact 0.          */
int emg3d_volume_average_adjoint(int64_t nx, int64_t ny, int64_t nz, const double* edges_x, const double* edges_y,
                                 const double* edges_z, int64_t mx, int64_t my, int64_t mz, const double* new_edges_x,
                                 const double* new_edges_y, const double* new_edges_z, const double* y, const double* new_vol,
                                 double* out);
/* Sensitivities on a model grid (optimize.SurveyJacobian(model_grid=)): the model lives on a grid of (nx,ny,nz) cells with the
 * given edges and reaches the handle's grid by volume averaging (A as above: old = model grid, new = the handle's grid).
 *   set_model_grid     : the segment tables of the three axes with their new-cell and old-cell offsets, built once and kept in
 *                        HBM, plus nC doubles of scratch and 3 nM doubles for results; counted by emg3d_mg_device_bytes, freed with
 *                        the handle.  A second call takes a model grid of the same (nx,ny,nz) in place (-2 for another size).
 *   set_regrid_factors : the diagonal factors per direction, F_c on the handle's grid (nC doubles), Q_c on the model grid (nM
 *                        doubles), resident; a direction given with the pointer of direction x shares its copy.  Later calls
 *                        replace the values in place and must share in the same way (-2 otherwise).  -7 without a model grid.
 *   grad_acc_get_model : out (nM doubles, F-ordered) = Q_x (.) A^T (F_x (.) acc) of the accumulator of emg3d_mg_grad_acc_*
 *                        (isotropic models: one factor pair serves the sum of the three directions).
 *   grad_acc3_get_model: out_c = Q_c (.) A^T (F_c (.) acc_c) of the three accumulators of emg3d_mg_grad_acc3_*.
 * Both leave the accumulators as they are (the _get calls afterwards return them unchanged); only nM-sized arrays cross
 * PCIe; the arithmetic is emg3d_volume_average_adjoint's with t[o] = (F[o] acc[o]) / vol[o], vol = (hx hy) hz, and the sum times
 * Q[i].  -7 without a model grid or factors.                                                                              */
int emg3d_mg_set_model_grid(emg3d_mg_t* mg, int64_t nx, int64_t ny, int64_t nz, const double* edges_x, const double* edges_y,
                            const double* edges_z);
int emg3d_mg_set_regrid_factors(emg3d_mg_t* mg, const double* F_x, const double* F_y, const double* F_z, const double* Q_x,
                                const double* Q_y, const double* Q_z);
int emg3d_mg_grad_acc_get_model(emg3d_mg_t* mg, double* out);
int emg3d_mg_grad_acc3_get_model(emg3d_mg_t* mg, double* out_x, double* out_y, double* out_z);
/* emg3d_interp3d on the tensor product of three coordinate vectors xi_x (mx), xi_y (my), xi_z (mz): out is F-ordered
 * (mx,my,mz), out[i + mx (j + my k)] = emg3d_interp3d at (xi_x[i], xi_y[j], xi_z[k]) bit for bit; method / has_fill /
 * fill_value / cval as there (maps.grid2grid, reference emg3d/maps.py:34-178, uses 0, 1 and 3).  The per-axis work is
 * O(mx + my + mz) on the host.                                                                                        */
int emg3d_interp3d_grid(int dtype, int64_t nx, int64_t ny, int64_t nz, const double* px, const double* py, const double* pz,
                        const void* values, int64_t mx, const double* xi_x, int64_t my, const double* xi_y, int64_t mz,
                        const double* xi_z, int method, int has_fill, double fill_value, double cval, void* out);

/* ---- batched systems: several sources through the same launches ------------------------------------------
 * The reference solves one (source, frequency) system per solver.solve call; a survey has many sources per
 * frequency on ONE model (simulations.py:916-1015 loops over them, one job per source-frequency pair).  Systems
 * that share grid, model and frequency share the operator and the cached line factorisations, so a handle can carry
 * n of them through every launch of the cycle (arrays [system][nE]; kernels index the system by a grid dimension):
 * the ~1100 latency-bound coarse-level launches of a cycle do n times the work and the level-0 sweeps fetch the
 * factor once for n right-hand sides.  Each system goes through exactly the arithmetic of a solve of its own --
 * results are bit-identical to n separate handles.
 *   emg3d_mg_set_batch(mg, n)   1 <= n <= 64, before the first cycle / prepare (returns -6 afterwards); zeroes
 *                               the fields.
 *   emg3d_mg_select(mg, b)      the system that the single-field entry points address from now on: set/get
 *                               sfield/efield, set_sfield_dipole/vector, get_hfield, get_receiver_response,
 *                               get_residual, sfield_norm, gradient, *_devptr.
 *   emg3d_mg_set_mask(mg, act)  act[n]: 0 freezes a system (converged: its cycles are skipped, its field stays
 *                               untouched); the norms reported for a frozen system are 0.
 * emg3d_mg_cycle / emg3d_mg_residual_norm then write n norms, emg3d_mg_cycles ncycles x n ([cycle][system]).
 * The Krylov workspace (emg3d_mg_vec_*) addresses the selected system only; emg3d_mg_bvec_* (below) is its batched
 * counterpart.  set_batch also returns -6 once either workspace holds vectors.  Environment EMG3D_BATCH_TUNE=1 (read at
 * emg3d_mg_create): coarse-level kernel choice by lines x systems -- faster (6-11 %), results then equal stand-alone
 * solves to rounding instead of bit for bit.                                                                      */
int emg3d_mg_set_batch(emg3d_mg_t* mg, int n);
int emg3d_mg_get_batch(emg3d_mg_t* mg);
int emg3d_mg_select(emg3d_mg_t* mg, int b);
int emg3d_mg_set_mask(emg3d_mg_t* mg, const int* active);

/* solver.residual(..., norm=True), solver.py:980-1039 on the level-0 state. */
int emg3d_mg_residual_norm(emg3d_mg_t* mg, double* l2);
/* ||sfield||_2 (solver.py:305). */
int emg3d_mg_sfield_norm(emg3d_mg_t* mg, double* l2);

/* solver.smoothing on the level-0 state (solver.py:738-799). */
int emg3d_mg_smooth(emg3d_mg_t* mg, int nu, int lr_dir);

/* Another frequency on the same handle (handles made by emg3d_mg_create_sv / emg3d_mg_create_vs): eta is re-formed from the
 * sigma*V (or sigma and V) kept in HBM, the coarse models of every hierarchy built so far, the transposed model copies and every cached
 * line factorisation are recomputed by the kernels a fresh handle would run -- bit for bit a fresh handle's results --,
 * while grids, transfer weights, work buffers and captured launch graphs stay (the per-frequency jobs of
 * Simulation.compute, emg3d/simulations.py:840-867, share everything but this scalar; models.py:631-658).
 * -7: the handle was created from eta arrays; -2: complex s mu_0 for a float64 handle.                            */
int emg3d_mg_set_smu0(emg3d_mg_t* mg, double smu0_re, double smu0_im);
/* The same for handles made by emg3d_mg_create_vse (-7 for any other; emg3d_mg_set_smu0 answers -7 for these). */
int emg3d_mg_set_smu0_eps(emg3d_mg_t* mg, double smu0_re, double smu0_im, double seps0);

/* Another MODEL on the same handle (handles made by emg3d_mg_create_vs / emg3d_mg_create_vse; -7 for any other, as
 * emg3d_mg_set_smu0 answers for a handle it cannot serve): p_x, p_y, p_z hold the property of a model on the same grid in
 * map `map` (codes: emg3d_mg_create_vs); NULL or p_x for p_y / p_z means "aliases p_x", and the pattern must be the one the
 * handle was created with (-2 otherwise: the anisotropy case of a handle is fixed; -2 too for an unknown map code).  The
 * arrays are uploaded into the conductivity buffers the handle has, sigma = backward(p) is formed there, then everything
 * emg3d_mg_set_smu0 recomputes is recomputed at the frequency the handle stands at (with its s eps_0 on epsilon_r
 * handles): bit for bit a handle created from that model.  No buffer moves, so captured launch graphs, the level-0 placement,
 * workspace vectors (emg3d_mg_vec_*, emg3d_mg_bvec_*) and accumulators stay; any batch size.  The host arrays may be freed
 * when the call returns.  A failed upload leaves the handle broken (every later call: hipErrorOutOfMemory).            */
int emg3d_mg_set_model(emg3d_mg_t* mg, int map, const double* p_x, const double* p_y, const double* p_z);
/* The conductivity of component comp (0, 1, 2; an aliased component gives sigma_x) as the device holds it: nC doubles,
 * F-ordered.  Same handles as emg3d_mg_set_model (-7 otherwise).                                                       */
int emg3d_mg_get_sigma(emg3d_mg_t* mg, int comp, double* out);

/* Entry of solver.multigrid (solver.py:471-492): the reference fixes the cycmax of level 0 when the function is
 * entered, from var.clevel[var.sc_dir] of THAT moment, and keeps it for all cycles of the call although sc_dir rotates
 * (semicoarsening=True or several digits).  It matters when the first direction has clevel 0 (level 0 is its coarsest
 * grid: small odd transverse sizes) and a later one has not: the children of every later F-cycle then get
 * new_cycmax = 1.  Call once per multigrid() call, after emg3d_mg_set_params, with the current sc_dir; without it every
 * cycle derives level 0's cycmax from its own sc_dir.                                                             */
int emg3d_mg_begin(emg3d_mg_t* mg, int sc_dir);

/* ONE level-0 iteration of solver.multigrid (solver.py:518-591): pre-smooth,
 * residual, restriction, recursive coarse-grid correction (V/W/F), prolongation,
 * post-smooth, and the end-of-cycle residual norm.  sc_dir/lr_dir are the
 * current var.sc_dir / var.lr_dir.  No host<->device traffic except *l2.    */
int emg3d_mg_cycle(emg3d_mg_t* mg, int sc_dir, int lr_dir, double* l2);
/* The same cycle; while the device runs it the host does emg3d_mg_prepare(next_sc_dir, next_lr_dir) -- the pair the
 * solver's rotation (solver.py:597-600) uses in the NEXT cycle -- so that the set-up of the second and third pair of an
 * sc+lr run (5 ms each at 128^3) is hidden behind the first cycles.  next_* < 0: nothing to prepare.  Same results. */
int emg3d_mg_cycle_next(emg3d_mg_t* mg, int sc_dir, int lr_dir, int next_sc_dir, int next_lr_dir, double* l2);
/* verb = 5 of the reference (solver.py:502-578: the residual norm after every smoothing call of every level, printed as
 * "it level cycmax [nx, ny, nz]: norm  pre-smoothing" ...): with the trace on, emg3d_mg_cycle* run their launches eagerly
 * and follow every smoothing call with a norm-only residual; emg3d_mg_get_trace returns the records collected since the
 * last call -- recs[i] = {it, level, cycmax, kind (0 coarsest level, 1 pre-, 2 post-smoothing), nx, ny, nz}, it = -1 on
 * level 0 (the caller counts level-0 iterations) -- and their norms, in the order the reference would print them.
 * One system per handle.                                                                                            */
int emg3d_mg_set_trace(emg3d_mg_t* mg, int on);
int emg3d_mg_get_trace(emg3d_mg_t* mg, int max_recs, int64_t* recs, double* norms, int* count);
/* Loop-invariant set-up of the cycles with this (sc_dir, lr_dir): grid hierarchy, restriction /
 * prolongation weights, coarse models (solver.py:802-901, done once instead of per cycle), the
 * cached line factorisations and the captured launch sequence.  Optional -- the first cycle does
 * the same on demand -- and idempotent; runs no cycle and leaves the fields untouched.          */
int emg3d_mg_prepare(emg3d_mg_t* mg, int sc_dir, int lr_dir);

/* Same, `ncycles` times back to back with FIXED sc_dir/lr_dir rotation
 * sc_cycle/lr_cycle (arrays of length n_sc/n_lr, start positions given);
 * l2 receives ncycles norms.  Used by bench.py (no per-cycle host sync).    */
int emg3d_mg_cycles(emg3d_mg_t* mg, int ncycles, const int* sc_cycle, int n_sc, const int* lr_cycle,
                    int n_lr, double* l2);

/* Device pointers / stream for zero-copy interop (torch, RCCL).
 * emg3d_mg_efield_devptr: the level-0 field in the reference layout [fx|fy|fz].  Large levels keep the field in a
 * parity-split working copy between cycles; the call then enqueues the conversion on the handle's stream and returns
 * the reference-layout buffer.  The pointer is therefore a SNAPSHOT: valid (and ordered behind the handle's stream)
 * until the next cycle / smoothing / solve call on the handle; writes through it are not seen by later cycles
 * (use emg3d_mg_set_efield).  Fetch it again after every such call.  NULL on error.                               */
void* emg3d_mg_efield_devptr(emg3d_mg_t* mg);
void* emg3d_mg_sfield_devptr(emg3d_mg_t* mg);
void* emg3d_mg_stream(emg3d_mg_t* mg);
int64_t emg3d_mg_nE(emg3d_mg_t* mg);
int emg3d_mg_sync(emg3d_mg_t* mg);
/* Bytes of device memory currently held by the handle. */
int64_t emg3d_mg_device_bytes(emg3d_mg_t* mg);

/* Timing of the dominant kernel (line-smoother substitution sweep) with HIP
 * events on the handle's stream: runs `reps` sweeps (nu=1) in direction
 * dir (1,2,3) on the level-0 state; returns average ms per sweep.          */
int emg3d_mg_time_sweep(emg3d_mg_t* mg, int dir, int reps, float* ms_per_sweep);
/* Placement of level 0's working copies (levels whose working copy is >= 256 MiB, multi-colour order; EMG3D_PLACE_TRIES=<n>,
 * default 12, 0 = off): the duration of a level-0 colour launch at 256^3 depends by up to 10 % on which piece of physical
 * memory the block it WRITES got, so before the first launch sequence on working copy w (0: x-lines, 1: y-/z-lines) is
 * captured the handle times up to n candidate blocks with one sweep each, until it holds one of the fast class, and keeps the
 * fastest; when the handle goes the block is parked under its role and the next handle of the process takes it without a
 * search.  The record: *tries candidates timed (0: nothing was placed, or *kept = -1: a block of an earlier handle's search
 * was taken), *kept the index of the one that stayed (0 = the block the handle had), ms[k] = ms per sweep (4 launches) of
 * candidate k; ms must hold 16 floats.  Results do not depend on it.                                                     */
int emg3d_mg_placement(emg3d_mg_t* mg, int w, int* tries, int* kept, float* ms);
/* Name of the kernel instantiation that the handle's most recent line-sweep launch selected, e.g.
 * "k_line_sweep_th<c128,3,8>" (what `rocprofv3 --kernel-trace` shows); name must hold >= 64 bytes.      */
int emg3d_mg_last_sweep_kernel(emg3d_mg_t* mg, char* name);
/* Same for the residual kernel (amat_x).                                    */
int emg3d_mg_time_residual(emg3d_mg_t* mg, int reps, float* ms_per_call);
/* Name of the kernel instantiation of the handle's most recent residual launch, e.g. "k_residual_zm<c128,1,4>"
 * (node planes per thread and block map are chosen by level size; all give identical results); >= 64 bytes. */
int emg3d_mg_last_residual_kernel(emg3d_mg_t* mg, char* name);

/* Device-side Krylov building blocks for the BiCGSTAB path (solver.py:610-734):
 * y = A x (core.amat_x on a zero field, negated: solver.py:646-660) and
 * x = M b (one preconditioner application = `ncycles` MG cycles on a zero
 * field, solver.py:667-677) on host vectors.                                */
int emg3d_mg_amatvec(emg3d_mg_t* mg, const void* x_host, void* y_host);

/* Device-resident vector workspace for the Krylov iteration that the reference
 * delegates to scipy.sparse.linalg.bicgstab / cgs / gcrotmk (call site solver.py:717-719;
 * SciPy is pinned only as scipy>=1.4, setup.py:39): the vectors r, r~, p, v, s, t, p^, s^, x
 * (gcrotmk: the Krylov, preconditioned and recycled outer vectors) stay in HBM, only scalars
 * cross PCIe.  Vector ids: 0..n-1 = workspace vectors (nE entries of the handle's dtype,
 * zero-initialised by emg3d_mg_vec_alloc, which may be called again to grow the workspace; n <= 256),
 * -1 = the level-0 source s, -2 = the level-0 field e (so that a preconditioner
 * application is vec_copy(-1, b); set_efield(NULL); cycles; vec_copy(x, -2)).
 *   vec_axpy  : y += alpha x          vec_scale : y *= alpha
 *   vec_dot   : out2 = (Re, Im) of sum conj(a_i) b_i  (numpy.vdot; plain dot for float64),
 *               deterministic reduction; synchronises the stream
 *   vec_amatvec: dst = A src          (core.amat_x on a zero field, negated: solver.py:646-660)
 * alpha_im is ignored for float64 handles.                                   */
int emg3d_mg_vec_alloc(emg3d_mg_t* mg, int n);
int emg3d_mg_vec_set(emg3d_mg_t* mg, int id, const void* host);
int emg3d_mg_vec_get(emg3d_mg_t* mg, int id, void* host);
int emg3d_mg_vec_copy(emg3d_mg_t* mg, int dst, int src);
int emg3d_mg_vec_axpy(emg3d_mg_t* mg, int y, double alpha_re, double alpha_im, int x);
int emg3d_mg_vec_scale(emg3d_mg_t* mg, int y, double alpha_re, double alpha_im);
int emg3d_mg_vec_dot(emg3d_mg_t* mg, int a, int b, double* out2);
int emg3d_mg_vec_amatvec(emg3d_mg_t* mg, int dst, int src);

/* The same workspace for ALL systems of a batched handle at once (solver.solve_sources with a Krylov solver): "batched
 * vectors" [nsys][nE] addressed by index 0..n-1 (zero-initialised; n <= 256), -1 = the whole level-0 source array,
 * -2 = the whole level-0 field array (brought to the reference layout first).  Every primitive acts on the systems that
 * are not frozen (emg3d_mg_set_mask) and leaves the others' data untouched; per system the result is bit for bit that
 * of the emg3d_mg_vec_* primitive on that system's vectors (same launch geometry per system, same summation order).
 * The emg3d_mg_vec_* workspace keeps its meaning on batched handles (nE-sized vectors, -1 / -2 = the selected system).
 *   bvec_alloc  : optional memory -- on failure hipErrorOutOfMemory is returned and the handle stays usable
 *   bvec_copy   : dst_b = src_b       bvec_zero : dst_b = 0
 *   bvec_axpy   : y_b += alpha_b x_b  bvec_scale: y_b *= alpha_b     alpha: [nsys][2] doubles (Re, Im; Im ignored for
 *                 float64 handles), passed to the kernel by value: no upload, no synchronisation
 *   bvec_dot    : out[2 b], out[2 b + 1] = (Re, Im) of sum conj(a_b,i) b_b,i; ONE device-to-host copy for all systems;
 *                 the entries of frozen systems are not written; synchronises the stream
 *   bvec_amatvec: dst_b = A src_b
 *   bvec_get / bvec_set: system b's slice of a batched vector <-> host (nE entries), frozen or not             */
int emg3d_mg_bvec_alloc(emg3d_mg_t* mg, int n);
int emg3d_mg_bvec_copy(emg3d_mg_t* mg, int dst, int src);
int emg3d_mg_bvec_zero(emg3d_mg_t* mg, int id);
int emg3d_mg_bvec_axpy(emg3d_mg_t* mg, int y, const double* alpha, int x);
int emg3d_mg_bvec_scale(emg3d_mg_t* mg, int y, const double* alpha);
int emg3d_mg_bvec_dot(emg3d_mg_t* mg, int a, int b, double* out);
int emg3d_mg_bvec_amatvec(emg3d_mg_t* mg, int dst, int src);
int emg3d_mg_bvec_get(emg3d_mg_t* mg, int id, int b, void* host);
int emg3d_mg_bvec_set(emg3d_mg_t* mg, int id, int b, const void* host);

#ifdef __cplusplus
}
#endif
#endif /* EMG3D_HIP_H */
