"""Inputs and references of the accuracy tests (tests/test_oracle_truth.py on the CPU, tests/test_gpu_accuracy.py on the GPU) and of
the family-level tests of the batched contract (tests/test_gpu_batch_families.py: every sweep kernel family, the point smoother and
the residual kernels with three systems in one handle, one of them frozen, and with 64).

Two generators, each a function of (shape, direction, dtype, seed) that returns float64 / complex128 arrays:

* `benign`: what the kernel-level parity tests draw (tests/test_gpu_kernels.py::_sweeps_against_oracle): widths U(0.5, 2),
  eta = 0.3j U(0.5, 2) (float64: -U(0.5, 2)), zeta U(0.5, 2), random field and source (here with the boundary's tangential
  components zero, as the fields of a solve have them).  Line systems of condition ~10: the float64
  reference is 10 to 20 ulp from the truth.
* `hard`: what real models do to a line -- widths stretched by 1.2 ... 1.3 per cell about the centre (axes of fewer than 8 cells:
  random widths), conductivity per cell from {1e-8 (air), 1e-2 (resistive body), 3 (sea water)} S/m with anisotropy factors
  (1, 2, 0.5), eta = -i omega mu_0 sigma V at 0.1 Hz (float64: -s mu_0 sigma V, s = 0.6), zeta = V / U(0.9, 1.3), random field and a
  random source at 1e-6 of it.  The float64 reference is 1e-13 ... 1e-9 from the truth (asserted per case in test_oracle_truth.py).

The truth is the oracle's smoother (oracle/emg3d_oracle.cpp) compiled with every scalar a long double (x87 extended precision, 64-bit
significand) on the same float64 inputs, converted exactly; `reference` is the float64 oracle.  Both are computed once per case and
shared read-only.

Batched runs: system 0 of a case is the case's own `e0`, `s`; `system_fields` draws the start field and source of system b >= 1 on the
same grid and model from a generator of its own (the draws above are not touched), `references_b` holds their oracle sweep and truth.
`wide_runs` gives every case its line length on 36 x 36 lines (324 per colour), so that a batched launch has more line blocks than
XCDs and the line map of `EMG_SWEEP_WG` (csrc/common.hpp) places blocks inside an XCD's share."""
import numpy as np

MU_0 = 4e-7 * np.pi
SIGMAS = (1e-8, 1e-2, 3.0)          # S/m: air, resistive body, sea water
ANISOTROPY = (1.0, 2.0, 0.5)        # sigma_x, sigma_y, sigma_z as multiples of the drawn sigma
FREQ = 0.1                          # Hz (complex128)
S_LAPLACE = 0.6                     # 1/s (float64)
BASE_WIDTH = 50.0                   # m: the smallest cell of a stretched axis


def n_edges(shape):
    nx, ny, nz = shape
    return nx * (ny + 1) * (nz + 1) + (nx + 1) * ny * (nz + 1) + (nx + 1) * (ny + 1) * nz


def _rng(shape, direction, dtype, seed, salt):
    return np.random.default_rng([salt, *shape, direction, np.dtype(dtype).itemsize, seed])


def field_views(f, shape):
    """(fx, fy, fz) F-ordered views of a flat field buffer."""
    nx, ny, nz = shape
    n1, n2 = nx * (ny + 1) * (nz + 1), (nx + 1) * ny * (nz + 1)
    return (f[:n1].reshape((nx, ny + 1, nz + 1), order='F'), f[n1:n1 + n2].reshape((nx + 1, ny, nz + 1), order='F'),
            f[n1 + n2:].reshape((nx + 1, ny + 1, nz), order='F'))


def _fields(rng, shape, cplx, source_scale):
    """Random start field and source, tangential components zero on the boundary (the smoothers take them as that: a line's system
    has no term for them, so `s - A e` vanishes on a solved line only then)."""
    nE = n_edges(shape)

    def rnd():
        a = rng.standard_normal(nE)
        a = a + 1j * rng.standard_normal(nE) if cplx else a
        fx, fy, fz = field_views(a, shape)
        fx[:, [0, -1], :] = 0; fx[:, :, [0, -1]] = 0
        fy[[0, -1], :, :] = 0; fy[:, :, [0, -1]] = 0
        fz[[0, -1], :, :] = 0; fz[:, [0, -1], :] = 0
        return a
    return rnd(), source_scale * rnd()


def benign(shape, direction, dtype, seed=0):
    rng = _rng(shape, direction, dtype, seed, 1)
    cplx = np.dtype(dtype) == np.complex128
    h = [rng.uniform(0.5, 2, n) for n in shape]
    eta = [np.asfortranarray(rng.uniform(0.5, 2, shape) * (0.3j if cplx else -1.0)) for _ in range(3)]
    zeta = np.asfortranarray(rng.uniform(0.5, 2, shape))
    e0, s = _fields(rng, shape, cplx, 1.0)
    return dict(h=h, eta=eta, zeta=zeta, e0=e0, s=s)


def hard(shape, direction, dtype, seed=0):
    rng = _rng(shape, direction, dtype, seed, 2)
    cplx = np.dtype(dtype) == np.complex128
    h = []
    for n in shape:
        if n < 8:
            h.append(BASE_WIDTH * rng.uniform(1., 4., n))
        else:
            h.append(BASE_WIDTH * rng.uniform(1.2, 1.3) ** np.abs(np.arange(n) - (n - 1) / 2))
    vol = np.einsum('i,j,k->ijk', *h)
    sigma = rng.choice(SIGMAS, size=shape)
    smu0 = (2j * np.pi * FREQ if cplx else S_LAPLACE) * MU_0
    eta = [np.asfortranarray(-smu0 * (f * sigma) * vol) for f in ANISOTROPY]
    zeta = np.asfortranarray(vol / rng.uniform(0.9, 1.3, shape))
    e0, s = _fields(rng, shape, cplx, 1e-6)
    return dict(h=h, eta=eta, zeta=zeta, e0=e0, s=s)


GENERATORS = {"benign": benign, "hard": hard}
GENERATOR_IDS = {"benign": 1, "hard": 2}
# Seeds of the hard cases the tests use: 0, but for the draws below, where seed 0 puts one pathological line into the case (a line
# through air cells only is close to singular: the float64 reference itself is then 1e-7 off, and the max-norm speaks of that line
# alone).  The smallest seed whose float64 reference is 2e-13 ... 5e-10 from the truth; test_oracle_truth.py holds every case to
# [1e-13, 1e-9].
HARD_SEEDS = {((4, 130, 6), 2, 'D'): 1, ((5, 6, 33), 3, 'D'): 1, ((5, 40, 6), 2, 'D'): 3, ((6, 5, 130), 3, 'D'): 1,
              ((6, 5, 250), 3, 'D'): 1, ((6, 5, 250), 3, 'd'): 1, ((6, 50, 8), 2, 'd'): 1, ((12, 10, 4), 3, 'd'): 1,
              ((16, 6, 5), 2, 'D'): 1, ((130, 4, 6), 1, 'd'): 2}
_cache = {}


def seed_of(kind, shape, direction, dtype):
    return HARD_SEEDS.get((tuple(shape), direction, np.dtype(dtype).char), 0) if kind == "hard" else 0


def _frozen(a):
    a.setflags(write=False)
    return a


def problem(kind, shape, direction, dtype, seed=None):
    """The inputs of a case, drawn once (seed None: the one the tests use, `seed_of`)."""
    seed = seed_of(kind, shape, direction, dtype) if seed is None else seed
    key = ("problem", kind, tuple(shape), direction, np.dtype(dtype).char, seed)
    if key not in _cache:
        p = GENERATORS[kind](tuple(shape), direction, dtype, seed)
        for a in (*p['h'], *p['eta'], p['zeta'], p['e0'], p['s']):
            a.setflags(write=False)
        _cache[key] = p
    return _cache[key]


def extended(a):
    """A float64 / complex128 array in np.longdouble / np.clongdouble (exact)."""
    a = np.asarray(a)
    return a.astype(np.clongdouble if np.iscomplexobj(a) else np.longdouble)


def sweep(oracle, p, direction, nu=2, order=1, ext=False):
    """`nu` sweeps of the oracle's smoother along `direction` (0: points) from p['e0'], in float64 or in extended precision."""
    up = extended if ext else np.array
    e = up(p['e0'])
    oracle.gauss_seidel(p['zeta'].shape, e, up(p['s']), *(up(a) for a in p['eta']), up(p['zeta']), *(up(a) for a in p['h']), nu,
                        direction=direction, order=order)
    return e


def amat_x(oracle, p, e, ext=False):
    """s - A e with the oracle's amat_x, in float64 or in extended precision (e in either)."""
    up = extended if ext else np.array
    r = up(p['s'])
    oracle.amat_x(p['zeta'].shape, r, up(e), *(up(a) for a in p['eta']), up(p['zeta']), *(up(a) for a in p['h']))
    return r


def references(oracle, kind, shape, direction, dtype, seed=None, order=1, nu=2):
    """(problem, float64 reference, extended truth) of `nu` sweeps: computed once per case."""
    seed = seed_of(kind, shape, direction, dtype) if seed is None else seed
    key = ("sweep", kind, tuple(shape), direction, np.dtype(dtype).char, seed, order, nu)
    if key not in _cache:
        p = problem(kind, shape, direction, dtype, seed)
        _cache[key] = (p, _frozen(sweep(oracle, p, direction, nu, order)), _frozen(sweep(oracle, p, direction, nu, order, ext=True)))
    return _cache[key]


def err(x, truth):
    """max|x - truth| / max|truth|, evaluated in np.longdouble."""
    truth = np.asarray(truth)
    d = np.abs(np.asarray(x).astype(truth.dtype) - truth).max()
    return float(d / np.abs(truth).max())


# ---- further systems of a case (batched handles) ------------------------------------------------------------------------------------
SYSTEM_SALT = 3                     # (`_rng` uses 1 for the benign and 2 for the hard generator)
SOURCE_SCALE = {"benign": 1.0, "hard": 1e-6}
# (systems 1 and 2 of every hard run: float64 reference 3.6e-13 ... 5.2e-11 from the truth, the sweep changes the field by >= 0.9;
# tests/test_oracle_truth.py holds them to the window of system 0, [1e-13, 1e-9])


def system_fields(kind, shape, direction, dtype, b):
    """(e0_b, s_b) of system `b` of a batched run on the case `problem(kind, shape, direction, dtype)`: system 0 is the case's own
    pair; b >= 1 is drawn with `_fields` (same boundary treatment, same source scale) from a generator salted by SYSTEM_SALT and b."""
    if b == 0:
        p = problem(kind, shape, direction, dtype)
        return p['e0'], p['s']
    char = np.dtype(dtype).char
    key = ("fields", kind, tuple(shape), direction, char, b)
    if key not in _cache:
        rng = np.random.default_rng([SYSTEM_SALT, b, GENERATOR_IDS[kind], *shape, direction, np.dtype(dtype).itemsize,
                                     seed_of(kind, shape, direction, dtype), 0])
        e0, s = _fields(rng, tuple(shape), np.dtype(dtype) == np.complex128, SOURCE_SCALE[kind])
        _cache[key] = (_frozen(e0), _frozen(s))
    return _cache[key]


def system_problem(kind, shape, direction, dtype, b):
    """The case's problem with the fields of system `b` (grid and model shared, not copied)."""
    e0, s = system_fields(kind, shape, direction, dtype, b)
    return dict(problem(kind, shape, direction, dtype), e0=e0, s=s)


def references_b(oracle, kind, shape, direction, dtype, b, order, nu=2):
    """(float64 reference, extended truth) of `nu` sweeps of system `b`: computed once per case and system."""
    if b == 0:
        return references(oracle, kind, shape, direction, dtype, order=order, nu=nu)[1:]
    key = ("sweep_b", kind, tuple(shape), direction, np.dtype(dtype).char, b, order, nu)
    if key not in _cache:
        p = system_problem(kind, shape, direction, dtype, b)
        _cache[key] = (_frozen(sweep(oracle, p, direction, nu, order)), _frozen(sweep(oracle, p, direction, nu, order, ext=True)))
    return _cache[key]


def reference_b(oracle, kind, shape, direction, dtype, b, order, nu=2):
    """The float64 reference of system `b` alone (no truth: what the 64-system runs compare with)."""
    key = ("sweep_b", kind, tuple(shape), direction, np.dtype(dtype).char, b, order, nu)
    if key in _cache or b == 0:
        return references_b(oracle, kind, shape, direction, dtype, b, order, nu)[0]
    key = ("sweep_b64", *key[1:])
    if key not in _cache:
        _cache[key] = _frozen(sweep(oracle, system_problem(kind, shape, direction, dtype, b), direction, nu, order))
    return _cache[key]


def first_difference(a, b, shape):
    """(component, i, j, k) of the first edge, in storage order, at which two fields differ; None where they are equal."""
    d = np.flatnonzero(np.asarray(a) != np.asarray(b))
    if d.size == 0:
        return None
    nx, ny, nz = shape
    dims = ((nx, ny + 1, nz + 1), (nx + 1, ny, nz + 1), (nx + 1, ny + 1, nz))
    k = int(d[0])
    for c, dim in enumerate(dims):
        n = dim[0] * dim[1] * dim[2]
        if k < n:
            return (c, *(int(v) for v in np.unravel_index(k, dim, order='F')))
        k -= n


FLOOR = 16 * 2.0 ** -53          # a few final roundings where the reference itself is at 10 to 20 ulp
FACTOR = 10.0                    # sound elimination orders sit at 1 x the reference's error, the two rejected ones at 150 x and 5000 x


def bound(err_ref):
    """What a float64 kernel may be off the truth: FACTOR x the float64 reference's own error on the same case."""
    return FACTOR * max(err_ref, FLOOR)


# ---- the cases of tests/test_gpu_accuracy.py ---------------------------------------------------------------------------------------
# One entry per kernel family and setting: the library that has it ('product': what ships, no variable set; 'lab': one environment
# variable per knob, read when a handle is created), the ordering, the (shape, direction) runs -- the smallest shapes that select the
# instantiation along x-, y- and z-lines -- and the kernel name `emg3d_sweep_plan` must answer, '{t}' standing for c128 / f64
# (tests/test_oracle_truth.py asks the planner on the CPU, the GPU test asks the handle).  `fused`: whether the launch log must show
# the colour passes of the call fused into one launch (None: not looked at).
_QOFF = {"EMG3D_QPL": "0"}
_THM = dict(_QOFF, EMG3D_THA="0")
_THM_RUNS = [((5, 7, 16), 3), ((16, 5, 6), 1), ((6, 33, 5), 2)]
_THA_RUNS = [((40, 6, 6), 1), ((6, 50, 8), 2), ((8, 6, 64), 3)]
_QC_RUNS = [((16, 6, 5), 1), ((6, 16, 5), 2), ((5, 6, 33), 3)]
_ONE = [((16, 6, 5), 1), ((16, 6, 5), 2), ((16, 6, 5), 3)]
_CHAIN_RUNS = [((4, 12, 10), 1), ((10, 4, 12), 2), ((12, 10, 4), 3)]


def _case(name, kernel, runs, library="lab", env=None, ordering="colour", fused=None):
    return dict(name=name, kernel=kernel, runs=runs, library=library, env=dict(env or {}), ordering=ordering, fused=fused)


def _thm_cases():
    out = []
    for tag, kernel, env in (("thm38", "k_line_sweep_thm<{t},3,8>", {}), ("thm28", "k_line_sweep_thm<{t},2,8>", {"EMG3D_TW_STAGES": "2"}),
                             ("thm34", "k_line_sweep_thm<{t},3,4>", {"EMG3D_TH_LPW": "4"}),
                             ("thm312", "k_line_sweep_thm<{t},3,12>", {"EMG3D_TH_LPW": "12"})):
        out.append(_case(tag + "_zkeep", kernel, _THM_RUNS, env=dict(_THM, **env)))
        out.append(_case(tag + "_parked", kernel, _THM_RUNS, env=dict(_THM, EMG3D_THM_ZKEEP="0", **env)))
    return out


SWEEP_CASES = [
    # the scan kernel's chain form: lines of <= 4 blocks; per-pass launches, and what ships (the passes of a call fused)
    _case("chain", "k_line_sweep_qpl_chain<{t},1,1>", _CHAIN_RUNS, env={"EMG3D_QPL_FUSE": "0"}, fused=False),
    _case("chain_fused_product", "k_line_sweep_qpl_chain<{t},1,1>", _CHAIN_RUNS, library="product", fused=True),
    # fused colour passes, chain form (4-block lines) and scan form (8-block lines; lab build only)
    _case("fused", "k_line_sweep_qpl_chain<{t},1,1>", [((40, 4, 4), 2), ((40, 4, 4), 3), ((4, 40, 8), 1)], env={"EMG3D_QPL_FUSE": "8"},
          fused=True),
    _case("fused_scan", "k_line_sweep_qpl<{t},1,1>", [((8, 4, 40), 1), ((40, 8, 4), 2), ((4, 40, 8), 3)], env={"EMG3D_QPL_FUSE": "8"}, fused=True),
    # the scan kernel: one block per quad; two blocks per quad (lines of >= 32 blocks) in one wave and in two; eight waves per line
    _case("qpl11", "k_line_sweep_qpl<{t},1,1>", [((12, 6, 5), 1), ((5, 16, 6), 2), ((6, 5, 12), 3)], library="product"),
    _case("qpl12", "k_line_sweep_qpl<{t},1,2>", [((32, 6, 5), 1), ((5, 32, 6), 2), ((6, 5, 32), 3)], library="product"),
    _case("qpl22", "k_line_sweep_qpl<{t},2,2>", [((40, 6, 5), 1), ((5, 40, 6), 2), ((6, 5, 64), 3)], library="product"),
    _case("qpl82", "k_line_sweep_qpl<{t},8,2>", [((130, 4, 6), 1), ((4, 130, 6), 2), ((6, 5, 250), 3)], env={"EMG3D_QPL_MAX_NL": "256"}),
    _case("qpl_lex", "k_line_sweep_qpl<{t},", [((20, 6, 5), 1), ((6, 20, 5), 2), ((6, 5, 130), 3)], library="product", ordering="lex"),
    *_thm_cases(),
    _case("tha3", "k_line_sweep_tha<{t},3>", _THA_RUNS, env={"EMG3D_THA_MIN_LINES": "1"}),
    _case("tha2", "k_line_sweep_tha<{t},2>", _THA_RUNS, env={"EMG3D_THA_MIN_LINES": "1", "EMG3D_THA": "2"}),
    _case("qc34", "k_line_sweep_qc<{t},3,4>", _QC_RUNS, env=dict(_QOFF, EMG3D_Q="2")),
    _case("qc216", "k_line_sweep_qc<{t},2,16>", _QC_RUNS, env=dict(_QOFF, EMG3D_Q="2", EMG3D_Q_LPW="16", EMG3D_Q_STAGES="2")),
    # (the 64-bit offsets need a level with lines for the quad kernel in every direction: EMG3D_Q_MIN_LINES=1 says these few are)
    _case("qc_big", "k_line_sweep_qc_big<{t},", _QC_RUNS, env=dict(_QOFF, EMG3D_Q="2", EMG3D_Q_BIG="1", EMG3D_Q_MIN_LINES="1")),
    _case("rp4", "k_line_sweep_rp<{t},4>", _ONE, env=dict(_QOFF, EMG3D_TWIST="0", EMG3D_LPW="4")),
    _case("rp8", "k_line_sweep_rp<{t},8>", _ONE, env=dict(_QOFF, EMG3D_TWIST="0", EMG3D_LPW="8")),
    _case("tpl", "k_line_sweep<{t}>", _ONE, env={"EMG3D_SWEEP": "tpl"}),
]
# the point smoother (one kernel, no planner): direction 0, both orderings
POINT_CASES = [((8, 6, 5), "colour"), ((9, 11, 13), "colour"), ((8, 6, 5), "lex"), ((9, 11, 13), "lex")]
# k_residual and k_residual_zm on the hard model
RESIDUAL_SHAPES = [(20, 12, 9), (33, 17, 21)]
RESIDUAL_CASES = [("k_residual<{t},1>", {}), ("k_residual_zm<{t},1,4>", {"EMG3D_RES_ZM_MIN_CELLS": "0", "EMG3D_RES_KZ": "4"})]
DTYPES = (np.complex128, np.float64)


def tname(dtype):
    return "c128" if np.dtype(dtype) == np.complex128 else "f64"


def sweep_runs():
    """Every distinct (shape, direction, order) the GPU sweep tests run, points included."""
    runs = {(shape, d, 1 if c["ordering"] == "colour" else 0) for c in SWEEP_CASES for shape, d in c["runs"]}
    runs |= {(shape, 0, 1 if o == "colour" else 0) for shape, o in POINT_CASES}
    return sorted(runs)


# ---- wide runs: the same lines, many of them -----------------------------------------------------------------------------------------
WIDE = 36                  # transverse cells of a wide run: 18 x 18 = 324 lines per colour -- 11 ... 324 line blocks per system in every
#                            family's launch (the thread-per-line kernel: 6), more than the 8 XCDs, several counts no multiple of 8
WIDE_FUSED_SCAN = 20       # `fused_scan` stops fusing above this; 100 lines per colour
# (at 68 transverse cells the fused cases no longer fuse and qpl22 moves to k_line_sweep_tha: no wider than this)


def wide_of(case):
    return WIDE_FUSED_SCAN if case["name"] == "fused_scan" else WIDE


def wide_runs(case):
    """One run per (shape, direction) of a case: the line length and direction kept, both transverse axes `wide_of(case)` cells.
    Benign generator only: on the wide hard model the float64 oracle itself is 1e-8 ... 2e-5 from the truth (lines through the
    strongly stretched corner cells), and a bound relative to that says nothing."""
    w = wide_of(case)
    return [(tuple(n if a == d - 1 else w for a, n in enumerate(shape)), d) for shape, d in case["runs"]]
