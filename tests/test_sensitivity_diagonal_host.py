"""CPU: maps.sensitivity_diagonal, the host restatement of the survey sensitivity diagonal diag(J^H W J) -- no GPU needed.

* the transpose identity of one row: sum_j v_j (c_x + c_y + c_z)_j == sum_edges C(v) s mu_0 lambda E, with C(v) a numpy
  restatement of the transposed statements of edges2cellaverages (the device's maps.cellaverages2edges takes its place in
  tests/test_gpu_sensitivity_diagonal.py, where a GPU is at hand);
* the ROUNDING YARDSTICK of the kernel tests: the restatement in float64 against itself in np.longdouble on the inputs of
  tests/test_gpu_sensitivity_diagonal.py (``kernel_case`` below, shared with that module).  ``F64_VS_LONGDOUBLE`` records the
  largest max-norm deviation relative to the max of the result; the kernel-level tolerance is 4 x that (FMA contraction and
  another association of the twelve-term sums), the end-to-end tolerance twice the kernel-level one."""
import numpy as np
import pytest

SHAPES = [(5, 6, 7), (2, 3, 4), (9, 4, 2)]
NSYS = [1, 3, 64]
# Largest float64-versus-longdouble deviation of maps.sensitivity_diagonal over all kernel cases (3 grids x 2 types x 3 widths x
# both forms), measured by test_rounding_yardstick below (x86-64, 80-bit long double: 8.107e-16, the split form of (9, 4, 2) c128
# with one system) and rounded up to two digits.
F64_VS_LONGDOUBLE = 8.2e-16
TOL_KERNEL = 4 * F64_VS_LONGDOUBLE
TOL_SURVEY = 2 * TOL_KERNEL


def kernel_case(shape, real, nsys):
    """The inputs of one kernel-level case: a stretched grid of ``shape`` cells, ``nsys`` random forward and adjoint fields (the
    systems that are masked out, and those whose weights are all zero, hold NaN: whatever reads them shows), the two masks with
    holes (nsys = 64: bit 63 set in both), a weight table with zeros among the active pairs, s mu_0 of 1 Hz resp. s = 2."""
    import emg3d_amd as em
    rng = np.random.default_rng(1000 * nsys + 10 * sum(shape) + int(real))
    h = [40.0 * 1.25 ** np.abs(np.arange(n) - 0.4 * n) * rng.uniform(0.9, 1.1, n) for n in shape]
    grid = em.TensorMesh(h, origin=(-100., 50., -300.))
    nE = int(grid.nE)

    def rnd():
        a = rng.standard_normal((nsys, nE))
        return a if real else a + 1j * rng.standard_normal((nsys, nE))
    fwd, adj = rnd(), rnd()
    use_fwd, use_adj = np.zeros(nsys, dtype=np.int32), np.zeros(nsys, dtype=np.int32)
    W = rng.uniform(0.5, 2.0, (nsys, nsys))
    if nsys == 1:
        use_fwd[:] = use_adj[:] = 1
    elif nsys == 3:
        use_fwd[[0, 2]] = 1
        use_adj[[0, 1]] = 1
        W[1, 0] = 0.0                   # a skipped pair of two active systems
    else:
        use_fwd[[0, 2, 9, 17, 40, 63]] = 1
        use_adj[[0, 5, 7, 31, 63]] = 1
        W[5, 17] = W[63, 0] = W[0, 63] = 0.0
        W[7, :] = 0.0                   # an active adjoint system without a datum ...
        W[:, 9] = 0.0                   # ... and an active forward system without one: their fields are never read
        adj[7] = np.nan
        fwd[9] = np.nan
    fwd[use_fwd == 0] = np.nan
    adj[use_adj == 0] = np.nan
    smu0 = em.fields.FrequencySpec(-2.0 if real else 1.0).smu0
    return dict(grid=grid, fwd=fwd, adj=adj, use_fwd=use_fwd, use_adj=use_adj, W=W, smu0=smu0,
                W_eff=W * use_adj[:, None] * use_fwd[None, :])


def _deviation(got, want):
    want = np.asarray(want)
    return float(np.abs(np.asarray(got, dtype=want.dtype) - want).max() / np.abs(want).max())


def _edge_shapes(vnC):
    nx, ny, nz = vnC
    return (nx, ny + 1, nz + 1), (nx + 1, ny, nz + 1), (nx + 1, ny + 1, nz)


def cells2edges_numpy(v3, vol):
    """Every statement of edges2cellaverages, transposed: a boundary edge sees its cell two or four times."""
    nx, ny, nz = vol.shape
    want = [np.zeros(s, dtype=v3[0].dtype) for s in _edge_shapes(vol.shape)]

    def lo(n):          # cell max(e - 1, 0) of edge e = 0 .. n
        return np.maximum(np.arange(n + 1) - 1, 0)

    def hi(n):          # cell min(e, n - 1)
        return np.minimum(np.arange(n + 1), n - 1)
    for a in (lo, hi):
        for b in (lo, hi):
            want[0] += (vol * v3[0] / 4)[:, a(ny), :][:, :, b(nz)]
            want[1] += (vol * v3[1] / 4)[a(nx), :, :][:, :, b(nz)]
            want[2] += (vol * v3[2] / 4)[a(nx), :, :][:, b(ny), :]
    return want


def row_identity_gap(case, v, cells2edges):
    """For every pair of an adjoint and a forward field of ``case``: |sum_j v_j (c_x + c_y + c_z)_j - sum_edges C(v) s mu_0 lambda
    E| relative to the sum of the absolute terms of the right-hand side; the largest over the pairs."""
    from emg3d_amd import maps
    grid = case['grid']
    vnC = tuple(int(n) for n in grid.vnC)
    shapes = _edge_shapes(vnC)
    off = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
    vol = np.asarray(grid.cell_volumes).reshape(vnC, order='F')
    cv = np.concatenate([a.ravel(order='F') for a in cells2edges((v, v, v), vol)])
    worst = 0.0
    for ba in np.flatnonzero(case['use_adj']):
        for bf in np.flatnonzero(case['use_fwd']):
            if case['W_eff'][ba, bf] == 0:
                continue
            prod = (case['adj'][ba] * case['fwd'][bf]) * case['smu0']
            cc = maps._edges2cellaverages_host([prod[off[c]:off[c + 1]].reshape(shapes[c], order='F') for c in range(3)], vol)
            lhs = np.sum(v * ((cc[0] + cc[1]) + cc[2]))
            rhs = np.sum(cv * prod)
            worst = max(worst, abs(lhs - rhs) / np.sum(np.abs(cv * prod)))
    return worst


@pytest.mark.parametrize("real", [False, True], ids=["c128", "f64"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
def test_row_is_the_transpose_of_the_jvec_source(shape, real):
    """Both sides are sums of ~4 nE products in float64: 1e-13 of the sum of their absolute values."""
    case = kernel_case(shape, real, 3)
    v = np.random.default_rng(3).standard_normal(shape)
    gap = row_identity_gap(case, v, cells2edges_numpy)
    print(f"transpose identity {shape} {'f64' if real else 'c128'}: {gap:.2e}")
    assert gap < 1e-13


def test_restatement_equals_the_statement_loop():
    """_edges2cellaverages_host against the reference's loop (oracle/gradient.py), statement by statement: to the rounding of a
    sixteen-term sum, boundary multiplicities included."""
    from oracle import gradient as og
    from emg3d_amd import maps
    rng = np.random.default_rng(4)
    for shape in SHAPES:
        vol = rng.uniform(1, 2, shape)
        comps = [rng.standard_normal(s) + 1j * rng.standard_normal(s) for s in _edge_shapes(shape)]
        for got, want in zip(maps._edges2cellaverages_host(comps, vol), og.edges2cellaverages(*comps, vol)):
            assert _deviation(got, want) < 1e-15


def yardsticks():
    """Per kernel case and form: (shape, real, nsys, split, float64 result, longdouble result)."""
    from emg3d_amd import maps
    for shape in SHAPES:
        for real in (False, True):
            for nsys in NSYS:
                case = kernel_case(shape, real, nsys)
                for split in (False, True):
                    args = (case['grid'], case['fwd'], case['adj'], case['smu0'], case['W_eff'])
                    yield (shape, real, nsys, split, maps.sensitivity_diagonal(*args, components=split),
                           maps.sensitivity_diagonal(*args, components=split, dtype=np.longdouble))


def test_rounding_yardstick():
    """The recorded deviation bounds every case, and is no looser than twice what is measured (where long double is wider)."""
    worst = 0.0
    for shape, real, nsys, split, f64, ld in yardsticks():
        f64, ld = (f64, ld) if split else ((f64,), (ld,))
        assert all(a.dtype == np.float64 and b.dtype == np.longdouble and a.shape == shape for a, b in zip(f64, ld))
        assert all(np.isfinite(b).all() and b.min() >= 0 and b.max() > 0 for b in ld)
        dev = max(_deviation(a, b) for a, b in zip(f64, ld))
        print(f"{shape} {'f64' if real else 'c128'} nsys {nsys} split {split}: float64 vs longdouble {dev:.2e}")
        worst = max(worst, dev)
    print(f"largest deviation {worst:.3e} (recorded: {F64_VS_LONGDOUBLE:.1e})")
    assert worst <= F64_VS_LONGDOUBLE
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        assert worst >= F64_VS_LONGDOUBLE / 2


def test_kernel_uses_no_scratch(tmp_path):
    """The compiler's resource remarks for the four instantiations of k_sens_acc on gfx950: no scratch (the edge values of a cell
    are indexed with compile-time constants only), and the VGPR counts DESIGN 8.8 states (needs hipcc, not a GPU).  Likewise for the
    other per-cell kernels that share its cell frame, k_gradient and k_gradient_acc: no scratch, and no more VGPRs than each
    instantiation took when the frame was written out in every kernel."""
    import os
    import shutil
    import subprocess
    import __graft_entry__ as g
    from conftest import ROOT
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = subprocess.run([hipcc] + g.FLAGS + ["-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "emg3d_hip.o"),
                          os.path.join(ROOT, "emg3d_amd", "csrc", "emg3d_hip.hip")], capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    name, seen = None, {}
    for line in out.stderr.splitlines():
        if "Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
        elif name and ("k_sens_acc" in name or "k_gradient" in name):
            for key in ("ScratchSize [bytes/lane]:", " VGPRs:"):
                if key in line:
                    seen.setdefault(name, {})[key.strip()] = int(line.split(key)[1].split()[0])
    print(seen)
    sens = {k: v for k, v in seen.items() if "k_sens_acc" in k}
    assert len(sens) == 4, seen
    assert all(v["ScratchSize [bytes/lane]:"] == 0 for v in seen.values()), seen
    assert all(v["VGPRs:"] <= (164 if "c128" in k else 88) for k, v in sens.items()), seen
    # (kernel, scalar type, SPLIT) -> VGPRs; the mangled name carries k_gradient as 10k_gradientI, k_gradient_acc as 14k_gradient_accI
    bounds = {("10k_gradientI", "4c128", 0): 60, ("10k_gradientI", "4c128", 1): 62, ("10k_gradientI", "d", 0): 40,
              ("10k_gradientI", "d", 1): 40, ("14k_gradient_accI", "4c128", 0): 98, ("14k_gradient_accI", "4c128", 1): 116,
              ("14k_gradient_accI", "d", 0): 72, ("14k_gradient_accI", "d", 1): 76}
    for (kern, scalar, split), vgprs in bounds.items():
        hit = [v for k, v in seen.items() if k.startswith(f"_Z{kern}{scalar}Lb{split}E")]
        assert len(hit) == 1, (kern, scalar, split, seen)
        assert hit[0]["VGPRs:"] <= vgprs, (kern, scalar, split, hit[0])
    assert len(seen) == 12, seen


def test_weights_and_shapes():
    from emg3d_amd import maps
    case = kernel_case((2, 3, 4), False, 3)
    args = (case['grid'], case['fwd'], case['adj'], case['smu0'])
    one = maps.sensitivity_diagonal(*args, case['W_eff'])
    three = maps.sensitivity_diagonal(*args, case['W_eff'], components=True)
    assert one.shape == (2, 3, 4) and one.flags.f_contiguous and len(three) == 3
    # linear in the weights, pair by pair
    parts = np.zeros((2, 3, 4))
    for ba, bf in zip(*np.nonzero(case['W_eff'])):
        w = np.zeros((3, 3))
        w[ba, bf] = case['W_eff'][ba, bf]
        parts = parts + maps.sensitivity_diagonal(*args, w)
    assert np.array_equal(parts, one)
    assert np.array_equal(maps.sensitivity_diagonal(*args, np.zeros((3, 3))), np.zeros((2, 3, 4)))
    with pytest.raises(ValueError):
        maps.sensitivity_diagonal(*args, case['W_eff'][:2])
