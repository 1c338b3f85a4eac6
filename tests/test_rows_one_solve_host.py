"""CPU: the one-solve form of the rows of J (SurveyJacobian.sensitivity_rows / park_rows with solves=1, k_sens_rows_fill) -- no GPU needed.

* the ROTATION IDENTITY behind it, on the numpy restatement: the product jtvec(i e_d) forms is maps.sensitivity_rows(grid, fwd,
  -1j * adj, smu0) (the adjoint source of a datum weight w is scaled by conj(w)), and its real part is the imaginary part of
  maps.sensitivity_rows(grid, fwd, adj, smu0) -- to rounding, never bit for bit, which is why the default solves twice and why the
  one-solve form promises its imaginary parts to the rounding of the solves only;
* the checks of ``solves`` that need no device;
* the compiler's resource report of the four instantiations of k_sens_rows_fill (csrc/rows.hip)."""
import numpy as np
import pytest

from test_sensitivity_rows_host import TOL_ROWS_KERNEL, rows_case

ROTATION_SHAPES = [(5, 6, 7), (2, 3, 4), (9, 4, 2), (7, 6, 7)]


@pytest.mark.parametrize("components", [False, True], ids=["sum", "components"])
@pytest.mark.parametrize("nsys", [1, 3])
@pytest.mark.parametrize("shape", ROTATION_SHAPES, ids=str)
def test_rotation_identity(shape, nsys, components):
    """Re rows(fwd, -1j adj) == Im rows(fwd, adj) within TOL_ROWS_KERNEL of the row's largest magnitude (both sides are the same
    twelve-term sums with the parts of one operand swapped: the yardstick of the restatement against itself in longdouble, with its
    margin), and the two are NOT the same bits (measured: at most 3.6e-16)."""
    from emg3d_amd import maps
    case = rows_case(shape, False, nsys)
    fwd, adj = case['fwd'][case['jf']], case['adj'][case['ia']]
    rows = maps.sensitivity_rows(case['grid'], fwd, adj, case['smu0'], components=components)
    rotated = maps.sensitivity_rows(case['grid'], fwd, -1j * adj, case['smu0'], components=components)
    assert rows.shape == rotated.shape == (len(case['pairs']), 3 if components else 1) + shape
    size = np.abs(rows).reshape(rows.shape[:2] + (-1,)).max(axis=2)
    gap = float((np.abs(rotated.real - rows.imag).reshape(rows.shape[:2] + (-1,)).max(axis=2) / size).max())
    print(f"{shape} nsys {nsys} components {components}: Re rows(-1j adj) vs Im rows(adj) {gap:.2e} (tolerance {TOL_ROWS_KERNEL:.1e})")
    assert size.min() > 0 and gap <= TOL_ROWS_KERNEL
    assert not np.array_equal(rotated.real, rows.imag)
    # the other half of the rotation, for the sign convention: Im rows(-1j adj) == -Re rows(adj)
    assert float((np.abs(rotated.imag + rows.real).reshape(rows.shape[:2] + (-1,)).max(axis=2) / size).max()) <= TOL_ROWS_KERNEL


def test_solves_is_checked_without_a_device():
    """``solves`` other than 1 or 2 raises ValueError in both methods before any device call (the objects are never opened: a valid
    ``solves`` reaches the refusal of the closed object), with and without a model grid."""
    import emg3d_amd as em
    h = [np.array([95., 70., 52., 40., 44., 57., 76., 104.])] * 3
    grid = em.TensorMesh(h, origin=(-269., -269., -269.))
    rec = (np.array([-55., 30., 5.]), np.array([12., -44., 50.]), np.array([-20., 35., -8.]), np.zeros(3), np.zeros(3))
    model = em.Model(grid, np.ones(grid.nC), mapping='Conductivity')
    sj = em.optimize.SurveyJacobian(grid, model, [[0., 0., 0., 0., 0.]], [1.0, -2.0], rec, batch=2)
    coarse = em.TensorMesh([np.array([x[0:4].sum(), x[4:8].sum()]) for x in h], origin=grid.origin)
    cmodel = em.Model(coarse, np.ones(coarse.nC), mapping='Conductivity')
    sjm = em.optimize.SurveyJacobian(grid, cmodel, [[0., 0., 0., 0., 0.]], [1.0], rec, batch=1, model_grid=coarse)
    for obj, kw in ((sj, {}), (sjm, dict(mapped=True))):
        for bad in (0, 3, 'one', None, True, 1.0, -1):
            with pytest.raises(ValueError, match="solves"):
                obj.sensitivity_rows(0, solves=bad, **kw)
            with pytest.raises(ValueError, match="solves"):
                obj.park_rows(solves=bad, **kw)
        for good in (1, 2, np.int64(1)):
            with pytest.raises(RuntimeError, match="closed"):
                obj.sensitivity_rows(0, solves=good, **kw)
            with pytest.raises(RuntimeError, match="closed"):
                obj.park_rows(solves=good, **kw)
    # the earlier checks keep their order: a bad `mapped` is named first, a bad `i_freq` after `solves`
    with pytest.raises(TypeError, match="mapped"):
        sj.sensitivity_rows(0, mapped=1, solves=0)
    with pytest.raises(ValueError, match="solves"):
        sj.sensitivity_rows(7, solves=0)
    with pytest.raises(ValueError, match="i_freq"):
        sj.sensitivity_rows(7, solves=1)


def test_fill_kernel_uses_no_scratch_and_no_lds(tmp_path):
    """The compiler's resource remarks for the four instantiations of k_sens_rows_fill on gfx950 (csrc/rows.hip, the unit that
    instantiates it): no scratch, no LDS; the VGPR counts and waves per SIMD are printed, DESIGN 8.13 states them (needs hipcc, not
    a GPU)."""
    import os
    import shutil
    import subprocess
    import __graft_entry__ as g
    from conftest import ROOT
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = subprocess.run([hipcc] + g.FLAGS + ["-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "rows.o"),
                          os.path.join(ROOT, "emg3d_amd", "csrc", "rows.hip")], capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    keys = ("ScratchSize [bytes/lane]:", " VGPRs:", "Occupancy [waves/SIMD]:", "LDS Size [bytes/block]:")
    name, seen = None, {}
    for line in out.stderr.splitlines():
        if "Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
        elif name and "k_sens_rows_fill" in name:
            for key in keys:
                if key in line:
                    seen.setdefault(name, {})[key.strip()] = int(line.split(key)[1].split()[0])
    print(seen)
    assert len(seen) == 4 and all(len(v) == len(keys) for v in seen.values()), seen
    assert all(v["ScratchSize [bytes/lane]:"] == 0 and v["LDS Size [bytes/block]:"] == 0 for v in seen.values()), seen
