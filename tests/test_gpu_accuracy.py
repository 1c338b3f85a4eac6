"""GPU: the accuracy of every line-solve algebra against an extended-precision truth, per kernel family.

The parity tests compare HIP float64 with the oracle's float64 at 1e-10 on well-conditioned lines.  Here each kernel family -- the scan
kernel with one and two blocks per quad, in one and in several waves per line, its chain form and the fused colour passes; the two-sided
chain kernel at 4, 8 and 12 lines per pair of waves, with two and three prefetch stages, with and without the kept z; the affine kernel
with two and three helpers; the quad-per-line kernels; the one-sided kernel; the thread-per-line kernel; the point smoother -- runs two
sweeps on the benign generator of those tests AND on the hard one (stretched widths, air / resistive / sea-water cells: tests/_hard_cases.py),
both scalar types, x-, y- and z-lines, and is measured against the oracle's smoother in x87 extended precision:

    err(x) = max|x - truth| / max|truth|   (in np.longdouble)
    err(hip) <= 10 * max(err(reference_f64), 16 * 2^-53)

The comparison value is the float64 ORACLE's own error on the same case, never a HIP result.  The factor 10: sound elimination orders
sit at 1 x the reference (2e-12 against 2e-12 on ill-conditioned lines at full size), the two orders the project rejected for accuracy
at 150 x and 5000 x.  The floor covers a few final roundings where the reference is at 10 to 20 ulp.  Every case prints
`family shape direction dtype generator err(ref) err(hip) ratio`, ratio = err(hip) / max(err(ref), floor): what is held below 10.

Which kernel a case runs is asserted by name on the handle (and on the CPU in tests/test_accuracy_plan.py); the residual kernels
k_residual and k_residual_zm are held to the extended amat_x in the same way.

The field is not the only measure: on the layered marine model of tests/_hard_models.py the lines of the air layer are close to singular,
every elimination order is then equally far from the truth in the field, and what tells a sound line solve from an unsound one is the
residual it leaves (`test_layered_sweep_residual`, at the end of this file)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import _hard_cases as hc
import _hard_models as hm

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _lab_build(lab):
    yield


@pytest.fixture(scope="module")
def orc(oracle):
    if not oracle.has_extended():
        pytest.skip("np.longdouble is not the x87 extended format (64-bit significand in 16 bytes)")
    return oracle


def _set_env(monkeypatch, env):
    for k in [k for k in os.environ if k.startswith("EMG3D_") and k != "EMG3D_HIP_LIB"]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # read when a handle is created


def _handle(p, dtype, ordering):
    """A handle on the case's grid and model, source loaded."""
    import emg3d_amd as em
    from emg3d_amd.solver import DeviceMG, MGParameters
    grid = em.TensorMesh([np.array(h) for h in p['h']], origin=(0, 0, 0))
    var = MGParameters(verb=0, cycle='F', sslsolver=False, linerelaxation=True, semicoarsening=True, vnC=grid.vnC, ordering=ordering)
    dev = DeviceMG(grid, SimpleNamespace(eta_x=p['eta'][0], eta_y=p['eta'][1], eta_z=p['eta'][2], zeta=p['zeta']), np.dtype(dtype))
    dev.set_params(var)
    dev.set_sfield(p['s'])
    return dev


def _report(family, shape, direction, dtype, kind, e_ref, e_hip):
    ratio = e_hip / max(e_ref, hc.FLOOR)
    print(f"[accuracy] {family} {shape} dir {direction} {hc.tname(dtype)} {kind} err(ref) {e_ref:.2e} err(hip) {e_hip:.2e} "
          f"ratio {ratio:.2f}")
    return None if e_hip <= hc.bound(e_ref) else (family, shape, direction, kind, e_ref, e_hip, ratio)


def _smooth_case(orc, dtype, ordering, shape, direction, kind, want, fused=None, capfd=None):
    """Two sweeps on the device against the truth; returns the failure record or None.  Asserts the kernel by name."""
    p, ref, truth = hc.references(orc, kind, shape, direction, dtype, order=1 if ordering == "colour" else 0)
    with _handle(p, dtype, ordering) as dev:
        dev.set_efield(p['e0'])
        if capfd is not None:
            print(capfd.readouterr().out, end="")
        dev.smooth(2, direction)
        e = dev.get_efield()
        name = dev.last_sweep_kernel()
    if fused is not None:
        out = capfd.readouterr()
        print(out.out, end="")          # (the lines this test printed so far: reading the launch log took them along)
        assert ("fused passes" in out.err) == fused, (shape, direction, fused, out.err[-300:])
    assert name.startswith(want) if want else name == "", (shape, direction, name, want)
    assert np.isfinite(e).all() and not np.array_equal(e, p['e0'])
    return _report(name or "k_point_sweep", shape, direction, dtype, kind, hc.err(ref, truth), hc.err(e, truth))


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=hc.tname)
@pytest.mark.parametrize("case", hc.SWEEP_CASES, ids=[c["name"] for c in hc.SWEEP_CASES])
def test_line_sweeps(orc, lab, monkeypatch, request, case, dtype):
    fused = case["fused"]
    capfd = request.getfixturevalue("capfd") if fused is not None else None         # (the launch log is the library's stderr)
    _set_env(monkeypatch, dict(case["env"], **({"EMG3D_LOG": "1"} if fused is not None else {})))
    prev = lab.use(lab.LAB_PATH if case["library"] == "lab" else lab.LIB_PATH)
    try:
        bad = []
        for shape, direction in case["runs"]:
            for kind in ("benign", "hard"):
                bad.append(_smooth_case(orc, dtype, case["ordering"], shape, direction, kind, case["kernel"].format(t=hc.tname(dtype)),
                                        fused, capfd))
    finally:
        lab.use(prev)
    bad = [b for b in bad if b]
    assert not bad, bad


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=hc.tname)
@pytest.mark.parametrize("shape,ordering", hc.POINT_CASES)
def test_point_smoother(orc, monkeypatch, shape, ordering, dtype):
    _set_env(monkeypatch, {})
    bad = [_smooth_case(orc, dtype, ordering, shape, 0, kind, None) for kind in ("benign", "hard")]
    bad = [b for b in bad if b]
    assert not bad, bad


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=hc.tname)
@pytest.mark.parametrize("kernel,env", hc.RESIDUAL_CASES, ids=["k_residual", "k_residual_zm"])
@pytest.mark.parametrize("shape", hc.RESIDUAL_SHAPES)
def test_residual(orc, monkeypatch, shape, kernel, env, dtype):
    """s - A e of the hard model against the extended amat_x; the comparison value is the float64 oracle's amat_x error."""
    _set_env(monkeypatch, env)
    p = hc.problem("hard", shape, 0, dtype)
    key = ("residual", shape, np.dtype(dtype).char)
    if key not in hc._cache:
        hc._cache[key] = (hc._frozen(hc.amat_x(orc, p, p['e0'])), hc._frozen(hc.amat_x(orc, p, p['e0'], ext=True)))
    ref, truth = hc._cache[key]
    with _handle(p, dtype, "colour") as dev:
        dev.set_efield(p['e0'])
        r = dev.get_residual()
        name = dev.last_residual_kernel()
    assert name == kernel.format(t=hc.tname(dtype)), name
    assert np.isfinite(r).all() and np.abs(r).max() > 0
    bad = _report(name, shape, 0, dtype, "hard", hc.err(ref, truth), hc.err(r, truth))
    assert not bad, bad


class OffTheBound(AssertionError):
    """A measure above hc.bound: the only failure the expected-failure marks below stand for."""


# ---- the residual a line solve leaves on the layered model -------------------------------------------------------------------------
# Found by tests/test_gpu_cycle_accuracy.py and isolated here (tests/_hard_models.py, `sweep_references`): one smoothing call of two
# sweeps on level 0 of the layered 16 x 16 x 16 model, started from the field after the first cycle.  Lines in the air layer are
# close to singular; every kernel, like the float64 oracle, is then 1e-8 from the truth in the field -- the measure of the tests
# above --, but only the one-sided eliminations (the oracle's order: k_line_sweep_qc, _rp, the thread-per-line kernel) leave the
# oracle's residual, 1e-13 ||s||.  The scan kernel and the two-sided kernel leave 1e-7 ... 1e-6 ||s||, in the air cells.
_KNOWN = ("known defect (profiles/HISTORY.md, part T): ||A (e - e_truth)|| / ||s|| after one smoothing call, x- / y- / z-lines, measured on an "
          "MI355X against the float64 oracle's 6e-14 ... 8e-14: ")
LAYERED_SWEEP_CASES = [
    ("qpl", "product", {}, "k_line_sweep_qpl<{t},1,1>", _KNOWN + "complex 7.0e-7 / 1.1e-7 / 2.4e-7, float64 9.5e-7 / 9.3e-8 / 2.8e-7"),
    ("thm", "lab", dict(hc._THM), "k_line_sweep_thm<{t},3,8>", _KNOWN + "complex 2.5e-8 / 6.8e-7 / 3.7e-12, float64 1.3e-8 / 5.1e-7 / 2.3e-12"),
    ("qc", "lab", dict(hc._QOFF, EMG3D_Q="2"), "k_line_sweep_qc<{t},3,4>", None),
    ("rp", "lab", dict(hc._QOFF, EMG3D_TWIST="0", EMG3D_LPW="4"), "k_line_sweep_rp<{t},4>", None),
    ("tpl", "lab", {"EMG3D_SWEEP": "tpl"}, "k_line_sweep<{t}>", None),
]


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=hc.tname)
@pytest.mark.parametrize("name,library,env,kernel,known", [
    pytest.param(*c, marks=[pytest.mark.xfail(strict=True, raises=OffTheBound, reason=c[4])] if c[4] else [], id=c[0]) for c in LAYERED_SWEEP_CASES])
def test_layered_sweep_residual(orc, lab, monkeypatch, name, library, env, kernel, known, dtype):
    """err(hip) <= hc.bound(err(float64 oracle)) for the field AND for the residual ||A (e - e_truth)|| / ||s||, per direction."""
    _set_env(monkeypatch, env)
    prev = lab.use(lab.LAB_PATH if library == "lab" else lab.LIB_PATH)
    bad = []
    try:
        for direction in (1, 2, 3):
            p, truth, e_ref = hm.sweep_references(orc, dtype, direction)
            with _handle(p, dtype, "colour") as dev:
                dev.set_efield(p['e0'])
                dev.smooth(2, direction)
                e = dev.get_efield()
                got = dev.last_sweep_kernel()
            assert got.startswith(kernel.format(t=hc.tname(dtype))), (direction, got)
            assert np.isfinite(e).all() and not np.array_equal(e, p['e0'])
            e_hip = hm.sweep_errors(orc, p, e, truth)
            for m in ("field", "anorm"):
                bad.append(_report(got, hm.SWEEP_SHAPE, direction, dtype, "layered-" + m, e_ref[m], e_hip[m]))
    finally:
        lab.use(prev)
    bad = [b for b in bad if b]
    if bad:
        raise OffTheBound(bad)
