"""CPU-only: how many forward steps of a half keep their z in LDS in the two-sided chain kernel (csrc/sweep_plan.hpp
sweep_thm_zkeep, exported as emg3d_sweep_thm_zkeep).

k_line_sweep_thm parks the forward result z of every step in the field and loads it again on the way back; the last steps of a half
keep it in LDS instead.  The planner answers how many: the longest half, or what fits beside the instantiation's static LDS in the
160 KB of a workgroup.  Checked here, without a GPU: the depths of the shapes the design was reasoned on, zero where another kernel
family serves, that the depth follows the family when the device's size changes it, the phase rule (the first kept step is a
multiple of the prefetch depth), the lab build's cap, and that the kernel selection (emg3d_sweep_plan) answers as before."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

CUS = 256
LDS = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from emg3d_amd import _lib
    prev = _lib.use(None)
    yield _lib
    _lib.use(prev)


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in [k for k in os.environ if k.startswith("EMG3D_") and k != "EMG3D_HIP_LIB"]:
        monkeypatch.delenv(k)


def _step_bytes(lpw, tsize):
    return 4 * 5 * lpw * tsize          # 4 waves x 5 rows x lines per pair of waves


def _static(lpw, tsize):
    return (4 * 2 * 64 + 2 * 3 * 6 * lpw) * tsize       # exchange buffers of the 4 waves + the middle join of the 2 pairs


def _check_consistent(z, tsize, unroll=3):
    """The answer against the documented rule, from its own fields."""
    lpw = z["lines_per_pair"]
    assert z["static_lds_bytes"] == _static(lpw, tsize)
    assert z["cap"] == min(z["half"], (LDS - _static(lpw, tsize)) // _step_bytes(lpw, tsize))
    assert z["dyn_lds_bytes"] == z["cap"] * _step_bytes(lpw, tsize)
    assert z["dyn_lds_bytes"] + z["static_lds_bytes"] <= LDS
    first = z["half"] - z["kept"]
    assert 0 <= z["kept"] <= z["cap"] and (first % unroll == 0 or z["kept"] == 0)
    assert z["cap"] - z["kept"] < unroll


def test_128_c128_keeps_nearly_the_half(lib):
    for d in (1, 2, 3):
        assert lib.sweep_plan((128, 128, 128), d, cu_count=CUS)["kernel"] == "k_line_sweep_thm<c128,3,8>"
        z = lib.sweep_thm_zkeep((128, 128, 128), d, cu_count=CUS)
        assert z["half"] == 63 and z["lines_per_pair"] == 8
        assert 57 <= z["kept"] <= z["cap"] <= 59
        assert z["dyn_lds_bytes"] + z["static_lds_bytes"] <= LDS
        assert z["static_lds_bytes"] == 8192 + 4608
        _check_consistent(z, 16)


def test_128_f64_keeps_the_whole_half(lib):
    z = lib.sweep_thm_zkeep((128, 128, 128), 3, dtype=np.float64, cu_count=CUS)
    assert z["cap"] == z["kept"] == z["half"] == 63
    _check_consistent(z, 8)


def test_144_c128_at_12_lines_per_pair(lib):
    z = lib.sweep_thm_zkeep((144, 144, 144), 3, cu_count=CUS)
    assert lib.sweep_plan((144, 144, 144), 3, cu_count=CUS)["kernel"] == "k_line_sweep_thm<c128,3,12>"
    assert z["lines_per_pair"] == 12 and z["half"] == 71
    assert 36 <= z["kept"] <= z["cap"] <= 39
    _check_consistent(z, 16)


def test_long_lines_keep_the_cap(lib):
    z = lib.sweep_thm_zkeep((16, 16, 1200), 3, cu_count=CUS)
    assert lib.sweep_plan((16, 16, 1200), 3, cu_count=CUS)["kernel"].startswith("k_line_sweep_thm<c128")
    assert z["half"] == 599 and z["cap"] == (LDS - z["static_lds_bytes"]) // _step_bytes(z["lines_per_pair"], 16)
    assert z["cap"] - 2 <= z["kept"] <= z["cap"] < z["half"]
    _check_consistent(z, 16)


@pytest.mark.parametrize("shape, direction, family", [
    ((128, 128, 64), 1, "k_line_sweep_tha"), ((128, 128, 64), 2, "k_line_sweep_tha"), ((96, 96, 64), 3, "k_line_sweep_tha"),
    ((32, 32, 32), 3, "k_line_sweep_qpl"), ((128, 4, 4), 2, "k_line_sweep_qpl_chain"), ((256, 256, 256), 3, "k_line_sweep_qc")])
def test_other_families_keep_nothing(lib, shape, direction, family):
    for dtype in (np.complex128, np.float64):
        assert lib.sweep_plan(shape, direction, dtype=dtype, cu_count=CUS)["kernel"].split("<")[0] == family
        z = lib.sweep_thm_zkeep(shape, direction, dtype=dtype, cu_count=CUS)
        assert z == {"cap": 0, "dyn_lds_bytes": 0, "static_lds_bytes": 0, "half": 0, "kept": 0, "lines_per_pair": 0}


def test_keep_follows_the_family_across_device_sizes(lib):
    """Half the compute units: 128^3 goes to the quad kernel (4096 lines per colour = 8 per wave on 512 SIMDs) and keeps nothing;
    whatever emg3d_sweep_plan says, the keep is on exactly where it names k_line_sweep_thm."""
    changed = 0
    for shape in [(128, 128, 128), (144, 144, 144), (96, 96, 96), (128, 128, 64), (92, 92, 66), (16, 16, 1200), (64, 64, 64)]:
        for d in (1, 2, 3):
            for nsys in (1, 4):
                fam = []
                for cus in (CUS, CUS // 2):
                    p = lib.sweep_plan(shape, d, nsys=nsys, cu_count=cus)
                    z = lib.sweep_thm_zkeep(shape, d, nsys=nsys, cu_count=cus)
                    thm = p["kernel"].startswith("k_line_sweep_thm<")
                    assert (z["cap"] > 0) == thm and (z["kept"] > 0) == thm, (shape, d, nsys, cus, p, z)
                    if thm:
                        assert z["lines_per_pair"] == p["lines_per_wave"]
                        _check_consistent(z, 16)
                    fam.append(p["kernel"].split("<")[0])
                changed += fam[0] != fam[1]
    assert lib.sweep_plan((128, 128, 128), 3, cu_count=CUS // 2)["kernel"].startswith("k_line_sweep_qc<")
    assert lib.sweep_thm_zkeep((128, 128, 128), 3, cu_count=CUS // 2)["cap"] == 0
    assert changed >= 3


def test_batched_systems_keep_the_same_depth_per_instantiation(lib):
    """The system index does not enter the slot: a batched launch keeps what its instantiation (lines per pair) has room for."""
    for nsys in (1, 2, 4, 8):
        z = lib.sweep_thm_zkeep((128, 128, 128), 3, nsys=nsys, cu_count=CUS)
        assert z["lines_per_pair"] == lib.sweep_plan((128, 128, 128), 3, nsys=nsys, cu_count=CUS)["lines_per_wave"]
        _check_consistent(z, 16)
        assert z["kept"] >= 36


def test_lab_cap_and_phase_rule(lib, monkeypatch):
    """EMG3D_THM_ZKEEP (lab build): -1 as many as fit, 0 off, n at most n; the first kept step is a multiple of the prefetch depth
    (3, or 2 with EMG3D_TW_STAGES=2), so a cap that is not leaves up to depth - 1 steps unused."""
    prev = lib.use(lib.LAB_PATH)
    try:
        full = lib.sweep_thm_zkeep((128, 128, 128), 3, cu_count=CUS)
        assert full == dict(full, cap=59, kept=57)
        for stages, unroll in (("3", 3), ("2", 2)):
            monkeypatch.setenv("EMG3D_TW_STAGES", stages)
            for half_shape, half in (((128, 128, 128), 63), ((24, 24, 7), 3), ((7, 5, 17), 8), ((6, 5, 33), 16)):
                for cap in (-1, 0, 1, 2, 3, 4, 5, 15, 30, 45, 100):
                    monkeypatch.setenv("EMG3D_THM_ZKEEP", str(cap))
                    monkeypatch.setenv("EMG3D_QPL", "0")
                    monkeypatch.setenv("EMG3D_THA", "0")
                    z = lib.sweep_thm_zkeep(half_shape, 3, cu_count=CUS)
                    assert lib.sweep_plan(half_shape, 3, cu_count=CUS)["kernel"].startswith("k_line_sweep_thm<c128," + stages)
                    assert z["half"] == half
                    want_cap = min(half, 59) if cap < 0 else min(half, 59, cap)
                    assert z["cap"] == want_cap
                    first = half if want_cap == 0 else 0 if half <= want_cap else min(half, -(-(half - want_cap) // unroll) * unroll)
                    assert z["kept"] == half - first, (half_shape, stages, cap, z)
    finally:
        lib.use(prev)


def test_product_library_ignores_the_lab_variable(lib, monkeypatch):
    monkeypatch.setenv("EMG3D_THM_ZKEEP", "0")
    assert lib.sweep_thm_zkeep((128, 128, 128), 3, cu_count=CUS)["kept"] == 57


def test_invalid_arguments(lib):
    with pytest.raises(lib.HipLibraryError):
        lib.sweep_thm_zkeep((128, 128, 128), 4, cu_count=CUS)
    with pytest.raises(lib.HipLibraryError):
        lib.sweep_thm_zkeep((128, 1, 128), 3, cu_count=CUS)


def test_kernel_selection_unchanged(lib, monkeypatch):
    """emg3d_sweep_plan against the table recorded before this planner existed (tests/golden/sweep_plans.json): every row, both
    libraries."""
    with open(os.path.join(GOLDEN, "sweep_plans.json")) as fh:
        fix = json.load(fh)
    n = 0
    prev = lib.use(None)
    try:
        for group in fix["groups"]:
            lib.use(lib.LAB_PATH if group["library"] == "lab" else None)
            with monkeypatch.context() as mp:
                for k, v in group["env"].items():
                    mp.setenv(k, v)
                for nx, ny, nz, d, dt, ordering, nsys, cu, *want in group["rows"]:
                    p = lib.sweep_plan((nx, ny, nz), d, dtype=np.complex128 if dt == "c128" else np.float64, ordering=ordering,
                                       nsys=nsys, cu_count=cu)
                    got = [p["kernel"], p["lines_per_colour"], p["lines_per_wave"], p["rounds"], p["factor_kind"], int(p["split"]),
                           int(p["big_offsets"])]
                    assert got == want, (group["library"], group["env"], (nx, ny, nz), d, dt, ordering, nsys, cu, got, want)
                    n += 1
    finally:
        lib.use(prev)
    assert n >= 400
