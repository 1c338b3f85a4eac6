"""CPU-only: every case of tests/test_gpu_accuracy.py selects the kernel it is named after (tests/_hard_cases.py SWEEP_CASES).

The accuracy tests hold one elimination algebra each to the extended-precision truth; which kernel a (shape, direction) runs is the
planner's answer (csrc/sweep_plan.hpp, exported as emg3d_sweep_plan and emg3d_sweep_fuse_plan: shape logic, no GPU) under the case's
library and variables.  Checked here for a device of 256 compute units, so that a change of the planner that moves a case to another
family shows on the CPU, not as a wrong name on the GPU."""
import os

import pytest

import _hard_cases as hc

CUS = 256
NPASS = 7           # colour passes of a smoothing call of two sweeps (the turn-around's repeated colour skipped)


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


@pytest.mark.parametrize("case", hc.SWEEP_CASES, ids=[c["name"] for c in hc.SWEEP_CASES])
def test_case_selects_its_kernel(lib, monkeypatch, case):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    prev = lib.use(lib.LAB_PATH if case["library"] == "lab" else None)
    try:
        for dtype in hc.DTYPES:
            for shape, direction in case["runs"]:
                p = lib.sweep_plan(shape, direction, dtype=dtype, ordering=case["ordering"], cu_count=CUS)
                want = case["kernel"].format(t=hc.tname(dtype))
                assert p["kernel"].startswith(want), (case["name"], shape, direction, p["kernel"], want)
                assert not p["split"]
                f = lib.sweep_fuse_plan(shape, direction, NPASS, dtype=dtype, ordering=case["ordering"], cu_count=CUS)
                if case["fused"] is not None:
                    assert f["fused"] == case["fused"], (case["name"], shape, direction, f)
    finally:
        lib.use(prev)


@pytest.mark.parametrize("case", hc.SWEEP_CASES, ids=[c["name"] for c in hc.SWEEP_CASES])
def test_case_selects_its_kernel_with_three_systems(lib, monkeypatch, case):
    """What tests/test_gpu_batch_families.py runs: the narrow runs and the wide ones (same lines, 36 x 36 of them) in a batch of three
    stay with the case's kernel and its way of issuing the passes, and the wide runs keep their 324 lines per colour (fused_scan: 100)
    -- more line blocks than XCDs in every family's launch, which is what they are for."""
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    prev = lib.use(lib.LAB_PATH if case["library"] == "lab" else None)
    wide = hc.wide_runs(case)
    assert [d for _, d in wide] == [d for _, d in case["runs"]]
    try:
        for dtype in hc.DTYPES:
            want = case["kernel"].format(t=hc.tname(dtype))
            for is_wide, runs in ((False, case["runs"]), (True, wide)):
                for (shape, direction), (narrow, _) in zip(runs, case["runs"]):
                    p = lib.sweep_plan(shape, direction, dtype=dtype, ordering=case["ordering"], nsys=3, cu_count=CUS)
                    assert p["kernel"].startswith(want), (case["name"], shape, direction, p["kernel"], want)
                    assert not p["split"]
                    f = lib.sweep_fuse_plan(shape, direction, NPASS, dtype=dtype, ordering=case["ordering"], nsys=3, cu_count=CUS)
                    if case["fused"] is not None:
                        assert f["fused"] == case["fused"], (case["name"], shape, direction, f)
                    if is_wide:
                        assert shape[direction - 1] == narrow[direction - 1]
                        lines = 100 if case["name"] == "fused_scan" else 324
                        assert p["lines_per_colour"] == lines, (case["name"], shape, direction, p)
    finally:
        lib.use(prev)


def test_cases_cover_the_families_and_the_directions():
    fams = {c["kernel"].split("<")[0] for c in hc.SWEEP_CASES}
    assert fams == {"k_line_sweep", "k_line_sweep_rp", "k_line_sweep_qc", "k_line_sweep_qc_big", "k_line_sweep_thm", "k_line_sweep_tha",
                    "k_line_sweep_qpl", "k_line_sweep_qpl_chain"}
    for c in hc.SWEEP_CASES:
        assert {d for _, d in c["runs"]} == {1, 2, 3}, c["name"]
    assert len({c["name"] for c in hc.SWEEP_CASES}) == len(hc.SWEEP_CASES)


def test_kept_z_is_on_and_off_as_the_thm_cases_say(lib, monkeypatch):
    """The `_zkeep` cases keep forward results in LDS, the `_parked` cases (EMG3D_THM_ZKEEP=0) none."""
    prev = lib.use(lib.LAB_PATH)
    try:
        for case in hc.SWEEP_CASES:
            if not case["kernel"].startswith("k_line_sweep_thm<"):
                continue
            with monkeypatch.context() as mp:
                for k, v in case["env"].items():
                    mp.setenv(k, v)
                for dtype in hc.DTYPES:
                    for shape, direction in case["runs"]:
                        z = lib.sweep_thm_zkeep(shape, direction, dtype=dtype, cu_count=CUS)
                        assert (z["kept"] > 0) == case["name"].endswith("_zkeep"), (case["name"], shape, z)
    finally:
        lib.use(prev)
