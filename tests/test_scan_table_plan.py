"""CPU-only: where the scan kernel's colour launches load the scanned map matrices from a table (csrc/sweep_plan.hpp sweep_scantab,
exported as emg3d_sweep_scantab, which _lib.sweep_plan folds into its answer): shape logic of the product library on a device of 256 CUs, no GPU."""
import numpy as np
import pytest

CUS = 256


@pytest.fixture(scope="module")
def lib():
    from emg3d_amd import _lib
    return _lib


def test_short_lines_of_the_flagship_cycle_are_admitted(lib):
    """128 x 8 x 8 (level 4 of the 128^3 F-cycle with semicoarsening): the 8-block y- and z-lines, 8192 threads per colour launch,
    256 B per lane at complex128 in each of the four colours' tables; the 128-block x-lines belong to another kernel form."""
    for d in (2, 3):
        p = lib.sweep_plan((128, 8, 8), d, cu_count=CUS)
        assert p["kernel"] == "k_line_sweep_qpl<c128,1,1>" and p["scan_table"]
        assert p["scan_table_bytes"] == 4 * 8192 * 256
    p = lib.sweep_plan((128, 8, 8), 1, cu_count=CUS)
    assert not p["scan_table"] and p["scan_table_bytes"] == 0
    p = lib.sweep_plan((128, 8, 8), 2, dtype=np.float64, cu_count=CUS)
    assert p["scan_table"] and p["scan_table_bytes"] == 4 * 8192 * 128


def test_a_launch_above_the_size_limit_is_refused(lib):
    """16-block lines, 4096 lines per colour = 262 144 threads: the kernel form has a table (its size is reported), the size rule
    refuses it; the threshold follows the device."""
    p = lib.sweep_plan((128, 128, 16), 3, cu_count=CUS)
    assert p["kernel"] == "k_line_sweep_qpl<c128,1,1>"
    assert not p["scan_table"] and p["scan_table_bytes"] == 4 * 262144 * 384
    assert lib.sweep_plan((64, 16, 16), 3, cu_count=CUS)["scan_table"]
    assert not lib.sweep_plan((64, 16, 16), 3, cu_count=CUS // 8)["scan_table"]


def test_other_forms_have_no_table(lib):
    """The chain form (4-block lines), two blocks per quad (32-block lines), lines across several waves, the lexicographic order and
    the other kernel families."""
    for shape, d, kw in (((128, 4, 4), 2, {}), ((32, 32, 32), 1, {}), ((24, 8, 8), 1, {}), ((128, 8, 8), 2, dict(ordering='lex')),
                         ((128, 128, 128), 3, {})):
        p = lib.sweep_plan(shape, d, cu_count=CUS, **kw)
        assert not p["scan_table"] and p["scan_table_bytes"] == 0, (shape, d, p)
