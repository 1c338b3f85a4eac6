"""CPU: the geometry of the Gram launch of a row store (emg3d_rows_gram_plan / emg3d_rows_gram_job, csrc/rows.hpp) -- host arithmetic,
no GPU needed.

* the K-slabs tile [0, n_cols) exactly once, and the jobs' tile pairs cover every (a, b) with a >= b exactly once;
* the slab partition at a given n_cols is the same for every n_rows (the summation order of G must not depend on it), also past the
  size at which the slab length starts to grow;
* a workgroup's LDS stays within the 160 KB of a gfx950 compute unit;
* the launches the jobs run in (emg3d_rows_gram_batch) hold every job, fit the scratch size, and follow from n_cols and njobs."""
import numpy as np
import pytest

N_ROWS = [1, 15, 16, 17, 255, 256, 257, 700]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from emg3d_amd import _lib
    return _lib


def _n_cols(lib):
    S = lib.rows_gram_plan(1, 1)["slab"]            # the plan's own slab length (of every store up to 256 slabs of it)
    return S, [1, 3, 4, 5, 63, 64, 65, S - 1, S, S + 1, 3 * S + 7]


def _slabs(plan, n_cols):
    return [(s * plan["slab"], min(n_cols, (s + 1) * plan["slab"])) for s in range(plan["nslab"])]


def test_slabs_tile_the_columns_and_do_not_depend_on_the_rows(lib):
    S, cols = _n_cols(lib)
    # ... and past the size at which 256 slabs of S columns no longer suffice: the slab grows, in steps of the staging width
    for n_cols in cols + [256 * S, 256 * S + 1, 6_291_456, 2 ** 31 + 5]:
        first = None
        for n_rows in N_ROWS:
            plan = lib.rows_gram_plan(n_rows, n_cols)
            slabs = _slabs(plan, n_cols)
            assert slabs[0][0] == 0 and slabs[-1][1] == n_cols and all(a < b for a, b in slabs)
            assert all(slabs[k][1] == slabs[k + 1][0] for k in range(len(slabs) - 1))
            assert plan["slab"] % plan["kstep"] == 0 and plan["nslab"] <= 256
            assert plan["grid"] == plan["njobs"] * plan["nslab"]
            assert 0 < plan["lds_bytes"] <= 160 * 1024
            first = first or slabs
            assert slabs == first
    assert lib.rows_gram_plan(3, 256 * S)["slab"] == S and lib.rows_gram_plan(3, 256 * S + 1)["slab"] == S + 16


@pytest.mark.parametrize("n_rows", N_ROWS)
def test_jobs_cover_the_lower_triangle_once(lib, n_rows):
    plan = lib.rows_gram_plan(n_rows, 5)
    tile, block = plan["tile"], plan["block"]
    assert block % tile == 0 and plan["nblocks"] == -(-n_rows // block) and plan["njobs"] == len(plan["jobs"])
    nt = -(-n_rows // tile)
    seen = np.zeros((nt, nt), dtype=int)            # tile pairs
    for a0, a1, b0, b1 in plan["jobs"]:
        assert a0 % block == 0 and b0 % block == 0 and a0 >= b0 and a0 < a1 <= n_rows and b0 < b1 <= n_rows
        assert a1 - a0 <= block and b1 - b0 <= block
        for ta in range(a0 // tile, -(-a1 // tile)):
            for tb in range(b0 // tile, -(-b1 // tile)):
                if a0 != b0 or ta >= tb:            # a diagonal job computes the pairs ta >= tb of its block only
                    seen[ta, tb] += 1
    want = np.tril(np.ones((nt, nt), dtype=int))
    assert np.array_equal(seen, want)
    # element-wise: every (a, b), a >= b, lies in a covered tile pair
    a, b = np.tril_indices(n_rows)
    assert np.all(seen[a // tile, b // tile] == 1)


def test_jobs_per_launch(lib):
    """emg3d_rows_gram_batch, the arithmetic emg3d_rows_gram runs its launches by: the launches hold all jobs, each holds at least one,
    the partials of one launch fit the scratch size (unless a single job does not), and jobs_per_launch depends on n_rows through
    njobs only: it is min(njobs, a function of n_cols)."""
    S, cols = _n_cols(lib)
    for n_cols in cols + [15 * S + 9, 256 * S, 256 * S + 1, 128 ** 3, 6_291_456, 2 ** 31 + 5]:
        fit = None
        for n_rows in N_ROWS + [1024, 1925, 5000]:
            plan = lib.rows_gram_plan(n_rows, n_cols)
            jpl, launches = plan["jobs_per_launch"], plan["launches"]
            assert jpl >= 1 and launches == -(-plan["njobs"] // jpl)
            assert plan["job_bytes"] == 64 * plan["nslab"] * 256 * 8 and plan["scratch_bytes"] > 0
            assert jpl * plan["job_bytes"] <= plan["scratch_bytes"] or jpl == 1
            # the most that fit, and that number is the same for every n_rows
            cap = max(1, plan["scratch_bytes"] // plan["job_bytes"])
            assert jpl == min(plan["njobs"], cap)
            fit = fit or cap
            assert cap == fit
    # today's constants: 256 slabs make a job 32 MiB, 8 of them a launch; 16 slabs 2 MiB and 128
    assert lib.rows_gram_plan(385, 128 ** 3)["jobs_per_launch"] == 8 and lib.rows_gram_plan(385, 128 ** 3)["launches"] == 2
    assert lib.rows_gram_plan(384, 128 ** 3)["launches"] == 1
    p = lib.rows_gram_plan(1925, 15 * S + 9)
    assert (p["njobs"], p["jobs_per_launch"], p["launches"]) == (136, 128, 2)


def test_bad_arguments(lib):
    import ctypes
    out = (ctypes.c_int64 * 8)()
    h = lib.load()
    assert h.emg3d_rows_gram_batch(0, 5, out) == -2 and h.emg3d_rows_gram_batch(5, 0, out) == -2
    assert h.emg3d_rows_gram_batch(5, 5, None) == -2 and h.emg3d_rows_gram_batch(5, 5, out) == 0
    assert h.emg3d_rows_gram_plan(0, 5, out) == -2 and h.emg3d_rows_gram_plan(5, 0, out) == -2
    assert h.emg3d_rows_gram_plan(5, 5, None) == -2
    assert h.emg3d_rows_gram_job(5, 1, out) == -2 and h.emg3d_rows_gram_job(5, -1, out) == -2 and h.emg3d_rows_gram_job(5, 0, out) == 0
