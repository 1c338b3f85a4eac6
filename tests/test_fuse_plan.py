"""CPU-only: the planner of the fused colour passes (csrc/sweep_plan.hpp plan_fuse, exported as emg3d_sweep_fuse_plan).

On levels of short lines that the scan kernel serves, all colour passes of a smoothing call run in ONE launch: a workgroup owns a
slab of line nodes along the longer transverse axis, works on a private copy and recomputes a halo of neighbouring lines that shrinks
by one node per pass; a second launch writes every edge from its owner's copy.  Checked here, without a GPU: the slabs tile the
axis, every edge index has exactly one owner, the live ranges shrink by one and are clamped, a dependency simulation of the passes
finds every owned edge exact at the end, the scratch size is what the documentation says, levels outside the eligibility rules are
not fused, and the kernel selection (emg3d_sweep_plan) answers as it did before the change."""
import numpy as np
import pytest

CUS = 256
SHAPES = [(128, 4, 4), (4, 128, 4), (4, 4, 128), (128, 8, 8), (40, 4, 6), (6, 40, 8), (12, 4, 4)]
# colour c = cP + 2 cQ of the passes of a call of nu sweeps (backward 0,3,2,1 / forward 1,3,0,2, the repeated colour skipped)
SEQ = {1: [0, 3, 2, 1], 2: [0, 3, 2, 1, 3, 0, 2], 3: [0, 3, 2, 1, 3, 0, 2, 0, 3, 2, 1]}


@pytest.fixture(scope="module")
def lib():
    """The lab build: it also has the scan form of the fused loop (8-block lines, `max_seg=8`), which the product library leaves out
    because it lost its A/B (test_levels_outside_the_rules_are_not_fused looks at the product library too)."""
    import __graft_entry__ as g
    g.build()
    from emg3d_amd import _lib
    prev = _lib.use(_lib.LAB_PATH)
    yield _lib
    _lib.use(prev)


def _axes(direction):
    return {1: (1, 2), 2: (0, 2), 3: (0, 1)}[direction]


def _n_edges(n):
    return n[0] * (n[1] + 1) * (n[2] + 1) + (n[0] + 1) * n[1] * (n[2] + 1) + (n[0] + 1) * (n[1] + 1) * n[2]


def _simulate(plan, parities):
    """Which edge indices of each slab's private copy are exact after the passes.  Along the slab axis X a line at node j reads the
    node-type edges at j - 1 .. j + 1 and the X-directed edges at the cells j - 1, j, and writes the node-type edges at j and the
    cells j - 1, j; pass p solves the lines of X-parity parities[p] (node j has parity (j - 1) & 1).  A line that the slab does not
    run, or runs on inexact input, leaves what it writes inexact."""
    nX = plan["nX"]
    res = []
    for sl in plan["slabs"]:
        lo0, hi0 = sl["live"][0]
        node = np.zeros(nX + 1, bool)
        cell = np.zeros(nX, bool)
        node[lo0 - 1:hi0 + 2] = True                      # copied in: indices lo(0) - 1 .. hi(0) + 1
        cell[lo0 - 1:min(hi0 + 1, nX - 1) + 1] = True
        for (lo, hi), par in zip(sl["live"], parities):
            new_node, new_cell = node.copy(), cell.copy()
            for j in range(1, nX):
                if (j - 1) & 1 != par:
                    continue
                ok = lo <= j <= hi and node[j - 1:j + 2].all() and cell[j - 1:j + 1].all()
                new_node[j] = ok
                new_cell[j - 1] = ok
                new_cell[j] = ok
            node, cell = new_node, new_cell
        res.append((node, cell))
    return res


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [np.complex128, np.float64])
def test_slabs_ownership_and_live_ranges(lib, shape, dtype):
    tsize = np.dtype(dtype).itemsize
    seen = 0
    for direction in (1, 2, 3):
        P, Q = _axes(direction)
        for own in (0, 3, 5):
            for nsys in (1, 3):
                for npass in (1, 2, 3, 4, 7, 11, 16, 17):
                    plan = lib.sweep_fuse_plan(shape, direction, npass, dtype=dtype, nsys=nsys, cu_count=CUS, own=own, max_seg=8)
                    nL = shape[direction - 1]
                    nXe = max(shape[P], shape[Q])
                    we = min(own or 2, nXe - 1)
                    # (the private copies of a (level, direction) stay within the default budget of 64 MiB)
                    eligible = 3 <= npass <= 16 and nL <= 8 and nsys * -(-(nXe - 1) // we) * _n_edges(shape) * tsize <= 64 << 20
                    assert plan["fused"] == eligible, (shape, direction, npass, plan)
                    if not plan["fused"]:
                        continue
                    seen += 1
                    # the slab axis is the longer transverse axis (P on a tie)
                    axis = Q if shape[Q] > shape[P] else P
                    nX = shape[axis]
                    assert plan["axis"] == axis and plan["nX"] == nX and plan["npass"] == npass
                    w = plan["own"]
                    assert w == min(own or 2, nX - 1)
                    ns = plan["nslabs"]
                    assert ns == -(-(nX - 1) // w) == len(plan["slabs"])
                    assert plan["scratch_bytes"] == nsys * ns * _n_edges(shape) * tsize
                    x, a = 1, 0
                    for k, sl in enumerate(plan["slabs"]):
                        x0, x1 = sl["own"]
                        assert x0 == x and x0 < x1 <= nX and (x1 - x0 == w or (k == ns - 1 and x1 - x0 <= w))
                        x = x1
                        # owned edge indices: contiguous, the first slab from index 0, the last to nX + 1
                        ea, eb = sl["edges"]
                        assert ea == a and (ea == (0 if k == 0 else x0)) and eb == (nX + 1 if k == ns - 1 else x1)
                        a = eb
                        for p, (lo, hi) in enumerate(sl["live"]):
                            h = npass - 1 - p
                            assert lo == max(1, x0 - h) and hi == min(nX - 1, x1 + h)        # shrink by one per pass, clamped
                        lo, hi = sl["live"][-1]
                        assert lo <= x0 and hi >= min(x1, nX - 1)                            # the own range (and one node more)
                    assert x == nX and a == nX + 1
                    if nsys > 1:
                        continue
                    # dependency simulation: whatever parities the passes have, every owned index is exact at the end
                    for parities in ([p & 1 for p in range(npass)], [(p >> 1) & 1 for p in range(npass)], [0] * npass, [1] * npass,
                                     [(c & 1) for c in (SEQ[3] * 2)[:npass]], [(c >> 1) for c in (SEQ[3] * 2)[:npass]]):
                        for sl, (node, cell) in zip(plan["slabs"], _simulate(plan, parities)):
                            ea, eb = sl["edges"]
                            assert node[ea:min(eb, nX + 1)].all() and cell[ea:min(eb, nX)].all(), (shape, direction, npass, own, sl)
    assert seen


def test_levels_outside_the_rules_are_not_fused(lib):
    f = lambda *a, **k: lib.sweep_fuse_plan(*a, cu_count=CUS, **k)["fused"]
    assert f((128, 4, 4), 2, 7) and f((128, 4, 4), 3, 7)
    assert not f((128, 4, 4), 1, 7, max_seg=8)                      # 128-block lines
    assert not f((128, 4, 4), 2, 7, ordering='lex')                 # lexicographic order
    assert not f((128, 4, 4), 2, 2) and not f((128, 4, 4), 2, 17)   # fewer than 3 passes / more than the pass list holds
    assert not f((128, 8, 8), 2, 7) and f((128, 8, 8), 2, 7, max_seg=8)     # 8-block lines: not by default (profiles/HISTORY.md)
    assert not f((128, 16, 16), 2, 7, max_seg=16)                   # 16-block lines: out of scope
    assert not f((128, 4, 4), 2, 7, budget=100000)                  # private copies over the byte budget
    assert f((128, 4, 4), 2, 7, budget=64 * _n_edges((128, 4, 4)) * 16)           # 64 slabs of two nodes
    assert not f((128, 4, 4), 2, 7, nsys=2, budget=64 * _n_edges((128, 4, 4)) * 16)
    assert not f((1024, 4, 64), 2, 7)                               # more threads per colour launch than the descriptor tables serve
    prev = lib.use(lib.LIB_PATH)                                    # the product library: 4-block lines (chain form) only, whatever is asked
    try:
        assert f((128, 4, 4), 2, 7) and not f((128, 8, 8), 2, 7, max_seg=8) and not f((40, 4, 6), 3, 7, max_seg=8)
    finally:
        lib.use(prev)


# emg3d_sweep_plan for the sample shapes on a 256-CU device, colour order, one system, as the commit before this change answered:
# (shape, direction) -> (kernel c128, kernel f64, lines per colour, lines per workgroup, rounds, factor kind, split, 64-bit offsets)
PARENT_PLANS = {
    ((128, 4, 4), 1): ('k_line_sweep_qpl<c128,4,2>', 'k_line_sweep_qpl<f64,4,2>', 4, 1, 1, 0, False, False),
    ((128, 4, 4), 2): ('k_line_sweep_qpl_chain<c128,1,1>', 'k_line_sweep_qpl_chain<f64,1,1>', 128, 4, 1, 0, False, False),
    ((128, 4, 4), 3): ('k_line_sweep_qpl_chain<c128,1,1>', 'k_line_sweep_qpl_chain<f64,1,1>', 128, 4, 1, 0, False, False),
    ((4, 128, 4), 1): ('k_line_sweep_qpl_chain<c128,1,1>', 'k_line_sweep_qpl_chain<f64,1,1>', 128, 4, 1, 0, False, False),
    ((4, 128, 4), 2): ('k_line_sweep_qpl<c128,4,2>', 'k_line_sweep_qpl<f64,4,2>', 4, 1, 1, 0, False, False),
    ((4, 128, 4), 3): ('k_line_sweep_qpl_chain<c128,1,1>', 'k_line_sweep_qpl_chain<f64,1,1>', 128, 4, 1, 0, False, False),
    ((4, 4, 128), 1): ('k_line_sweep_qpl_chain<c128,1,1>', 'k_line_sweep_qpl_chain<f64,1,1>', 128, 4, 1, 0, False, False),
    ((4, 4, 128), 2): ('k_line_sweep_qpl_chain<c128,1,1>', 'k_line_sweep_qpl_chain<f64,1,1>', 128, 4, 1, 0, False, False),
    ((4, 4, 128), 3): ('k_line_sweep_qpl<c128,4,2>', 'k_line_sweep_qpl<f64,4,2>', 4, 1, 1, 0, False, False),
    ((128, 8, 8), 1): ('k_line_sweep_qpl<c128,4,2>', 'k_line_sweep_qpl<f64,4,2>', 16, 1, 1, 0, False, False),
    ((128, 8, 8), 2): ('k_line_sweep_qpl<c128,1,1>', 'k_line_sweep_qpl<f64,1,1>', 256, 2, 1, 0, False, False),
    ((128, 8, 8), 3): ('k_line_sweep_qpl<c128,1,1>', 'k_line_sweep_qpl<f64,1,1>', 256, 2, 1, 0, False, False),
    ((40, 4, 6), 1): ('k_line_sweep_qpl<c128,2,2>', 'k_line_sweep_qpl<f64,2,2>', 6, 1, 1, 0, False, False),
    ((40, 4, 6), 2): ('k_line_sweep_qpl_chain<c128,1,1>', 'k_line_sweep_qpl_chain<f64,1,1>', 60, 4, 1, 0, False, False),
    ((40, 4, 6), 3): ('k_line_sweep_qpl<c128,1,1>', 'k_line_sweep_qpl<f64,1,1>', 40, 2, 1, 0, False, False),
    ((6, 40, 8), 1): ('k_line_sweep_qpl<c128,1,1>', 'k_line_sweep_qpl<f64,1,1>', 80, 2, 1, 0, False, False),
    ((6, 40, 8), 2): ('k_line_sweep_qpl<c128,2,2>', 'k_line_sweep_qpl<f64,2,2>', 12, 1, 1, 0, False, False),
    ((6, 40, 8), 3): ('k_line_sweep_qpl<c128,1,1>', 'k_line_sweep_qpl<f64,1,1>', 60, 2, 1, 0, False, False),
    ((12, 4, 4), 1): ('k_line_sweep_qpl<c128,1,1>', 'k_line_sweep_qpl<f64,1,1>', 4, 1, 1, 0, False, False),
    ((12, 4, 4), 2): ('k_line_sweep_qpl_chain<c128,1,1>', 'k_line_sweep_qpl_chain<f64,1,1>', 12, 4, 1, 0, False, False),
    ((12, 4, 4), 3): ('k_line_sweep_qpl_chain<c128,1,1>', 'k_line_sweep_qpl_chain<f64,1,1>', 12, 4, 1, 0, False, False),
}


def test_kernel_selection_is_unchanged(lib):
    assert len(PARENT_PLANS) == 3 * len(SHAPES)
    for (shape, direction), want in PARENT_PLANS.items():
        for dtype, name in ((np.complex128, want[0]), (np.float64, want[1])):
            got = lib.sweep_plan(shape, direction, dtype=dtype, cu_count=CUS)
            assert (got["kernel"], got["lines_per_colour"], got["lines_per_wave"], got["rounds"], got["factor_kind"], got["split"],
                    got["big_offsets"]) == (name,) + tuple(want[2:]), (shape, direction, got)
