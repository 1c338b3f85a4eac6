"""GPU: the batched contract (include/emg3d_hip.h: emg3d_mg_set_batch / select / set_mask) per kernel family.

Every system of a batch gets bit for bit the result of a handle of its own, a frozen system keeps its field bit for bit, whichever
kernel a level selects.  Whether a line-sweep kernel honours that is decided inside the kernel: each family folds the system into
blockIdx.x through EMG_SWEEP_WG (csrc/common.hpp) together with the XCD-aware line map, and applies the system's offset and the mask in
its own prologue, helper waves, LDS staging and write-back.  tests/test_gpu_batch.py checks whole cycles, which reach whatever kernels
they happen to select; here every entry of tests/_hard_cases.py SWEEP_CASES (the 25 settings of tests/test_gpu_accuracy.py), the point
smoother and the two residual kernels run by name with three systems of independent fields in one handle:

* singles: one handle, one system, the three field pairs one after the other -- two sweeps each, field and residual kept;
* batch: set_batch(3), mask [1, 0, 1], two sweeps: systems 0 and 2 are the singles' fields, system 1 its start field; mask [0, 1, 0],
  two sweeps: system 1 is its single's field, 0 and 2 unchanged; mask [1, 1, 1]: every residual is its single's;
* the kernel by name on the batched handle, and the launch log where the case says whether the passes of a call are fused;
* independent ground, so that a fault both handles share cannot hide: every batched system against the oracle's smoother in x87
  extended precision with the bound of the accuracy tests, err(hip_b) <= 10 * max(err(reference_f64_b), 16 * 2^-53), and on the benign
  generator within 1e-10 of the float64 oracle (the tolerance of tests/test_gpu_kernels.py::_sweeps_against_oracle).

The runs are the narrow ones of the accuracy tests on both generators -- at most 8 line blocks per system, so a block's place inside
an XCD's share, j_ of EMG_SWEEP_WG, is always 0 -- and `hc.wide_runs`: the same lines, 36 x 36 of them (benign generator), where every
family launches more line blocks than there are XCDs (tests/test_accuracy_plan.py holds the kernels and the line counts on the CPU).
test_sixty_four_systems runs two of the wide runs at the widest batch a handle takes, every third system frozen.

What the module sees, tried once on a scratch build: the mask of EMG_SWEEP_WG read at (b_ + 1) % n_ fails the frozen-system
assertions of every case but `tpl` and the point smoother (which take the system from blockIdx.y through EMG_BATCH), narrow and
wide; j_ dropped from the XCD line map fails every wide run that uses the map (all but `tpl` and the three fused cases, whose one
launch takes the slab from j_ without the map) and no narrow run; j_ dropped there too fails the fused cases at every run.

Every run prints `[batch] family shape direction dtype generator system err(ref) err(hip) ratio`; a bit-for-bit failure names the
family, the run, the system and the first differing edge (component, i, j, k)."""
import numpy as np
import pytest

import _hard_cases as hc
from conftest import relerr
from test_gpu_accuracy import _handle, _set_env

pytestmark = pytest.mark.gpu
NSYS = 3
PARITY = 1e-10          # HIP float64 against the float64 oracle on well-conditioned lines


@pytest.fixture(autouse=True)
def _lab_build(lab):
    yield


@pytest.fixture(scope="module")
def orc(oracle):
    if not oracle.has_extended():
        pytest.skip("np.longdouble is not the x87 extended format (64-bit significand in 16 bytes)")
    return oracle


def _same(bad, got, want, shape, what):
    """Bit for bit, or a record with the first differing edge."""
    if not np.array_equal(got, want):
        bad.append((*what, "first differing edge (component, i, j, k)", hc.first_difference(got, want, shape)))


def _verdict(bad):
    """One failure record per line (an assertion message would abbreviate the list)."""
    if bad:
        pytest.fail("\n".join(" ".join(str(v) for v in rec) for rec in bad), pytrace=False)


def _report(bad, family, shape, direction, dtype, kind, b, e_ref, e_hip):
    ratio = e_hip / max(e_ref, hc.FLOOR)
    print(f"[batch] {family} {shape} dir {direction} {hc.tname(dtype)} {kind} system {b} err(ref) {e_ref:.2e} err(hip) {e_hip:.2e} "
          f"ratio {ratio:.2f}")
    if not e_hip <= hc.bound(e_ref):
        bad.append((family, shape, direction, kind, "system", b, "off the truth", e_ref, e_hip, ratio))


def _batched(p, dtype, ordering, nsys):
    dev = _handle(p, dtype, ordering)
    dev.set_batch(nsys)             # (zeroes the fields: every system is loaded afterwards)
    assert dev.nsys == nsys
    return dev


def _load(dev, fields):
    for b, (e0, s) in enumerate(fields):
        dev.select(b)
        dev.set_sfield(s)
        dev.set_efield(e0)


def _fields_of(dev, nsys):
    out = []
    for b in range(nsys):
        dev.select(b)
        out.append(dev.get_efield())
    return out


def _singles(p, fields, dtype, ordering, direction):
    """Each system alone on one handle of one system: (field after two sweeps, its residual)."""
    single, single_r = [], []
    with _handle(p, dtype, ordering) as dev:
        for e0, s in fields:
            dev.set_sfield(s)
            dev.set_efield(e0)
            dev.smooth(2, direction)
            single.append(dev.get_efield())
            single_r.append(dev.get_residual())
        name = dev.last_sweep_kernel()
    return single, single_r, name


def _batched_run(orc, bad, dtype, ordering, shape, direction, kind, want, fused=None, capfd=None):
    """The protocol of the module's docstring on one (shape, direction, generator); failures are appended to `bad`."""
    order = 1 if ordering == "colour" else 0
    p = hc.problem(kind, shape, direction, dtype)
    fields = [hc.system_fields(kind, shape, direction, dtype, b) for b in range(NSYS)]
    run = (want or "k_point_sweep", shape, direction, hc.tname(dtype), kind)
    single, single_r, name1 = _singles(p, fields, dtype, ordering, direction)
    for b in range(NSYS):
        assert np.isfinite(single[b]).all() and not np.array_equal(single[b], fields[b][0])
    with _batched(p, dtype, ordering, NSYS) as dev:
        _load(dev, fields)
        if capfd is not None:
            print(capfd.readouterr().out, end="")           # (drops the launch log of the single handle)
        dev.set_mask([1, 0, 1])
        dev.smooth(2, direction)
        name = dev.last_sweep_kernel()
        log = capfd.readouterr() if capfd is not None else None
        got = _fields_of(dev, NSYS)
        _same(bad, got[0], single[0], shape, (*run, "mask 101, system 0 against its single handle"))
        _same(bad, got[2], single[2], shape, (*run, "mask 101, system 2 against its single handle"))
        _same(bad, got[1], fields[1][0], shape, (*run, "mask 101, frozen system 1 against its start field"))
        dev.set_mask([0, 1, 0])
        dev.smooth(2, direction)
        log2 = capfd.readouterr() if capfd is not None else None
        got = _fields_of(dev, NSYS)
        _same(bad, got[1], single[1], shape, (*run, "mask 010, system 1 against its single handle"))
        _same(bad, got[0], single[0], shape, (*run, "mask 010, frozen system 0 unchanged"))
        _same(bad, got[2], single[2], shape, (*run, "mask 010, frozen system 2 unchanged"))
        dev.set_mask([1, 1, 1])
        for b in range(NSYS):
            dev.select(b)
            _same(bad, dev.get_residual(), single_r[b], shape, (*run, f"residual of system {b} against its single handle"))
    if log is not None:
        print(log.out, log2.out, sep="", end="")
        if fused is not None:
            for lg in (log, log2):
                assert ("fused passes" in lg.err) == fused, (shape, direction, fused, lg.err[-300:])
    assert (name.startswith(want) if want else name == "") and name == name1, (shape, direction, name, name1, want)
    for b in range(NSYS):
        ref, truth = hc.references_b(orc, kind, shape, direction, dtype, b, order)
        _report(bad, name or "k_point_sweep", shape, direction, dtype, kind, b, hc.err(ref, truth), hc.err(got[b], truth))
        if kind == "benign" and not relerr(got[b], ref) < PARITY:
            bad.append((*run, "system", b, "off the float64 oracle", relerr(got[b], ref)))


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=hc.tname)
@pytest.mark.parametrize("case", hc.SWEEP_CASES, ids=[c["name"] for c in hc.SWEEP_CASES])
def test_batched_line_sweeps(orc, lab, monkeypatch, request, case, dtype):
    fused = case["fused"]
    capfd = request.getfixturevalue("capfd") if fused is not None else None         # (the launch log is the library's stderr)
    _set_env(monkeypatch, dict(case["env"], **({"EMG3D_LOG": "1"} if fused is not None else {})))
    prev = lab.use(lab.LAB_PATH if case["library"] == "lab" else lab.LIB_PATH)
    want = case["kernel"].format(t=hc.tname(dtype))
    bad = []
    try:
        for shape, direction in case["runs"]:
            for kind in ("benign", "hard"):
                _batched_run(orc, bad, dtype, case["ordering"], shape, direction, kind, want, fused, capfd)
        for shape, direction in hc.wide_runs(case):
            _batched_run(orc, bad, dtype, case["ordering"], shape, direction, "benign", want, fused, capfd)
    finally:
        lab.use(prev)
    _verdict(bad)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=hc.tname)
@pytest.mark.parametrize("shape,ordering", hc.POINT_CASES)
def test_batched_point_smoother(orc, monkeypatch, shape, ordering, dtype):
    _set_env(monkeypatch, {})
    bad = []
    for kind in ("benign", "hard"):
        _batched_run(orc, bad, dtype, ordering, shape, 0, kind, None)
    _verdict(bad)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=hc.tname)
@pytest.mark.parametrize("kernel,env", hc.RESIDUAL_CASES, ids=["k_residual", "k_residual_zm"])
@pytest.mark.parametrize("shape", hc.RESIDUAL_SHAPES)
def test_batched_residual(orc, monkeypatch, shape, kernel, env, dtype):
    """s - A e of three independent field pairs on the hard model in one handle: each bit for bit its single handle's, its norm too,
    and within the bound of the extended amat_x (the comparison value is the float64 oracle's amat_x error)."""
    _set_env(monkeypatch, env)
    p = hc.problem("hard", shape, 0, dtype)
    fields = [hc.system_fields("hard", shape, 0, dtype, b) for b in range(NSYS)]
    want = kernel.format(t=hc.tname(dtype))
    single, norms = [], []
    with _handle(p, dtype, "colour") as dev:
        for e0, s in fields:
            dev.set_sfield(s)
            dev.set_efield(e0)
            norms.append(dev.residual_norm())           # (the same kernel in its norm-only mode, <T,2...>)
            single.append(dev.get_residual())
        assert dev.last_residual_kernel() == want, dev.last_residual_kernel()
    bad = []
    with _batched(p, dtype, "colour", NSYS) as dev:
        _load(dev, fields)
        rn = dev.residual_norm()
        assert dev.last_residual_kernel() == want.replace(",1", ",2", 1), dev.last_residual_kernel()
        got = []
        for b in range(NSYS):
            dev.select(b)
            got.append(dev.get_residual())
        assert dev.last_residual_kernel() == want, dev.last_residual_kernel()
    for b in range(NSYS):
        assert np.isfinite(got[b]).all() and np.abs(got[b]).max() > 0
        _same(bad, got[b], single[b], shape, (want, shape, hc.tname(dtype), f"residual of system {b} against its single handle"))
        if rn[b] != norms[b]:
            bad.append((want, shape, "norm of system", b, rn[b], norms[b]))
        key = ("residual_b", shape, np.dtype(dtype).char, b)
        if key not in hc._cache:
            pb = hc.system_problem("hard", shape, 0, dtype, b)
            hc._cache[key] = (hc._frozen(hc.amat_x(orc, pb, pb['e0'])), hc._frozen(hc.amat_x(orc, pb, pb['e0'], ext=True)))
        ref, truth = hc._cache[key]
        _report(bad, want, shape, 0, dtype, "hard", b, hc.err(ref, truth), hc.err(got[b], truth))
    _verdict(bad)


SIXTY_FOUR = [("qpl11", ((12, 36, 36), 1)), ("thm38_zkeep", ((36, 36, 16), 3))]


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=hc.tname)
@pytest.mark.parametrize("family,run", SIXTY_FOUR, ids=[f for f, _ in SIXTY_FOUR])
def test_sixty_four_systems(oracle, lab, monkeypatch, family, run, dtype):
    """The widest batch a handle takes on two wide runs, every third system frozen: the live ones within 1e-10 of the float64 oracle,
    the frozen ones their start fields, systems 0, 31 (frozen) and 63 bit for bit a single handle's result resp. the start field."""
    case = next(c for c in hc.SWEEP_CASES if c["name"] == family)
    shape, direction = run
    assert run in hc.wide_runs(case)
    nsys = 64
    _set_env(monkeypatch, case["env"])
    prev = lab.use(lab.LAB_PATH if case["library"] == "lab" else lab.LIB_PATH)
    want = case["kernel"].format(t=hc.tname(dtype)).split(",")[0]
    p = hc.problem("benign", shape, direction, dtype)
    fields = [hc.system_fields("benign", shape, direction, dtype, b) for b in range(nsys)]
    live = [b % 3 != 1 for b in range(nsys)]
    bad = []
    try:
        single = {}
        with _handle(p, dtype, "colour") as dev:
            for b in (0, 63):
                dev.set_sfield(fields[b][1])
                dev.set_efield(fields[b][0])
                dev.smooth(2, direction)
                single[b] = dev.get_efield()
        with _batched(p, dtype, "colour", nsys) as dev:
            _load(dev, fields)
            dev.set_mask([int(v) for v in live])
            dev.smooth(2, direction)
            name = dev.last_sweep_kernel()
            got = _fields_of(dev, nsys)
        plan = lab.sweep_plan(shape, direction, dtype=dtype, nsys=nsys)["kernel"]
    finally:
        lab.use(prev)
    # (the family of the case; the planner may give 64 systems other lines per wave than one system: 12 instead of 8 for the
    # two-sided kernel at 256 compute units -- the single handle's result holds bit for bit all the same)
    assert name.startswith(want) and name == plan, (name, want, plan)
    assert not live[31] and live[0] and live[63]
    worst = 0.
    for b in range(nsys):
        what = (name, shape, direction, hc.tname(dtype), "system", b)
        if not live[b]:
            _same(bad, got[b], fields[b][0], shape, (*what, "frozen, against its start field"))
            continue
        if b in single:
            _same(bad, got[b], single[b], shape, (*what, "against its single handle"))
        d = relerr(got[b], hc.reference_b(oracle, "benign", shape, direction, dtype, b, 1))
        worst = max(worst, d)
        if not d < PARITY:
            bad.append((*what, "off the float64 oracle", d))
    print(f"[batch64] {name} {shape} dir {direction} {hc.tname(dtype)} live {sum(live)} of {nsys}, worst against the float64 oracle {worst:.2e}")
    _verdict(bad)
