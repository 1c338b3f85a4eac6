"""GPU: the products of the row store at the geometry of a production store -- emg3d_rows_gram (k_rows_gram, k_rows_gram_reduce),
emg3d_rows_matvec, emg3d_rows_rmatvec, emg3d_rows_colsumsq, emg3d_rows_project.  Stores are filled from the host; the references
are numpy.  tests/test_gpu_rows.py stops at 700 x (3 S + 7): there the slab length is S, the Gram matrix is one launch, and no
clamped load meets a value that is not finite.  Every test here first asserts FROM THE PLAN that its shape has the property it is
there for, so that another ROWS_SLAB_MIN, ROWS_SLABS_MAX or scratch size fails it instead of emptying it.

a. Exact integers (rows, v, y from -8 .. 8, cm and s from 1 .. 4: every partial sum is an integer far below 2^53, so any order of
   summation gives the same float64) at slabs that have grown: 255 slabs of S + 16 with a last slab of 33 columns, 256 slabs with a
   ragged last one, 128^3 columns (slab 8192), and two row blocks (an off-diagonal job) at a grown slab.
b. Exact integers across a launch boundary: 136 jobs of which a launch holds 128.
c. Random floats at a grown slab against np.longdouble within gamma_{n_cols + 2} |R| |cm| |R|^T; rmatvec bit for bit its loop.
d. Nested stores: G of 17 rows is G[:17, :17] of a store of 129 rows that begins with them, bit for bit.
e. A NaN or Inf in one element costs G its row and column, matvec its row, colsumsq and rmatvec its column, and nothing else.
f. project with 17 k-steps (one live row in the last) and three blocks of output rows, the last through the 32-row kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _em():
    import emg3d_amd as em
    return em


def _plan(n_rows, n_cols):
    return _em()._lib.rows_gram_plan(n_rows, n_cols)


def _geometry(n_rows, n_cols):
    """The plan, its last slab's columns, and one printed line of it."""
    p = _plan(n_rows, n_cols)
    last = n_cols - (p["nslab"] - 1) * p["slab"]
    print(f"plan {n_rows} x {n_cols}: slab {p['slab']}, nslab {p['nslab']}, last slab {last} columns, {p['nblocks']} row blocks, "
          f"{p['njobs']} jobs, jobs_per_launch {p['jobs_per_launch']}, launches {p['launches']}")
    return p, last


def _fill(R):
    store = _em().solver.DeviceRows(*R.shape)
    for i, row in enumerate(R):
        store.set_row(i, row)
    return store


def _same(got, want, what):
    """Equal element for element; the first few bad indices otherwise."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _gamma(n):
    return n * U / (1 - n * U)


# ---- a. exact integers at long slabs ------------------------------------------------------------------------------------------
SLABS_MAX = 256         # ROWS_SLABS_MAX (the plan exports no name for it; the asserts on nslab below hold the shapes to it)


def _long_shapes():
    S, k = _plan(1, 1)["slab"], _plan(1, 1)["kstep"]
    return {"17 x 256S+1": (17, SLABS_MAX * S + 1), "17 x 256(S+16)-5": (17, SLABS_MAX * (S + k) - 5), "17 x 128^3": (17, 128 ** 3),
            "129 x 256S+1": (129, SLABS_MAX * S + 1)}


_INT = {}


def _int_data(n_rows, n_cols):
    """One draw per n_cols, of the most rows any shape takes of it; small integer types, cast by the caller."""
    if n_cols not in _INT:
        most = max(r for r, c in _long_shapes().values() if c == n_cols)
        rng = np.random.default_rng(2000 + n_cols % 1000)
        _INT[n_cols] = (rng.integers(-8, 9, (most, n_cols), dtype=np.int8), rng.integers(1, 5, n_cols, dtype=np.int8),
                        rng.integers(-8, 9, n_cols, dtype=np.int8), rng.integers(-8, 9, most, dtype=np.int8),
                        rng.integers(1, 5, most, dtype=np.int8))
        for a in _INT[n_cols]:
            a.setflags(write=False)
    Ri, cm, v, y, s = _INT[n_cols]
    return Ri[:n_rows], cm, v, y[:n_rows], s[:n_rows]


@pytest.mark.parametrize("shape", ["17 x 256S+1", "17 x 256(S+16)-5", "17 x 128^3", "129 x 256S+1"])
def test_exact_integers_at_long_slabs(shape):
    n_rows, n_cols = _long_shapes()[shape]
    p, last = _geometry(n_rows, n_cols)
    S, k = _plan(1, 1)["slab"], p["kstep"]
    # the property, from the plan
    assert p["slab"] > S and p["slab"] % k == 0 and p["nslab"] > 200
    if shape in ("17 x 256S+1", "129 x 256S+1"):
        assert (n_cols, p["slab"], p["nslab"], last) == (524_289, S + 16, 255, 33)
        assert last == 2 * k + 1                            # two staging steps and one tail column
    elif shape == "17 x 256(S+16)-5":
        assert (n_cols, p["slab"], p["nslab"], last) == (528_379, S + 16, 256, 2059) and last % k != 0
    else:
        assert (n_cols, p["slab"], p["nslab"], last) == (2_097_152, 8192, 256, 8192)
    if n_rows == 129:       # two row blocks: a diagonal job, an off-diagonal one, and a diagonal one of a single live row
        assert p["nblocks"] == 2 and p["njobs"] == 3
        assert [a0 != b0 for a0, a1, b0, b1 in p["jobs"]] == [False, True, False] and p["jobs"][2][:2] == (128, 129)
    else:
        assert p["njobs"] == 1
    assert p["launches"] == 1
    assert 64 * 4 * n_cols < 2 ** 53                        # |R[a][j] cm[j] R[b][j]| <= 256: every partial sum is exact

    Ri, cmi, vi, yi, si = _int_data(n_rows, n_cols)
    R, cm, v, y, s = (a.astype(np.float64) for a in (Ri, cmi, vi, yi, si))
    G, G1 = (R * cm) @ R.T, R @ R.T                         # exact in float64 whatever the order
    assert np.array_equal(G1[:3, :3], Ri[:3].astype(np.int64) @ Ri[:3].astype(np.int64).T)
    assert np.array_equal(G[:3, :3], (Ri[:3].astype(np.int64) * cmi) @ Ri[:3].astype(np.int64).T)
    sq = R * R
    with _fill(R) as store:
        got, got1 = store.gram(cm), store.gram()
        _same(got, G, (shape, "gram(cm)"))
        _same(got1, G1, (shape, "gram()"))
        _same(got, got.T, (shape, "gram(cm) symmetric"))
        _same(got1, got1.T, (shape, "gram() symmetric"))
        _same(store.matvec(v), R @ v, (shape, "matvec"))
        _same(store.rmatvec(y, cm), cm * (y @ R), (shape, "rmatvec(y, cm)"))
        _same(store.rmatvec(y), y @ R, (shape, "rmatvec(y)"))
        _same(store.colsumsq(), sq.sum(axis=0), (shape, "colsumsq()"))
        _same(store.colsumsq(s), s @ sq, (shape, "colsumsq(s)"))


# ---- b. exact integers across a launch boundary -----------------------------------------------------------------------------
def _jobs_of(bad, p):
    """The jobs that hold the elements `bad` (index pairs) of G: (job, its launch, its rows) -- the upper triangle is the mirror of
    the job that holds the lower element."""
    hi, lo = np.maximum(bad[:, 0], bad[:, 1]) // p["block"], np.minimum(bad[:, 0], bad[:, 1]) // p["block"]
    jobs = np.unique(hi * (hi + 1) // 2 + lo)
    return [(int(j), int(j) // p["jobs_per_launch"], p["jobs"][int(j)]) for j in jobs]


def test_exact_integers_across_a_launch_boundary():
    one = _plan(1, 1)
    S, block = one["slab"], one["block"]
    n_rows, n_cols = 15 * block + 5, 15 * S + 9
    p, last = _geometry(n_rows, n_cols)
    assert (n_rows, n_cols) == (1925, 30_729)
    assert (p["nslab"], p["nblocks"], p["njobs"], p["jobs_per_launch"], p["launches"]) == (16, 16, 136, 128, 2)
    assert last == 9 and p["jobs_per_launch"] * p["job_bytes"] <= p["scratch_bytes"]
    second = p["jobs"][p["jobs_per_launch"]:]               # the second launch: 8 jobs, off-diagonal and diagonal, 5 live rows
    assert len(second) == 8 and any(a0 == b0 for a0, a1, b0, b1 in second) and any(a0 != b0 for a0, a1, b0, b1 in second)
    assert all(a1 - a0 == 5 for a0, a1, b0, b1 in second)

    rng = np.random.default_rng(1925)
    R = rng.integers(-8, 9, (n_rows, n_cols), dtype=np.int8).astype(np.float64)
    cm = rng.integers(1, 5, n_cols, dtype=np.int8).astype(np.float64)
    G1 = R @ R.T
    G = (R * cm) @ R.T
    assert 64 * 4 * n_cols < 2 ** 53 and np.abs(G).max() < 2 ** 53 and np.abs(G1).max() < 2 ** 53
    with _fill(R) as store:
        for what, got, want in (("gram(cm)", store.gram(cm), G), ("gram()", store.gram(), G1)):
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"{what}: {len(bad)} bad elements, the first {bad[:8].tolist()}, in the jobs (job, launch, " \
                                  f"(a0, a1, b0, b1)) {_jobs_of(bad, p)}"
            assert np.array_equal(got, got.T), what


# ---- c, d. random floats at a grown slab; nested stores ---------------------------------------------------------------------
_FLT = {}


def _float_data():
    """17 rows of 256 S + 1 columns with row scales 10^U(-3, 3), a signed cm, v and y; and the Gram matrices of their store, computed
    once and left unchanged."""
    if not _FLT:
        S = _plan(1, 1)["slab"]
        n_rows, n_cols = 17, SLABS_MAX * S + 1
        rng = np.random.default_rng(771)
        R = rng.standard_normal((n_rows, n_cols)) * 10 ** rng.uniform(-3, 3, (n_rows, 1))
        cm = rng.uniform(0.1, 10., n_cols) * rng.choice([-1., 1.], n_cols, p=[0.1, 0.9])
        v, y = rng.standard_normal(n_cols), rng.standard_normal(n_rows)
        with _fill(R) as store:
            G, G1, mv = store.gram(cm), store.gram(), store.matvec(v)
            again = (store.gram(cm), store.gram(), store.matvec(v))
            rm, rm1 = store.rmatvec(y, cm), store.rmatvec(y)
        for a in (R, cm, v, y, G, G1, mv, rm, rm1) + again:
            a.setflags(write=False)
        _FLT.update(R=R, cm=cm, v=v, y=y, G=G, G1=G1, mv=mv, again=again, rm=rm, rm1=rm1)
    return _FLT


def _rmatvec_loop(R, y, cm=None):
    acc = np.zeros(R.shape[1])
    for i in range(R.shape[0]):
        acc = acc + y[i] * R[i]
    return acc if cm is None else cm * acc


def test_random_floats_at_a_grown_slab():
    S = _plan(1, 1)["slab"]
    p, last = _geometry(17, SLABS_MAX * S + 1)
    assert p["slab"] == S + 16 and p["nslab"] == 255 and last == 33
    d = _float_data()
    R, cm, v, y = d["R"], d["cm"], d["v"], d["y"]
    n_cols = R.shape[1]
    Rl = R.astype(np.longdouble)
    for what, got, exact, bound in (("gram(cm)", d["G"], (Rl * cm) @ Rl.T, (np.abs(R) * np.abs(cm)) @ np.abs(R).T),
                                    ("gram()", d["G1"], Rl @ Rl.T, np.abs(R) @ np.abs(R).T),
                                    ("matvec", d["mv"], Rl @ v.astype(np.longdouble), np.abs(R) @ np.abs(v))):
        ratio = np.abs(got - exact) / (_gamma(n_cols + 2) * bound)
        print(f"17 x {n_cols}: {what}, largest error / bound {float(ratio.max()):.3e}")
        assert np.all(ratio <= 1.0), (what, float(ratio.max()))
    _same(d["rm"], _rmatvec_loop(R, y, cm), "rmatvec(y, cm) is the ascending loop")
    _same(d["rm1"], _rmatvec_loop(R, y), "rmatvec(y) is the ascending loop")
    _same(d["G"], d["G"].T, "gram(cm) symmetric")
    _same(d["G1"], d["G1"].T, "gram() symmetric")
    for first, second in zip((d["G"], d["G1"], d["mv"]), d["again"]):           # the same bits at every call
        assert first.tobytes() == second.tobytes()


def test_nested_stores():
    """The first 17 rows of a store of 129 give the G of a store of those 17: the summation order of an element follows from n_cols
    alone, and cm rides on the row of the smaller index in both.  The 112 rows behind them are live (shifted, scaled copies)."""
    d = _float_data()
    R, cm, v = d["R"], d["cm"], d["v"]
    n_cols = R.shape[1]
    p = _plan(129, n_cols)
    assert p["slab"] == _plan(17, n_cols)["slab"] and p["nblocks"] == 2 and p["njobs"] == 3
    with _em().solver.DeviceRows(129, n_cols) as store:
        for i in range(129):
            store.set_row(i, R[i] if i < 17 else np.roll(R[i % 17], i) * (1.0 + i / 128.0))
        G, G1, mv = store.gram(cm), store.gram(), store.matvec(v)
    assert np.all(np.isfinite(G)) and np.all(G1[17:, 17:].diagonal() > 0)
    _same(G1[:17, :17], d["G1"], "gram() of the first 17 rows")
    _same(G[:17, :17], d["G"], "gram(cm) of the first 17 rows")
    _same(mv[:17], d["mv"], "matvec of the first 17 rows")
    _same(G, G.T, "gram(cm) symmetric")


# ---- e. a poisoned row stays in its row -------------------------------------------------------------------------------------
_CLEAN = {}


def _clean(n_rows):
    """Random rows of S + 1 columns and every product of their store, computed once per n_rows."""
    if n_rows not in _CLEAN:
        S = _plan(1, 1)["slab"]
        rng = np.random.default_rng(50 + n_rows)
        R = rng.standard_normal((n_rows, S + 1)) * 10 ** rng.uniform(-2, 2, (n_rows, 1))
        cm = rng.uniform(0.1, 10., S + 1) * rng.choice([-1., 1.], S + 1, p=[0.1, 0.9])
        v, y = rng.standard_normal(S + 1), rng.standard_normal(n_rows)
        with _fill(R) as store:
            out = dict(R=R, cm=cm, v=v, y=y, G=store.gram(cm), G1=store.gram(), mv=store.matvec(v), cs=store.colsumsq(),
                       rm=store.rmatvec(y))
        assert all(np.all(np.isfinite(a)) and np.all(a != 0) for a in out.values())
        for a in out.values():
            a.setflags(write=False)
        _CLEAN[n_rows] = out
    return _CLEAN[n_rows]


@pytest.mark.parametrize("variant", ["nan in the last row", "inf in the last row", "nan in row 0"])
@pytest.mark.parametrize("n_rows", [17, 129, 130])
def test_a_poisoned_row_stays_in_its_row(n_rows, variant):
    """Every load of k_rows_gram past n_rows reads the LAST row and selects it to zero, every load past a slab's end reads the slab's
    last column: the poison sits where those loads read it (the last row; the last column, which is a slab of its own) and where
    they do not (row 0; a column inside).  A NaN gives NaN; +Inf gives the infinity of the one product's sign, since every other
    term of the sum is finite and none of the store is zero (a zero that was multiplied in, not selected, makes it NaN)."""
    c = _clean(n_rows)
    R, cm, v, y = c["R"], c["cm"], c["v"], c["y"]
    n_cols = R.shape[1]
    p = _plan(n_rows, n_cols)
    assert p["nslab"] == 2 and n_cols - p["slab"] == 1 and n_rows % p["tile"] != 0          # a clamped column and clamped rows
    row = 0 if variant.endswith("row 0") else n_rows - 1
    poison = np.nan if variant.startswith("nan") else np.inf
    others = np.arange(n_rows) != row
    for col in (70, n_cols - 1):
        Rp = R.copy()
        Rp[row, col] = poison
        with _fill(Rp) as store:
            got = dict(G=store.gram(cm), G1=store.gram(), mv=store.matvec(v), cs=store.colsumsq(), rm=store.rmatvec(y))
        for name, w in (("G", cm[col]), ("G1", 1.0)):
            G = got[name]
            where = (n_rows, variant, col, name)
            # everywhere else: the bits of the store without the poison
            _same(G[np.ix_(others, others)], c[name][np.ix_(others, others)], where + ("off the poisoned row and column",))
            if np.isnan(poison):
                assert np.all(np.isnan(G[row, :])) and np.all(np.isnan(G[:, row])), where
            else:
                want = np.inf * np.sign(w * R[:, col])
                want[row] = np.inf * np.sign(w)
                _same(G[row, :], want, where + ("the poisoned row",))
                _same(G[:, row], want, where + ("the poisoned column",))
        where = (n_rows, variant, col)
        _same(got["mv"][others], c["mv"][others], where + ("matvec off the poisoned row",))
        assert np.isnan(got["mv"][row]) if np.isnan(poison) else got["mv"][row] == np.inf * np.sign(v[col]), where
        keep = np.arange(n_cols) != col
        for name in ("cs", "rm"):
            _same(got[name][keep], c[name][keep], where + (name, "off the poisoned column"))
            assert not np.isfinite(got[name][col]), where + (name,)


# ---- f. project past one block of output rows and sixteen k-steps -----------------------------------------------------------
def test_project_three_passes_and_a_single_row_in_the_last_step():
    em = _em()
    one = em._lib.rows_project_plan(1, 1, 1)
    block, cols, kstep = one["block"], one["cols"], one["kstep"]
    n_rows, m, n_cols = 16 * kstep + 1, 2 * block + 1, 2 * cols + 7
    p = em._lib.rows_project_plan(n_rows, m, n_cols)
    assert (n_rows, m, n_cols) == (257, 513, 135)
    assert -(-n_rows // kstep) == 17 and n_rows % kstep == 1 and p["passes"] == 3 and p["last_rows"] == 32 and p["panels"] == 3
    rng = np.random.default_rng(257)
    Ri, Mi = rng.integers(-8, 9, (n_rows, n_cols)), rng.integers(-4, 5, (m, n_rows))
    assert 8 * 4 * n_rows < 2 ** 53
    R = Ri.astype(np.float64)
    with _fill(R) as store:
        with store.project(Mi.astype(np.float64)) as out:
            assert (out.n_rows, out.n_cols) == (m, n_cols)
            got = np.array([out.get_row(i) for i in range(m)])
        _same(got, Mi @ Ri, "project equals the int64 product")
        _same(np.array([store.get_row(i) for i in range(n_rows)]), R, "the source is unchanged")
