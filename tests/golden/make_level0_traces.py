"""
Generate tests/golden/level0_traces.json: what the level-0 multigrid loop of emg3d_amd/solver.py asks of a device handle, and
what it prints and returns, for scripted residual norms.  No GPU and no built library are needed: a stand-in for ``DeviceMG``
(``FakeHandle``) records every call with its arguments and answers ``residual_norm`` / ``cycle`` / ``sfield_norm`` from the
script; it goes in through the public entry points (``solve(handle=)``, ``solve_sources(handle=)``, ``multigrid(dev=)``,
``_batched_multigrid``).

The fixture records the behaviour of the code it was generated from; tests/test_level0_loop_host.py replays every case
(``CASES`` / ``run_case`` of this module) and demands equality.  Regenerate it only together with a deliberate change of the loop.

Per case: the call list, the captured stdout, ``log_message`` and the state of every ``MGParameters``, every ``info_dict`` without
``time`` and ``runtime_at_cycle``; clock readings are masked (``mask``), NaN and infinities are strings.

Run:  python tests/golden/make_level0_traces.py
"""
import contextlib
import io
import itertools
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from emg3d_amd import fields, meshes, solver  # noqa: E402

PATH = os.path.join(HERE, "level0_traces.json")
CLOCK = re.compile(r"\d+:\d\d:\d\d")            # [hh:mm:ss] stamps and h:mm:ss runtimes
TRACE_CALLS = ("set_trace", "get_trace")        # (plus the residual_norm after the initial smoothing: see the test)


def mask(text):
    return CLOCK.sub("h:mm:ss", text)


def enc(x):
    """JSON form of an argument or a result: numbers as they are (NaN / inf as strings), small arrays as lists, anything
    nE-sized or opaque as a tag."""
    if x is None or isinstance(x, (bool, str)):
        return x
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x) if np.isfinite(x) else str(float(x))
    if isinstance(x, solver.MGParameters):
        return "<var>"
    if hasattr(x, "field"):
        return "<field>"
    if isinstance(x, np.ndarray):
        return [enc(v) for v in x.tolist()] if x.size <= 64 else f"<array {x.shape} {x.dtype}>"
    if isinstance(x, (list, tuple)):
        return [enc(v) for v in x]
    if isinstance(x, dict):
        return {k: enc(v) for k, v in x.items()}
    return f"<{type(x).__name__}>"


class FakeHandle:
    """Stand-in for ``DeviceMG``: ``calls`` holds ``[name, args..., {kwargs}]`` of every call; ``residual_norm`` / ``cycle`` /
    ``sfield_norm`` answer from their scripts (a float for one system, an array otherwise), everything else trivially."""
    SFIELD, EFIELD = -1, -2
    RECORDED = ("set_params", "set_sfield", "set_source", "set_efield", "select", "set_mask", "begin", "smooth", "set_trace",
                "close")

    def __init__(self, nsys=1, cycle=(), residual=(), sfield=(1.0,), nE=3 * 16 * 17 * 17):
        self.nsys, self.nE, self.device = nsys, nE, 0
        self.dtype = np.dtype(np.complex128)
        self.calls = []
        self._script = {"cycle": list(cycle), "residual_norm": list(residual), "sfield_norm": list(sfield)}

    def _rec(self, name, args, kwargs):
        self.calls.append([name] + [enc(a) for a in args] + ([enc(kwargs)] if kwargs else []))

    def __getattr__(self, name):
        if name not in self.RECORDED:
            raise AttributeError(name)
        return lambda *args, **kwargs: self._rec(name, args, kwargs)

    def _norms(self, name):
        v = self._script[name].pop(0)
        return float(v) if self.nsys == 1 else np.array(v, dtype=np.float64)

    def residual_norm(self):
        self._rec("residual_norm", (), {})
        return self._norms("residual_norm")

    def cycle(self, *args, **kwargs):
        self._rec("cycle", args, kwargs)
        return self._norms("cycle")

    def sfield_norm(self):
        self._rec("sfield_norm", (), {})
        return float(self._script["sfield_norm"].pop(0))

    def set_batch(self, n):
        self._rec("set_batch", (n,), {})
        self.nsys = int(n)

    def get_efield(self, out=None):
        self._rec("get_efield", (out,), {})
        return out

    def get_trace(self):
        self._rec("get_trace", (), {})
        return [(-1, 0, 2, 1, (16, 16, 16), 0.5), (1, 1, 2, 0, (8, 8, 8), 0.25), (-1, 0, 2, 2, (16, 16, 16), 0.125)]

    def get_receiver_response(self, rec, **kwargs):
        self._rec("get_receiver_response", (rec,), kwargs)
        return np.zeros(np.size(rec[0]), dtype=self.dtype)

    def vec_get(self, i):
        self._rec("vec_get", (i,), {})
        return np.zeros(self.nE, dtype=self.dtype)


def grid16():
    return meshes.TensorMesh([np.ones(16) * 50.0] * 3, origin=(-400.0, -400.0, -400.0))


def var_state(var):
    return {"exit_message": var.exit_message, "it": var.it, "l2": enc(var.l2), "sc_dir": enc(var.sc_dir), "lr_dir": enc(var.lr_dir),
            "error_at_cycle": enc(var.error_at_cycle), "log_message": mask(var.log_message)}


def info_state(info):
    return {k: (mask(v) if k == "log" else enc(v)) for k, v in info.items() if k not in ("time", "runtime_at_cycle")}


# --------------------------------------------------------------------------- the cases
# one system: the norm after each cycle (the initial norm is 1 = the source's norm; tol = 1e-6)
SCRIPTS = {
    "converging": [1e-1, 1e-2, 1e-4, 1e-5, 1e-7],
    "diverging": [0.5, 20.0],
    "nan": [0.5, float("nan")],
    "stagnating": [0.5, 0.4, 0.3] + [0.3] * 4,
    "maxit": [0.5, 0.4, 0.3],
}


def one_system_cases():
    out = []
    for (name, norms), nu_init, verb, rot in itertools.product(SCRIPTS.items(), (0, 2), (-1, 1, 3, 4, 5), (True, False)):
        opts = dict(nu_init=nu_init, verb=verb, semicoarsening=rot, linerelaxation=rot)
        if name == "maxit":
            opts["maxit"] = 3
        out.append({"name": f"one:{name}:nu_init={nu_init}:verb={verb}:rotation={rot}", "kind": "one", "cycle": norms, "opts": opts})
    return out


ONE = one_system_cases()
SRC = (0.0, 0.0, 0.0, 0.0, 0.0)
THREE = {"cycle": [[0.1, 0.1, 0.5], [1e-2, 1e-7, 0.4], [1e-3, 7.0, 0.4], [1e-7, 7.0, 0.4]] + [[7.0, 7.0, 0.4]] * 4}
CASES = ONE + [
    dict(ONE[[c["name"] for c in ONE].index("one:converging:nu_init=0:verb=4:rotation=True")], name="one:no-prepare-ahead",
         prepare_ahead=False),
    # one system as a preconditioner: multigrid() and _batched_multigrid() directly
    {"name": "pre:diverging", "kind": "pre", "cycle": [0.5, 20.0], "opts": dict(verb=4, semicoarsening=True, linerelaxation=True)},
    {"name": "pre:maxit", "kind": "pre", "cycle": [0.5, 0.4, 0.3], "opts": dict(verb=4, semicoarsening=True, linerelaxation=True)},
    {"name": "pre:maxit:fixed", "kind": "pre", "cycle": [0.5], "opts": dict(verb=-1, semicoarsening=False, linerelaxation=False)},
    # three systems as a preconditioner: system 1 fails in the second cycle and is frozen, the others run out of cycles
    {"name": "pre:three", "kind": "pre", "nsys": 3, "cycle": [[0.5, 0.5, 0.5], [0.4, 20.0, 0.4], [0.3, 7.0, 0.3]],
     "opts": dict(verb=4, semicoarsening=True, linerelaxation=True)},
    # multigrid() with an efield to upload and download; and on a handle of its own (solver.DeviceMG replaced)
    {"name": "multigrid:efield", "kind": "mg", "cycle": SCRIPTS["converging"], "opts": dict(verb=5, nu_init=2)},
    {"name": "multigrid:own", "kind": "mg", "own": True, "cycle": SCRIPTS["converging"], "opts": dict(verb=5)},
    {"name": "multigrid:own:fails", "kind": "mg", "own": True, "cycle": [0.5, 20.0],
     "opts": dict(verb=5, sslsolver="bicgstab", semicoarsening=True)},
] + [
    # three systems through solve_sources: system 1 converges at cycle 2, system 0 at cycle 4, system 2 stagnates
    dict(THREE, name=f"three:verb={verb}:rotation={rot}", kind="sources", sfield=[1.0, 1.0, 1.0],
         opts=dict(verb=verb, semicoarsening=rot, linerelaxation=rot))
    for verb, rot in itertools.product((-1, 1, 4, 5), (True, False))
] + [
    dict(THREE, name="three:zero-source", kind="sources", sfield=[1.0, 0.0, 1.0], opts=dict(verb=4, linerelaxation=True)),
    dict(THREE, name="three:receivers:no-download", kind="sources", sfield=[1.0, 1.0, 1.0], opts=dict(verb=1, nu_init=1),
         rec=True, download=False),
    {"name": "three:resident=2", "kind": "sources", "resident": 2, "sfield": [1.0, 1.0],
     "cycle": [[0.1, 0.1, 7.0], [1e-7, 1e-2, 7.0], [7.0, 1e-7, 7.0]], "opts": dict(verb=4, semicoarsening=True)},
    {"name": "one-of-one:sources", "kind": "sources", "nsys": 1, "sfield": [1.0], "cycle": SCRIPTS["converging"],
     "opts": dict(verb=5, nu_init=2, semicoarsening=True, linerelaxation=True)},
    # solve() extras
    {"name": "solve:efield-good", "kind": "solve", "efield": True, "residual": [1e-9], "cycle": [], "opts": dict(verb=3)},
    {"name": "solve:efield-continue", "kind": "solve", "efield": True, "residual": [0.5, 0.5], "cycle": [1e-3, 1e-7],
     "opts": dict(verb=4, return_info=True)},
    {"name": "solve:zero-source", "kind": "solve", "sfield": [0.0], "cycle": [], "opts": dict(verb=3, return_info=True)},
    {"name": "solve:no-download", "kind": "solve", "download": False, "cycle": SCRIPTS["converging"],
     "opts": dict(verb=1, return_info=True)},
    {"name": "solve:no-info", "kind": "solve", "cycle": SCRIPTS["converging"], "opts": dict(verb=2, return_info=False)},
    {"name": "solve:source-on-device", "kind": "solve", "source": (SRC, 0), "cycle": SCRIPTS["converging"],
     "opts": dict(verb=1, return_info=True)},
]


def fake_for(case):
    nsys = case.get("nsys", 3 if case["kind"] == "sources" else 1)
    ones = 1.0 if nsys == 1 else [1.0] * nsys
    residual = case.get("residual", [ones, 0.9 if nsys == 1 else [0.9] * nsys])
    return FakeHandle(nsys=nsys, cycle=case["cycle"], residual=residual, sfield=case.get("sfield", [1.0]))


def loop_var(case):
    """``MGParameters`` as ``solve`` hands them to the loop: the source's norm is 1."""
    opts = dict(cycle="F", sslsolver=False, semicoarsening=False, linerelaxation=False, vnC=(16, 16, 16))
    opts.update(case["opts"])
    var = solver.MGParameters(**opts)
    var.l2_refe = 1.0
    var.error_at_cycle[0] = 1.0
    var._dev_efield_current = True
    return var


def run_multigrid(case, fake, var, efield=None):
    """``multigrid(dev=fake)``; returns whether it raised ``_ConvergenceError``."""
    try:
        solver.multigrid(grid16(), None, None, efield, var, dev=fake)
    except solver._ConvergenceError:
        return True
    return False


def run_case(case):
    """Run one case on the code as it is; returns its record."""
    grid = grid16()
    fake = fake_for(case)
    out = {}
    kind = case["kind"]
    prepare_ahead = solver.PREPARE_AHEAD
    solver.PREPARE_AHEAD = case.get("prepare_ahead", True)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            if kind in ("one", "solve"):
                sfield = fields.SourceField(grid, freq=1.0)
                kwargs = dict(case["opts"])
                kwargs.setdefault("return_info", True)
                efield = fields.Field(grid, dtype=sfield.dtype, freq=1.0) if case.get("efield") else None
                if "source" in case:
                    kwargs["source"] = case["source"]
                res = solver.solve(grid, None, sfield, efield, handle=fake, download=case.get("download", True), **kwargs)
                got_field, info = (res if isinstance(res, tuple) else
                                   (None, res) if isinstance(res, dict) else (res, None))
                out["returned_field"] = got_field is not None
                out["infos"] = [info_state(info)] if info is not None else []
            elif kind == "sources":
                n = case.get("resident", fake.nsys)
                res = solver.solve_sources(grid, None, None if "resident" in case else [SRC] * n, 1.0, handle=fake,
                                           resident=case.get("resident"), download=case.get("download", True),
                                           rec=(np.zeros(2), np.zeros(2), np.zeros(2), 0.0, 0.0) if case.get("rec") else None,
                                           **case["opts"])
                out["n_fields"] = None if res[0] is None else len(res[0])
                out["infos"] = [info_state(i) for i in res[1]]
            elif kind == "pre":
                # the same script through both entry points, each with parameters and a handle of its own
                vars_ = [loop_var(dict(case, opts=dict(case["opts"], sslsolver="bicgstab"))) for _ in range(fake.nsys)]
                failed, on_device = solver._batched_multigrid(fake, vars_, [1] * fake.nsys)
                out["failed"], out["on_device"] = enc(failed), enc(on_device)
                out["vars"] = [var_state(v) for v in vars_]
                if fake.nsys == 1:
                    single, var = fake_for(case), loop_var(dict(case, opts=dict(case["opts"], sslsolver="bicgstab")))
                    out["multigrid_raised"] = run_multigrid(case, single, var)
                    out["multigrid_calls"] = single.calls
                    out["multigrid_var"] = var_state(var)
            elif kind == "mg":
                var = loop_var(case)
                if case.get("own"):
                    device_mg = solver.DeviceMG
                    solver.DeviceMG = lambda *a, **k: fake
                    try:
                        try:
                            solver.multigrid(grid, None, fields.SourceField(grid, freq=1.0), None, var)
                            out["multigrid_raised"] = False
                        except solver._ConvergenceError:
                            out["multigrid_raised"] = True
                    finally:
                        solver.DeviceMG = device_mg
                else:
                    var._dev_efield_current = False
                    out["multigrid_raised"] = run_multigrid(case, fake, var, fields.Field(grid, dtype=fake.dtype, freq=1.0))
                out["vars"] = [var_state(var)]
    finally:
        solver.PREPARE_AHEAD = prepare_ahead
    out["calls"] = fake.calls
    out["stdout"] = mask(buf.getvalue())
    out["left_in_script"] = {k: len(v) for k, v in fake._script.items()}
    return out


def main():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    record = {c["name"]: run_case(c) for c in CASES}
    # each script must have reached the branch it is there for
    for c in ONE:
        want = {"converging": "CONVERGED", "diverging": "DIVERGED", "nan": "DIVERGED", "stagnating": "STAGNATED",
                "maxit": "MAX. ITERATION REACHED, NOT CONVERGED"}[c["name"].split(":")[1]]
        assert record[c["name"]]["infos"][0]["exit_message"] == want, c["name"]
    with open(PATH, "w") as fh:
        fh.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'), sort_keys=True)}"
                                     for k, v in record.items()) + "\n}\n")
    print(f"wrote {PATH}: {len(record)} cases, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
