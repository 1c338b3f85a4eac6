"""CPU-only: the level-0 multigrid loop of solver.py (``_batched_multigrid``; ``multigrid`` runs it for one system) against a
stand-in for the device handle that records every call and answers the residual norms from a script
(tests/golden/make_level0_traces.py: ``FakeHandle``, the cases, ``run_case``).  tests/golden/level0_traces.json holds, per case,
the calls, the printed text, the logs and the ``info_dict`` recorded when ``multigrid`` and ``_batched_multigrid`` still were two
statements of the loop; every case is replayed through the same entry points and must come out equal."""
import contextlib
import importlib.util
import io
import json
import os

import pytest

from conftest import GOLDEN
from emg3d_amd import solver

_spec = importlib.util.spec_from_file_location("make_level0_traces", os.path.join(GOLDEN, "make_level0_traces.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def recorded():
    with open(rec.PATH) as fh:
        return json.load(fh)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(c["name"] for c in rec.CASES)


@pytest.mark.parametrize("case", rec.CASES, ids=[c["name"] for c in rec.CASES])
def test_replay_equals_the_record(case, recorded):
    got = json.loads(json.dumps(rec.run_case(case), sort_keys=True))
    want = recorded[case["name"]]
    assert got["calls"] == want["calls"]
    assert got["stdout"] == want["stdout"]
    assert got == want


def _without_trace(calls):
    """The call list without what only the verb = 5 trace of a single solve asks for: ``set_trace``, ``get_trace`` and the norm
    after the initial smoothing."""
    out = []
    for c in calls:
        if c[0] in rec.TRACE_CALLS or (c[0] == "residual_norm" and out and out[-1][0] == "smooth"):
            continue
        out.append(c)
    return out


@pytest.mark.parametrize("case", [c for c in rec.CASES if c["kind"] == "one" or (c["kind"] == "pre" and c.get("nsys", 1) == 1)],
                         ids=lambda c: c["name"])
def test_single_loop_is_the_batched_loop_with_one_system(case):
    """``multigrid(dev=)`` asks of the handle what ``_batched_multigrid(dev, [var], [1])`` asks (apart from the trace of verb = 5; no
    field is downloaded here) and leaves the same parameters; below verb = 5 it prints the same.  A failing preconditioner is a
    raised ``_ConvergenceError`` there and ``failed == [0]`` here."""
    if case["kind"] == "pre":
        case = dict(case, opts=dict(case["opts"], sslsolver="bicgstab"))
    single, batched = rec.fake_for(case), rec.fake_for(case)
    var_s, var_b = rec.loop_var(case), rec.loop_var(case)
    out_s, out_b = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out_s):
        raised = rec.run_multigrid(case, single, var_s)
    with contextlib.redirect_stdout(out_b):
        failed, on_device = solver._batched_multigrid(batched, [var_b], [1])
    assert failed == ([0] if raised else []) and list(on_device) == [1]
    assert not any(c[0] == "set_mask" for c in single.calls + batched.calls)
    assert _without_trace(single.calls) == _without_trace(batched.calls)
    assert not any(c[0] in rec.TRACE_CALLS for c in batched.calls)
    state_s, state_b = rec.var_state(var_s), rec.var_state(var_b)
    if case["opts"]["verb"] < 5:
        assert rec.mask(out_s.getvalue()) == rec.mask(out_b.getvalue())
    else:
        del state_s["log_message"], state_b["log_message"]
    assert state_s == state_b
    assert type(var_s.l2) is float
