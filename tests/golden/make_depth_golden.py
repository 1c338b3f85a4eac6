"""
Generate tests/golden/depth.npz by IMPORTING the reference (emg3d v0.17.0) at run time, exactly as make_golden.py does
(`_import_reference`; nothing of the reference is written into this repository: the fixture holds inputs, records and results
only).

Cycle parity at depth: the reference's own `solver.solve` on grids whose hierarchy is up to seven levels deep, three cycles
each (maxit=3, tol=1e-30), with the residual norm after EVERY smoothing call of every level at full precision.  The reference
computes these norms for its verb=5 log and hands them to `solver._print_gs_info(it, level, cycmax, grid, norm)`, which rounds
them to four digits; that function is wrapped here for the duration of a solve (verb=5, log=-1) and its arguments are kept.
The first call of a solve is the "initial error" line, not a smoothing call, and is dropped; the kind of a call (coarsest level
/ pre- / post-smoothing) is read off the log line that the same call produced.

The cases and their problem (grid widths, tri-axial resistivities and mu_r drawn from default_rng(sum(vnC))) are those of
tests/_depth.py (CASES, problem); per case TAG the file holds

  TAG_vnC, TAG_freq, TAG_src, TAG_kw           the inputs: the problem is rebuilt from them (tests/_depth.py::problem)
  TAG_check                                    sums of the widths, of rho and of mu_r: the rebuilt problem is the same one
  TAG_records (n, 8) int                       per smoothing call: cycle, level, it, cycmax, kind, nx, ny, nz
  TAG_norms (n,)                               the residual norm of that level after the call
  TAG_error_at_cycle (4,)                      source norm and the three end-of-cycle norms
  TAG_efield                                   the final field (T cases only)
  TAG_oracle_dev (n,)                          |oracle (lexicographic order) - reference| per record: the spread between two
  TAG_oracle_dev_cycle (4,)                    implementations of the same arithmetic (tests/_depth.py::check_norms), and the
                                               same for error_at_cycle
  TAG_nrec_F                                   W cases: the number of records of the reference's F-cycle run of the case

The generator asserts that the oracle's trace has the reference's structure, and -- W must be distinguishable from F -- that
the reference's W and F runs of every W case make a different number of smoothing calls.

The archive is written with fixed time stamps: a second run reproduces the file byte for byte (the script says so when the
file exists).

Run:  python tests/golden/make_depth_golden.py     (about 5 minutes: the reference runs as pure Python, 10-50 s per solve)
"""
import io
import os
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE), ROOT]
from make_golden import _import_reference  # noqa: E402
import _depth  # noqa: E402

KINDS = ("coarsest level", "pre-smoothing", "post-smoothing")


def reference_run(emg3d, grid, model, sfield, **kw):
    """(records, norms, error_at_cycle, field) of the reference's solve."""
    from emg3d import solver
    calls = []
    orig = solver._print_gs_info

    def keep(it, level, cycmax, grid, norm):
        calls.append((int(it), int(level), int(cycmax), tuple(int(n) for n in grid.vnC), float(norm)))
        return orig(it, level, cycmax, grid, norm)
    solver._print_gs_info = keep
    try:
        e, info = solver.solve(grid, model, sfield, verb=5, log=-1, maxit=_depth.MAXIT, tol=_depth.TOL, return_info=True, **kw)
    finally:
        solver._print_gs_info = orig
    kinds = [k for line in info['log'].split('\n') for k, name in enumerate(KINDS) if line.rstrip().endswith(name)]
    calls = calls[1:]           # (the first is "initial error")
    assert len(kinds) == len(calls), (len(kinds), len(calls))
    records, norms = _depth.split_records([(it, lv, cm, kind, vnC, norm) for (it, lv, cm, vnC, norm), kind in zip(calls, kinds)])
    return records, norms, np.array(info['error_at_cycle']), np.array(e.field if hasattr(e, 'field') else e)


def save_fixed(path, arrays):
    """np.savez_compressed with fixed time stamps in the archive."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())


def main(tags):
    emg3d = _import_reference()
    from emg3d import models
    from oracle import oracle
    oracle.build()
    out = {}
    for tag in tags:
        vnC, freq, kw = _depth.CASES[tag]
        t0 = time.perf_counter()
        grid, model, sfield = _depth.problem(emg3d, vnC, freq)
        records, norms, errs, field = reference_run(emg3d, grid, model, sfield, **kw)
        t1 = time.perf_counter()
        omesh, omodel = _depth.oracle_problem(oracle, vnC, models.VolumeModel(grid, model, sfield))
        orec, onorms, oerrs, _ = _depth.oracle_run(oracle, omesh, omodel, np.array(sfield.field), **kw)
        _depth.assert_same_records(orec, records, f"{tag}: oracle against reference")
        h, _, rho, mu_r = _depth.problem_arrays(vnC)
        out.update({f'{tag}_vnC': np.array(vnC), f'{tag}_freq': np.array(freq), f'{tag}_src': np.array(_depth.SRC),
                    f'{tag}_kw': np.array(repr(kw)), f'{tag}_check': _depth.checksum(h, rho, mu_r),
                    f'{tag}_records': np.array([r[:5] + r[5] for r in records], dtype=np.int64), f'{tag}_norms': norms,
                    f'{tag}_error_at_cycle': errs, f'{tag}_oracle_dev': np.abs(onorms - norms),
                    f'{tag}_oracle_dev_cycle': np.abs(oerrs - errs)})
        if tag in _depth.WITH_FIELD:
            out[f'{tag}_efield'] = field
        msg = (f"{tag:4s} {vnC} {kw['cycle']}: {len(records)} records, levels 0...{max(r[1] for r in records)}, "
               f"{len({r[5] for r in records})} level shapes, reference {t1 - t0:.0f} s, "
               f"oracle dev max {np.abs(onorms - norms).max() / errs[0]:.1e} ||s||")
        if kw['cycle'] == 'W':
            nF = len(reference_run(emg3d, grid, model, sfield, **dict(kw, cycle='F'))[0])
            assert nF != len(records), f"{tag}: the reference's W and F runs both make {nF} smoothing calls"
            out[f'{tag}_nrec_F'] = np.array(nF)
            msg += f", F run {nF} records"
        print(msg, flush=True)
    out['cases'] = np.array(list(tags))
    if list(tags) != list(_depth.CASES):
        print("(subset of the cases: nothing written)")
        return
    path = os.path.join(HERE, 'depth.npz')
    old = open(path, 'rb').read() if os.path.exists(path) else None
    save_fixed(path, out)
    same = "" if old is None else (", byte for byte the file that was there" if old == open(path, 'rb').read() else ", DIFFERS from the file that was there")
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays{same}")


if __name__ == "__main__":
    main(sys.argv[1:] or list(_depth.CASES))
