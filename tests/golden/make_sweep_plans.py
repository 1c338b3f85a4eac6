"""
Generate tests/golden/sweep_plans.json: what `emg3d_sweep_plan` (the launch selection of the line smoother,
csrc/sweep_plan.hpp) answers for a table of (library, lab variables, shape, direction, dtype, ordering, nsys, cu_count).
No GPU is needed (cu_count > 0) and nothing is allocated, so the table also holds levels of many GiB.

The fixture records the selection of the libraries it was generated from; tests/test_host_logic.py replays it against the
built libraries and demands equality of every field.  Regenerate it only together with a deliberate change of the selection.

  table     product library: edge lengths EDGES ** 3 plus EXTRA shapes, x 3 directions x f64 / c128 x colour / lex x nsys 1 / 8
            x 256 / 128 CUs, and the same with EMG3D_BATCH_TUNE=1;
            lab library (variables set in os.environ around the calls: the library reads them per call): LAB_EDGES ** 3 plus
            EXTRA for every entry of LAB_ENVS, 256 CUs.
  fixture   a sample of the table drawn with a fixed seed, small enough to read (see sample()).

Run:  python tests/golden/make_sweep_plans.py [--lib-dir DIR] [--dump FILE] [--no-fixture]
      --lib-dir   directory holding libemg3d_hip.so and libemg3d_hip_lab.so (default: emg3d_amd/ of this tree)
      --dump      also write the FULL table, one row per line (to compare two builds with `cmp`)
"""
import argparse
import ctypes
import itertools
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

EDGES = [2, 3, 4, 5, 8, 16, 17, 32, 33, 64, 65, 90, 128, 129, 136, 144, 160, 200, 256, 448, 512]
LAB_EDGES = [2, 4, 8, 16, 17, 32, 33, 64, 65, 128, 200, 256]
EXTRA = [(160, 160, 768), (640, 640, 640), (384, 384, 384), (128, 64, 64), (256, 128, 128), (128, 64, 128), (320, 32, 40),
         (64, 72, 264), (96, 160, 48), (256, 128, 64), (184, 184, 184), (224, 224, 224), (288, 288, 288)]
LAB_ENVS = [
    {"EMG3D_TWIST": "0"}, {"EMG3D_SWEEP": "tpl"}, {"EMG3D_Q_BIG": "1"}, {"EMG3D_Q": "2"}, {"EMG3D_Q": "0"}, {"EMG3D_THA": "2"},
    {"EMG3D_THA": "0"}, {"EMG3D_Q_LPW": "8"}, {"EMG3D_Q": "2", "EMG3D_Q_LPW": "2"}, {"EMG3D_TH_LPW": "4"}, {"EMG3D_TH_LPW": "12"},
    {"EMG3D_TWIST": "0", "EMG3D_LPW": "8"}, {"EMG3D_TWIST": "0", "EMG3D_LPW": "12"}, {"EMG3D_TWIST": "0", "EMG3D_LPW": "4"},
    {"EMG3D_Q_STAGES": "2"}, {"EMG3D_Q_STAGES": "3"}, {"EMG3D_QPL_CHAIN": "0"}, {"EMG3D_QPL_CHAIN": "16"}, {"EMG3D_BATCH_TUNE": "1"},
    {"EMG3D_QPL": "0"}, {"EMG3D_QPL": "5"}, {"EMG3D_SPLIT": "1"}, {"EMG3D_SPLIT": "0"}, {"EMG3D_XT": "0"}, {"EMG3D_QPL_MAX_NL": "8"},
    {"EMG3D_QPL_M2": "2"}, {"EMG3D_TW_STAGES": "2"}, {"EMG3D_SPLIT_MIN_CELLS": "1000"},
    {"EMG3D_QPL": "0", "EMG3D_Q": "2", "EMG3D_Q_MIN_LINES": "1", "EMG3D_Q_BIG": "1"},
    {"EMG3D_QPL": "0", "EMG3D_THA_MIN": "3", "EMG3D_THA_MIN_LINES": "1"},
    {"EMG3D_QPL": "0", "EMG3D_TWIST": "0", "EMG3D_Q": "0"},
]
SEED = 20240611
COLUMNS = ["nx", "ny", "nz", "direction", "dtype", "ordering", "nsys", "cu_count", "kernel", "lines_per_colour", "lines_per_wave",
           "rounds", "factor_kind", "split", "big_offsets"]


def open_lib(path):
    lib = ctypes.CDLL(path)
    i64, ci = ctypes.c_int64, ctypes.c_int
    lib.emg3d_sweep_plan.restype = ci
    lib.emg3d_sweep_plan.argtypes = [ci, i64, i64, i64, ci, ci, ci, ci, ctypes.c_char_p, ctypes.POINTER(i64)]
    return lib


def plans(lib, shapes, nsyss, cus):
    """Rows in COLUMNS order."""
    name = ctypes.create_string_buffer(64)
    info = (ctypes.c_int64 * 6)()
    rows = []
    for (nx, ny, nz), d, dt, order, nsys, cu in itertools.product(shapes, (1, 2, 3), (1, 0), (1, 0), nsyss, cus):
        st = lib.emg3d_sweep_plan(dt, nx, ny, nz, d, order, nsys, cu, name, info)
        assert st == 0, (st, nx, ny, nz, d)
        rows.append([nx, ny, nz, d, "c128" if dt else "f64", "colour" if order else "lex", nsys, cu, name.value.decode()] + list(info))
    return rows


def table(lib_dir):
    """[(library, variables, rows)]"""
    prod = open_lib(os.path.join(lib_dir, "libemg3d_hip.so"))
    lab = open_lib(os.path.join(lib_dir, "libemg3d_hip_lab.so"))
    shapes = list(itertools.product(EDGES, repeat=3)) + EXTRA
    lab_shapes = list(itertools.product(LAB_EDGES, repeat=3)) + EXTRA
    known = [k for k in os.environ if k.startswith("EMG3D_")]
    assert not known, f"unset {known} first: the libraries read them"
    out = [("prod", {}, plans(prod, shapes, (1, 8), (256, 128)))]
    for lib, tag, env, sh in [(prod, "prod", {"EMG3D_BATCH_TUNE": "1"}, lab_shapes)] + [(lab, "lab", e, lab_shapes) for e in LAB_ENVS]:
        os.environ.update(env)
        try:
            out.append((tag, env, plans(lib, sh, (1, 8), (256,))))
        finally:
            for k in env:
                del os.environ[k]
    out.append(("lab", {}, plans(lab, lab_shapes, (1, 8), (256, 128))))
    return out


def check(tab):
    """The families the fixture must hold (each seen to be selected by the libraries the fixture was first generated from)."""
    prod = {r[8] for tag, env, rows in tab if tag == "prod" and not env for r in rows}
    for tn in ("c128", "f64"):
        want = [f"k_line_sweep_qc<{tn},2,16>", f"k_line_sweep_qc<{tn},3,16>", f"k_line_sweep_qc_big<{tn},3,16>",
                f"k_line_sweep_thm<{tn},3,8>", f"k_line_sweep_thm<{tn},3,12>", f"k_line_sweep_tha<{tn},3>",
                f"k_line_sweep_qpl_chain<{tn},1,1>", f"k_line_sweep<{tn}>"] + \
               [f"k_line_sweep_qpl<{tn},{nw},{m}>" for nw, m in ((1, 1), (1, 2), (2, 1), (2, 2), (4, 2), (8, 2))]
        missing = [w for w in want if w not in prod]
        assert not missing, missing
    assert any(n.startswith("k_line_sweep_rp<c128,") for n in prod)

    def lab(env):
        return {r[8] for tag, e, rows in tab if tag == "lab" and e == env for r in rows}
    assert any(n.startswith("k_line_sweep_rp<") for n in lab({"EMG3D_TWIST": "0"}))
    assert lab({"EMG3D_SWEEP": "tpl"}) == {"k_line_sweep<c128>", "k_line_sweep<f64>"}
    assert "k_line_sweep_qc_big<c128,2,16>" in lab({"EMG3D_Q_BIG": "1"})          # 256^3
    assert "k_line_sweep_qc<c128,3,4>" in lab({"EMG3D_Q": "2"})
    assert "k_line_sweep_tha<c128,2>" in lab({"EMG3D_THA": "2"})
    assert "k_line_sweep_qc<c128,3,8>" in lab({"EMG3D_Q_LPW": "8"})
    assert "k_line_sweep_thm<c128,3,4>" in lab({"EMG3D_TH_LPW": "4"})
    assert "k_line_sweep_rp<c128,8>" in lab({"EMG3D_TWIST": "0", "EMG3D_LPW": "8"})
    assert "k_line_sweep_rp<c128,12>" in lab({"EMG3D_TWIST": "0", "EMG3D_LPW": "12"})
    assert "k_line_sweep_qc<c128,2,16>" not in lab({"EMG3D_Q_STAGES": "3"}) and "k_line_sweep_qc<c128,3,16>" not in lab({"EMG3D_Q_STAGES": "2"})
    assert not any("chain" in n for n in lab({"EMG3D_QPL_CHAIN": "0"}))
    chain4 = {tuple(r[:8]) for tag, e, rows in tab if tag == "lab" and not e for r in rows if "chain" in r[8] and r[7] == 256}
    chain16 = {tuple(r[:8]) for tag, e, rows in tab if tag == "lab" and e == {"EMG3D_QPL_CHAIN": "16"} for r in rows if "chain" in r[8]}
    assert chain4 < chain16
    for tag in ("prod", "lab"):     # EMG3D_BATCH_TUNE=1 changes names with 8 systems
        base = {tuple(r[:8]): r[8] for t, e, rows in tab if t == tag and not e for r in rows}
        tuned = [r for t, e, rows in tab if t == tag and e == {"EMG3D_BATCH_TUNE": "1"} for r in rows]
        assert any(r[6] == 8 and tuple(r[:8]) in base and base[tuple(r[:8])] != r[8] for r in tuned), tag


def sample(tab):
    """A few hundred rows that a reader can take in.  Product library: one row of every (dtype, kernel name, lines per wave, factor
    layout, split, 64-bit offsets) that occurs, plus rows until every (dtype, kernel name) is seen with every direction, ordering,
    batch size and device size it occurs with.  A group with variables set: one row per (dtype, kernel name) among the rows whose
    answer DIFFERS from the same library's answer without the variables."""
    rng = random.Random(SEED)
    base = {tag: {tuple(r[:8]): r[8:] for r in rows} for tag, env, rows in tab if not env}

    def one_per(rows, key):
        strata = {}
        for r in rows:
            strata.setdefault(key(r), []).append(r)
        return [rng.choice(strata[k]) for k in sorted(strata)]
    groups = []
    for tag, env, rows in tab:
        if env:
            changed = [r for r in rows if base[tag].get(tuple(r[:8])) != r[8:]]
            keep = one_per(changed or rows, lambda r: (r[4], r[8], r[5]))       # (no row differs: the variable is not seen in the record)
        elif tag == "lab":
            keep = one_per(rows, lambda r: (r[4], r[8]))
        else:
            keep = one_per(rows, lambda r: (r[4], r[8], r[10], r[12], r[13], r[14]))
            seen = {(r[4], r[8], c, r[c]) for r in keep for c in (3, 5, 6, 7)}
            for r in rng.sample(rows, len(rows)):
                new = {(r[4], r[8], c, r[c]) for c in (3, 5, 6, 7)} - seen
                if new:
                    keep.append(r)
                    seen |= new
        groups.append({"library": tag, "env": env, "rows": sorted(keep)})
    return {"columns": COLUMNS, "groups": groups}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-dir", default=os.path.join(ROOT, "emg3d_amd"))
    ap.add_argument("--dump")
    ap.add_argument("--no-fixture", action="store_true")
    args = ap.parse_args()
    tab = table(args.lib_dir)
    check(tab)
    n = sum(len(rows) for _, _, rows in tab)
    if args.dump:
        with open(args.dump, "w") as fh:
            for tag, env, rows in tab:
                for r in rows:
                    fh.write(json.dumps([tag, env] + r, separators=(",", ":"), sort_keys=True) + "\n")
    if not args.no_fixture:
        fix = sample(tab)
        path = os.path.join(HERE, "sweep_plans.json")
        with open(path, "w") as fh:
            fh.write('{"columns":' + json.dumps(fix["columns"], separators=(",", ":")) + ',\n"groups":[\n')
            fh.write(",\n".join('{"library":%s,"env":%s,"rows":[\n%s]}' % (json.dumps(g["library"]), json.dumps(g["env"], sort_keys=True),
                                 ",\n".join(json.dumps(r, separators=(",", ":")) for r in g["rows"])) for g in fix["groups"]))
            fh.write("\n]}\n")
        kept = sum(len(g["rows"]) for g in fix["groups"])
        print(f"wrote sweep_plans.json: {kept} of {n} rows, {os.path.getsize(path)} bytes")
    print(f"table: {n} rows")


if __name__ == "__main__":
    main()
