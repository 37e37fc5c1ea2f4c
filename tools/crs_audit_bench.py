"""Times the CRS audit with the table checks (tkmk.verify.crs_audit(..., circuit=True)) on the two shapes DESIGN.md section 8 reports:
the production shape (s_max = 256, 166 placements) and BASELINE.json configs[3] (s_max = 1024), on the synthetic circuits and fixed-tau
reference strings tools/prove_bench.py stages.  Prints one JSON document: per shape the report's `seconds` (the audit that existed) and
`table_seconds` (the table checks) of every run, side by side.

  python tools/crs_audit_bench.py [--runs 3] [--out FILE]

--locate times the locate pass (crs_audit(..., circuit=True, locate=True)) instead: per shape the honest file with and without it (nothing
extra launches, so the two are within the run-to-run spread), then the same file with ONE record in the middle of xy_powers, and then of
the eta table, overwritten by its neighbour (a valid point in the wrong place; the file is patched in place and restored), each audited
without and with the pass: the difference is what locating costs, beside its findings and its count of pairing products.
--parent-lib FILE adds the same audits through a libtkmk_prover.so built from the parent commit (tkmk_crs_audit_circuit_files).

  python tools/crs_audit_bench.py --locate [--runs 2] [--parent-lib FILE] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import shutil
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tokamak-zk-evm_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = (("production_2p20", 256, 166), ("configs3_2p22", 1024, None))


def _section_offset(path, section):
    """byte offset and length of a section of a TKCRS001 payload (tkmk/crs.py)"""
    from tkmk import crs as crsmod
    with open(path, "rb") as f:
        head = f.read(12 + 4 * crsmod.SECTION_COUNT)
    assert head[:8] == crsmod.MAGIC
    lens = struct.unpack("<%dI" % crsmod.SECTION_COUNT, head[12:])
    k = crsmod.SECTION_NAMES.index(section)
    return len(head) + sum(lens[:k]), lens[k]


class Neighbour:
    """with Neighbour(path, section, index): record `index` of the section holds a copy of record index + 1"""

    def __init__(self, path, section, index):
        self.path, (off, n) = path, _section_offset(path, section)
        assert 96 * (index + 2) <= n
        self.at = off + 96 * index

    def __enter__(self):
        with open(self.path, "r+b") as f:
            f.seek(self.at)
            self.was, nxt = f.read(96), f.read(96)
            assert self.was != nxt and any(self.was) and any(nxt)
            f.seek(self.at)
            f.write(nxt)
        return self

    def __exit__(self, *exc):
        with open(self.path, "r+b") as f:
            f.seek(self.at)
            f.write(self.was)


def _parent_audit(lib, qap, crs):
    ok, doc = ctypes.c_int(-1), ctypes.c_void_p()
    code = lib.tkmk_crs_audit_circuit_files(os.fsencode(qap), os.fsencode(crs), ctypes.byref(ok), ctypes.byref(doc))
    if code != 0:
        raise RuntimeError("the parent library's audit failed: %s" % lib.tkmk_prover_last_error().decode())
    rep = json.loads(ctypes.string_at(doc.value).decode())
    lib.tkmk_prover_free_string(doc)
    return ok.value == 1, rep


def _timed(call):
    t = time.perf_counter()
    ok, rep = call()
    return ok, rep, round(time.perf_counter() - t, 3)


def locate_shape(verify, files, runs, parent):
    sp = files["setup_params"]
    s_max, m_i = sp["s_max"], sp["l_D"] - sp["l"]
    rs_x, rs_y = max(2 * sp["n"], 2 * m_i), 2 * s_max
    path = os.path.join(files["crs"], "combined_sigma.tkcrs")
    cases = [("honest", None, None),
             ("xy_powers_middle", "xy_powers", (rs_x // 2) * rs_y + rs_y // 2),
             ("eta_middle", "eta_inv_li_o_inter_alpha4_kj", (m_i // 2) * s_max + s_max // 2)]
    out = {"workload": files["workload"], "setup_params": sp, "extents": {"rs_x": rs_x, "rs_y": rs_y, "m_i": m_i, "s_max": s_max}, "cases": {}}
    for name, section, index in cases:
        entry = {"section": section, "index": index, "runs": []}
        tamper = Neighbour(path, section, index) if section else None
        if tamper:
            tamper.__enter__()
        try:
            for k in range(runs):
                run = {}
                ok0, rep0, run["wall_without"] = _timed(lambda: verify.crs_audit(files["qap"], files["crs"], circuit=True))
                ok1, rep1, run["wall_with"] = _timed(lambda: verify.crs_audit(files["qap"], files["crs"], circuit=True, locate=True))
                if ok0 != (section is None) or ok1 != ok0:
                    raise RuntimeError("%s: unexpected verdicts %r %r: %s" % (name, ok0, ok1, rep1["reason"]))
                run["seconds_without"], run["seconds_with"] = rep0["seconds"], rep1["seconds"]
                run["table_seconds_without"], run["table_seconds_with"] = rep0["table_seconds"], rep1["table_seconds"]
                run["locate_seconds"], run["locate_products"] = rep1["locate_seconds"], rep1["locate_products"]
                if parent is not None:
                    okp, repp, run["wall_parent"] = _timed(lambda: _parent_audit(parent, files["qap"], files["crs"]))
                    if okp != ok0 or repp["reason"] != rep0["reason"]:
                        raise RuntimeError("%s: the parent library disagrees with this one without the pass" % name)
                    run["seconds_parent"], run["table_seconds_parent"] = repp["seconds"], repp["table_seconds"]
                entry["runs"].append(run)
                print(name, "run", k, json.dumps(run), flush=True)
            entry["located"] = json.loads(json.dumps(rep1["located"]).replace(files["tmp"], "<tmp>"))     # the staging directory's name says nothing
            if section:
                found = [f for f in rep1["located"] if f["section"] == section]
                if not found or any(f["index"] != index for f in found):
                    raise RuntimeError("%s: located %r, not %s[%d]" % (name, rep1["located"], section, index))
        finally:
            if tamper:
                tamper.__exit__()
        out["cases"][name] = entry
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--locate", action="store_true", help="time the locate pass on tampered files instead")
    ap.add_argument("--parent-lib", default=None, help="with --locate: a libtkmk_prover.so of the parent commit to audit the same files with")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    args = ap.parse_args()
    import tkmk
    from tkmk import verify
    import prove_bench
    tkmk.set_device(0)
    parent = None
    if args.parent_lib:
        tkmk.lib()                                  # libtkmk_hip.so first: the parent library links against it
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.tkmk_prover_last_error.restype = ctypes.c_char_p
        parent.tkmk_prover_free_string.argtypes = [ctypes.c_void_p]
        parent.tkmk_crs_audit_circuit_files.argtypes = [ctypes.c_char_p] * 2 + [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p)]
    what = ("tkmk_crs_audit_files_ex with TKMK_CRS_AUDIT_LOCATE beside the audit without it" if args.locate else "tkmk_crs_audit_circuit_files")
    doc = {"what": what + " on synthetic circuits with fixed-tau reference strings; seconds per run", "shapes": {}}
    for name, s_max, placements in SHAPES:
        if name not in args.shapes.split(","):
            continue
        print("staging", name, flush=True)
        files = prove_bench.stage_files(s_max=s_max, placements=placements)
        try:
            if args.locate:
                doc["shapes"][name] = locate_shape(verify, files, args.runs, parent)
                continue
            runs = []
            for k in range(args.runs):
                t = time.perf_counter()
                ok, rep = verify.crs_audit(files["qap"], files["crs"], circuit=True)
                wall = time.perf_counter() - t
                if not ok:
                    raise RuntimeError("the honest reference string failed its audit: " + rep["reason"])
                runs.append({"wall": round(wall, 3), "seconds": rep["seconds"], "table_seconds": rep["table_seconds"]})
                print(name, "run", k, json.dumps(runs[-1]), flush=True)
            sp = files["setup_params"]
            doc["shapes"][name] = {"workload": files["workload"], "setup_params": sp,
                                   "points": {s["name"]: s["points"] for s in rep["sections"]},
                                   "tables": rep["tables"], "runs": runs}
        finally:
            shutil.rmtree(files["tmp"], ignore_errors=True)
            tkmk.release_scratch()
    text = json.dumps(doc, indent=1)
    if args.out:
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
