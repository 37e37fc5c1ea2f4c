"""Times the CRS audit with the table checks (tkmk.verify.crs_audit(..., circuit=True)) on the two shapes DESIGN.md section 8 reports:
the production shape (s_max = 256, 166 placements) and BASELINE.json configs[3] (s_max = 1024), on the synthetic circuits and fixed-tau
reference strings tools/prove_bench.py stages.  Prints one JSON document: per shape the report's `seconds` (the audit that existed) and
`table_seconds` (the table checks) of every run, side by side.

  python tools/crs_audit_bench.py [--runs 3] [--out FILE]
"""
import argparse
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tokamak-zk-evm_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import tkmk
    from tkmk import verify
    import prove_bench
    tkmk.set_device(0)
    doc = {"what": "tkmk_crs_audit_circuit_files on synthetic circuits with fixed-tau reference strings; seconds per run", "shapes": {}}
    for name, s_max, placements in (("production_2p20", 256, 166), ("configs3_2p22", 1024, None)):
        print("staging", name, flush=True)
        files = prove_bench.stage_files(s_max=s_max, placements=placements)
        try:
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
