"""Times the witness check (tkmk.verify.witness_check, TKMK_PROVER_CHECK_WITNESS) on the two shapes DESIGN.md section 8 reports: the
production shape (s_max = 256, 166 placements) and BASELINE.json configs[3] (s_max = 1024), on the synthetic circuits and fixed-tau
reference strings tools/prove_bench.py stages.  Per shape:
  stand_alone   the report's `seconds` of tkmk_witness_check_files (no reference string) and of tkmk_prover_check_witness, per run
  knob          init_s / total_s of resident proofs with TKMK_PROVER_CHECK_WITNESS=1 and unset, ALTERNATING in one process
  knob_off      (--parent-tree DIR: a built checkout of the parent commit) the knob-off proofs in child processes, one context each, the
                parent's tree and this one alternating on the same files: the knob-off time must not move, and the margin is the spread the
                parent shows against itself over its repeated runs, which is written next to the result
  sharded       (--sharded G, instead of the three above) G virtual ranks over the loopback transport on this one GPU
                (tkmk.dist.loopback_comms): per rank the `seconds` of the collective check (tkmk_prover_check_witness_sharded), the bytes the
                copy section's all-gather hands every rank (G x the longest per-rank source list x 32, from permutation.json), and the
                sharded proof with the knob set and unset, alternating — the unset proof is the unchecked sharded proof as it was before
                the knob reached sharded contexts.  The ranks take turns on one device: these are not multi-GPU figures.
Prints one JSON document.

  python tools/witness_check_bench.py [--runs 5] [--rounds 2] [--parent-tree DIR] [--sharded G] [--out FILE]
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "TKMK_PROVER_CHECK_WITNESS"


def _paths(tree):
    for p in (tree, os.path.join(tree, "tokamak-zk-evm_amd"), os.path.join(tree, "tools")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _proofs(prover, files, runs, warmup=1):
    out = []
    for k in range(warmup + runs):
        _, tm = prover.prove(files["synth"], os.path.join(files["tmp"], "out"), want_json=False)
        if k >= warmup:
            out.append({"init_s": round(tm["init_s"], 5), "total_s": round(tm["total_s"], 5)})
    return out


def child(args):
    """one context of the library of --tree on staged files, knob unset: `runs` proofs -> one JSON line"""
    _paths(args.tree)
    os.environ.pop(KNOB, None)
    import tkmk
    from tkmk import service
    tkmk.set_device(0)
    files = json.load(open(args.child))
    with service.Prover(files["qap"], files["crs"]) as p:
        print(json.dumps({"tree": args.tree, "runs": _proofs(p, files, args.runs)}), flush=True)


def _median(runs, key):
    return round(statistics.median(r[key] for r in runs), 5)


def gathered_bytes(synth_dir, s_max, world):
    """what tkmk_comm_all_gather_dev hands every rank in the copy section: entry e's source value is packed by rank Y mod G, every
    rank's list is padded to the longest (host/tkmk_witness_check.hpp) -> (bytes per rank, entries, longest list)"""
    last = {}
    for e in json.load(open(os.path.join(synth_dir, "permutation.json"))):       # the last writer of a cell wins
        last[int(e["row"]) * s_max + int(e["col"])] = int(e["Y"])
    count = [0] * world
    for y in last.values():
        count[y % world] += 1
    return world * max(count + [0]) * 32, len(last), max(count + [0])


def sharded_shape(files, world, runs):
    """-> the `sharded` record of one shape: G loopback ranks of the production library on the staged files"""
    from tkmk import dist, service, verify
    comms = dist.loopback_comms(world)
    provers = dist.run_ranks(comms, lambda c: service.Prover(files["qap"], files["crs"], comm=c))
    by_rank = {p.comm.rank: p for p in provers}
    out_dir = os.path.join(files["tmp"], "out_sharded")
    try:
        nbytes, entries, longest = gathered_bytes(files["synth"], files["setup_params"]["s_max"], world)
        rec = {"world": world, "transport": "loopback (one GPU, the ranks take turns)", "entries": entries, "longest_source_list": longest,
               "gathered_bytes_per_rank": nbytes, "check_seconds_per_rank": []}

        def check(c):
            ok, rep = verify.witness_check(None, files["synth"], prover=by_rank[c.rank], collective=True)
            if not ok:
                raise RuntimeError("the honest witness failed its check: " + rep["reason"])
            return rep["seconds"]

        def prove(c):
            _, tm = by_rank[c.rank].prove(files["synth"], out_dir if c.rank == 0 else None, want_json=False)
            return {"init_s": round(tm["init_s"], 5), "total_s": round(tm["total_s"], 5)}
        for k in range(runs):
            rec["check_seconds_per_rank"].append(dist.run_ranks(comms, check))
            print("sharded check run", k, json.dumps(rec["check_seconds_per_rank"][-1][0]), flush=True)
        dist.run_ranks(comms, prove)                                             # warm-up
        on, off = [], []
        for k in range(runs):
            os.environ[KNOB] = "1"
            on.append(dist.run_ranks(comms, prove))
            os.environ.pop(KNOB)
            off.append(dist.run_ranks(comms, prove))
        rank0 = lambda runs_, key: round(statistics.median(r[0][key] for r in runs_), 5)      # noqa: E731
        rec["knob"] = {"on_per_rank": on, "off_per_rank": off, "median_init_s_rank0": {"on": rank0(on, "init_s"), "off": rank0(off, "init_s")},
                       "median_total_s_rank0": {"on": rank0(on, "total_s"), "off": rank0(off, "total_s")}}
        print("sharded knob", json.dumps({k: rec["knob"][k] for k in ("median_init_s_rank0", "median_total_s_rank0")}), flush=True)
        return rec
    finally:
        for p in provers:
            p.close()
        for c in comms:
            c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="with --parent-tree: child processes per tree")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--sharded", type=int, default=0, metavar="G", help="G loopback ranks: the collective check and the sharded knob only")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    _paths(ROOT)
    import tkmk
    from tkmk import service, verify
    import prove_bench
    tkmk.set_device(0)
    os.environ.pop(KNOB, None)
    doc = {"what": "the witness check on synthetic circuits with fixed-tau reference strings; seconds", "shapes": {}}
    for name, s_max, placements in (("production_2p20", 256, 166), ("configs3_2p22", 1024, None)):
        print("staging", name, flush=True)
        files = prove_bench.stage_files(s_max=s_max, placements=placements)
        try:
            shape = {"setup_params": files["setup_params"], "placements": files["placements"]}
            if args.sharded:
                shape["sharded"] = sharded_shape(files, args.sharded, args.runs)
                tkmk.release_scratch()
                doc["shapes"][name] = shape
                continue
            alone = []
            for k in range(args.runs):
                ok, rep = verify.witness_check(files["qap"], files["synth"])
                if not ok:
                    raise RuntimeError("the honest witness failed its check: " + rep["reason"])
                alone.append(rep["seconds"])
                print(name, "stand-alone run", k, json.dumps(rep["seconds"]), flush=True)
            shape["stand_alone_files"] = alone
            shape["entries"] = rep["copy"]["entries"]
            shape["public_wires"] = rep["public"]["wires"]
            with service.Prover(files["qap"], files["crs"]) as p:
                resident = []
                for k in range(args.runs):
                    ok, rep = verify.witness_check(None, files["synth"], prover=p)
                    assert ok
                    resident.append(rep["seconds"])
                shape["stand_alone_resident"] = resident
                on, off = [], []
                p.prove(files["synth"], os.path.join(files["tmp"], "out"), want_json=False)      # warm-up
                for k in range(args.runs):
                    os.environ[KNOB] = "1"
                    on += _proofs(p, files, 1, warmup=0)
                    os.environ.pop(KNOB)
                    off += _proofs(p, files, 1, warmup=0)
                shape["knob"] = {"on": on, "off": off, "median_init_s": {"on": _median(on, "init_s"), "off": _median(off, "init_s")},
                                 "median_total_s": {"on": _median(on, "total_s"), "off": _median(off, "total_s")}}
                print(name, "knob", json.dumps({k: shape["knob"][k] for k in ("median_init_s", "median_total_s")}), flush=True)
            tkmk.release_scratch()
            if args.parent_tree:
                manifest = os.path.join(files["tmp"], "files.json")
                json.dump({k: files[k] for k in ("tmp", "qap", "synth", "crs")}, open(manifest, "w"))
                per = {"parent": [], "this": []}
                for r in range(args.rounds):
                    for who, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
                        cmd = [sys.executable, os.path.join(ROOT, "tools", "witness_check_bench.py"), "--child", manifest, "--tree", tree, "--runs", str(args.runs)]
                        t = time.perf_counter()
                        line = subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=600).stdout.strip().splitlines()[-1]
                        runs = json.loads(line)["runs"]
                        per[who].append({"median_init_s": _median(runs, "init_s"), "median_total_s": _median(runs, "total_s"), "runs": runs,
                                         "process_s": round(time.perf_counter() - t, 2)})
                        print(name, "knob off,", who, "process", r, per[who][-1]["median_init_s"], per[who][-1]["median_total_s"], flush=True)
                summary = {}
                for key in ("median_init_s", "median_total_s"):
                    pa, th = [x[key] for x in per["parent"]], [x[key] for x in per["this"]]
                    summary[key] = {"parent": pa, "this": th, "parent_spread": round(max(pa) - min(pa), 5),
                                    "this_minus_parent": round(statistics.mean(th) - statistics.mean(pa), 5),
                                    "inside_parent_spread": abs(statistics.mean(th) - statistics.mean(pa)) <= max(pa) - min(pa)}
                shape["knob_off"] = {"processes": per, "summary": summary}
            doc["shapes"][name] = shape
        finally:
            shutil.rmtree(files["tmp"], ignore_errors=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
