#!/usr/bin/env python3
"""Batch verification against N single verifications, in one process with one resident context, on one MI355X.

Files: the s_max = 8 synthetic circuit of tools/synth_circuit.py through bin/trusted-setup and bin/preprocess, eight distinct proofs from
the resident prover (item k of a batch is proof k mod 8: a verification does not depend on the circuit size beyond l_free, and identical
proofs are not merged by the batch — only the records of the reference string and of a shared preprocess are).  For N in {1, 8, 64, 512}:
  single       N calls of tkmk_prover_verify, the only way before the batch entries existed;
  host/device  tkmk_prover_verify_batch by either route, all items honest, and with ONE false item (an evaluation of proof.json flipped)
               in the middle of the batch;
each with the report's own split of seconds (parse, membership, fold, pairings) and its number of pairing products.
Writes profiles/verify_batch.json (or --out PATH) and prints one JSON line.  --sizes 1,8 restricts N; --repeat K takes the best of K."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tokamak-zk-evm_amd")
sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tools")]
os.environ.setdefault("TKMK_HOST_THREADS", "16")


def arg(name, default):
    for k, a in enumerate(sys.argv[1:]):
        if a == name:
            return sys.argv[k + 2]
        if a.startswith(name + "="):
            return a.split("=", 1)[1]
    return default


def main():
    import random
    import synth_circuit
    import tkmk
    from tkmk import proofio, service, verify
    sizes = [int(v) for v in arg("--sizes", "1,8,64,512").split(",")]
    repeat = int(arg("--repeat", "2"))
    out_path = arg("--out", os.path.join(ROOT, "profiles", "verify_batch.json"))
    tkmk.set_device(0)
    tmp = tempfile.mkdtemp(prefix="verify_batch_bench_")
    inst = synth_circuit.build(tmp, random.Random(91), s_max=8, n_gate_kinds=2, used_placements=8, bit_fraction=0.4)
    crs, pre = os.path.join(tmp, "crs"), os.path.join(tmp, "pre")
    os.makedirs(crs), os.makedirs(pre)
    env = {k: v for k, v in os.environ.items() if k not in ("TKMK_FR_ROOT_GENERATOR", "TKMK_SUBCIRCUIT_LIBRARY")}
    for cmd in ([os.path.join(PKG, "bin", "trusted-setup"), "--fixed-tau", "--subcircuit-library", inst["qap"], "--output", crs],
                [os.path.join(PKG, "bin", "preprocess"), "--crs", crs, "--synthesizer-stat", inst["synth"], "--output", pre, "--subcircuit-library", inst["qap"]]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        if r.returncode != 0:
            raise SystemExit("%s failed: %s" % (cmd[0], r.stderr[-2000:]))
    synth = inst["synth"]
    result = {"circuit": {k: inst["setup_params"][k] for k in ("n", "s_max", "l", "l_D", "l_free")}, "host_threads": int(os.environ["TKMK_HOST_THREADS"]),
              "repeat": repeat, "sizes": {}}
    with service.Prover(inst["qap"], crs) as ctx:
        proofs = []
        for k in range(8):
            d = os.path.join(tmp, "proof%d" % k)
            os.makedirs(d)
            ctx.prove(synth, d, want_json=False)
            proofs.append(d)
        doc = json.load(open(os.path.join(proofs[0], "proof.json")))
        h = doc["proof_entries_part2"][-4]                                              # R_eval
        doc["proof_entries_part2"][-4] = h[:-1] + ("0" if h[-1] != "0" else "1")
        bad = os.path.join(tmp, "bad")
        os.makedirs(bad)
        proofio.write_json(os.path.join(bad, "proof.json"), doc)
        verify.verify_batch_with(ctx, [(synth, pre, proofs[0])], route="device")        # first touch of the device route (arenas, code objects)

        def best(fn, times=repeat):
            runs = []
            for _ in range(times):
                t = time.perf_counter()
                rep = fn()
                runs.append((time.perf_counter() - t, rep))
            walls.append(sorted(round(r[0], 6) for r in runs))
            return min(runs, key=lambda r: r[0])

        walls = []                                                                      # every repeat's wall time of the last best() calls

        for n in sizes:
            row = {}
            honest = [(synth, pre, proofs[k % 8]) for k in range(n)]
            one_bad = list(honest)
            one_bad[n // 2] = (synth, pre, bad)

            # the N single calls are timed once above 64 items (0.1 s each)
            wall, verdicts = best(lambda: [verify.prover_verify(ctx, *it)[0] for it in honest], repeat if n <= 64 else 1)
            assert all(verdicts)
            row["single"] = {"wall_s": round(wall, 6), "per_proof_s": round(wall / n, 6)}
            for route in ("host", "device"):
                for name, items, want in (("honest", honest, [True] * n), ("one_bad", one_bad, [k != n // 2 for k in range(n)])):
                    wall, (each, rep) = best(lambda: verify.verify_batch_with(ctx, items, route=route))
                    assert each == want and rep["route"] == route, (n, route, name)
                    row["%s_%s" % (route, name)] = {"wall_s": round(wall, 6), "per_proof_s": round(wall / n, 6), "products": rep["products"],
                                                    "seconds": rep["seconds"], "speedup_vs_single": round(row["single"]["wall_s"] / wall, 2),
                                                    "repeats_wall_s": walls[-1],        # sorted: the spread between the best two is the run's noise
                                                    "segmented_jobs": rep.get("segmented_jobs", 0), "pipeline_jobs": rep.get("pipeline_jobs", 0)}
            result["sizes"][str(n)] = row
            print("N = %d: %s" % (n, json.dumps(row)), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(result, open(out_path, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
