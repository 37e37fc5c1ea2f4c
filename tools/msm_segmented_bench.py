#!/usr/bin/env python3
"""tkmk_msm_segmented against tkmk_msm_multi_ex on few-term jobs, in one process on one MI355X.

Every shape is ten (or more) jobs over index lists into one resident table of plain records, as the batch verifier's fold issues them:
  fold       the one-item fold: jobs of 1, 1, 1, 1, 1, 1, 3, 5, 22 and 24 terms, with 128-bit scalars (bitsize 128) and with 255-bit ones;
  equal      ten equal jobs of 2^k terms, k = 0 .. 12; the crossover is the largest 2^k up to which the segmented entry is never slower;
  finish     the two tails on one-term jobs, 10 .. 1000 of them: k_msm_segmented_finish alone (one lane per job: 4 x windows doublings,
             windows additions, one inversion — the single-lane latency), forced through the asynchronous form, beside the synchronous
             call, which finishes a small call on the host.
Wall times are host clocks around the synchronous calls, the two entries alternating round by round after two warm-up rounds (median and
minimum of --reps rounds); the kernels' own times come from a separate pass with the event profiler on (tkmk_profile_get "msm.segmented",
"msm.segmented_finish").  Both entries' results are compared byte for byte at every shape before anything is timed.
Writes profiles/msm_segmented.json (or --out PATH) and prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tokamak-zk-evm_amd")]

TABLE = 4096
FOLD_SIZES = [1, 1, 1, 1, 1, 1, 3, 5, 22, 24]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--max-log", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_segmented.json"))
    args = ap.parse_args()
    import numpy as np
    import oracle
    import tkmk
    tkmk.set_device(0)
    rnd = np.random.default_rng(17)
    d_table = tkmk.DeviceBuffer.from_host(np.asarray(oracle.g1_random_bases(23, TABLE)))
    full = np.asarray(oracle.fr_random(24, 10 << args.max_log)).reshape(-1, 32).copy()
    half = full.copy()
    half[:, 16:] = 0                                                   # 128-bit scalars
    d_full, d_half = tkmk.DeviceBuffer.from_host(full.reshape(-1)), tkmk.DeviceBuffer.from_host(half.reshape(-1))

    def make_jobs(sizes, d_scalars):
        idx = rnd.integers(0, TABLE, max(sum(sizes), 1), dtype=np.uint32)
        d_idx = tkmk.DeviceBuffer.from_host(idx.view(np.uint8))
        jobs, at = [], 0
        for n in sizes:
            jobs.append(dict(scalars=d_scalars, scalar_offset=32 * at, bases=d_table, n=n, base_index=d_idx, index_offset=4 * at, table_len=TABLE))
            at += n
        return jobs

    def wall(fns):
        """{name: fn} -> {name: {"median_ms", "min_ms"}}, the entries alternating inside every round"""
        runs = {k: [] for k in fns}
        for r in range(args.reps + 2):
            for k, fn in fns.items():
                t = time.perf_counter()
                fn()
                if r >= 2:
                    runs[k].append((time.perf_counter() - t) * 1e3)
        return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)} for k, v in runs.items()}

    def kernels(fn):
        """the two kernels' own times per call, event-bracketed, in a pass of their own"""
        tkmk.profile_enable(True)
        tkmk.profile_reset()
        for _ in range(args.reps):
            fn()
        out = {}
        for name in ("msm.segmented", "msm.segmented_finish"):
            ms, cnt = tkmk.profile_get(name)
            out[name + "_ms"] = round(ms / max(cnt, 1), 4)
        tkmk.profile_enable(False)
        return out

    def shape(sizes, d_scalars, bitsize):
        jobs = make_jobs(sizes, d_scalars)
        seg = lambda: tkmk.msm_segmented(jobs, bitsize=bitsize)                                  # noqa: E731
        multi = lambda: tkmk.msm_multi_ex(jobs, bitsize=bitsize)                                 # noqa: E731
        # a one-term job of msm_multi_ex goes through a kernel that does not read bitsize: compare where both mask (or nothing is masked)
        keep = [k for k, n in enumerate(sizes) if n != 1 or not bitsize]
        a, b = seg(), multi()
        assert all((a[144 * k:144 * (k + 1)] == b[144 * k:144 * (k + 1)]).all() for k in keep), "the two entries disagree"
        row = {"jobs": len(sizes), "terms": sum(sizes), "bitsize": bitsize or 255}
        row.update(wall({"segmented": seg, "multi_ex": multi}))
        row["kernels"] = kernels(seg)
        return row

    result = {"reps": args.reps, "table_records": TABLE, "fold": {}, "equal": {}, "finish": {}}
    result["fold"]["scalars_128"] = shape(FOLD_SIZES, d_half, 128)
    result["fold"]["scalars_255"] = shape(FOLD_SIZES, d_full, 0)
    print("fold:", json.dumps(result["fold"]), file=sys.stderr, flush=True)
    crossover, unbroken = 0, True
    for k in range(args.max_log + 1):
        row = shape([1 << k] * 10, d_full, 0)
        result["equal"][str(1 << k)] = row
        unbroken = unbroken and row["segmented"]["median_ms"] <= row["multi_ex"]["median_ms"]
        if unbroken:
            crossover = 1 << k
        print("10 x %d terms: %s" % (1 << k, json.dumps(row)), file=sys.stderr, flush=True)
    result["crossover_terms"] = crossover
    # the two tails: a synchronous call of few jobs finishes on the host, a large or an asynchronous one in k_msm_segmented_finish;
    # the asynchronous form (device results, then the status query, which waits) forces the kernel at any size
    for n_jobs in (10, 32, 64, 128, 256, 1000):
        jobs = make_jobs([1] * n_jobs, d_full)

        def device_tail():
            tkmk.msm_segmented(jobs, results_on_device=True, is_async=True)
            tkmk.msm_segmented_status()

        row = wall({"library_choice": lambda: tkmk.msm_segmented(jobs), "device_tail": device_tail})
        k = kernels(device_tail)
        result["finish"][str(n_jobs)] = {"finish_kernel_ms": k["msm.segmented_finish_ms"], "main_kernel_ms": k["msm.segmented_ms"], "call_wall": row}
        print("%d one-term jobs: %s" % (n_jobs, json.dumps(result["finish"][str(n_jobs)])), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
