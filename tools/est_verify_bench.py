"""The estimator checker (avr_range_keys_verify_device: the resolved records held to the key records by the update rule) timed beside
the resolver whose output it checks (avr_range_resolve_device), on the shapes of profiles/range_keys_bench.json:

  w2_one       config 2 (512 slices), one group of all slices
  w2_groups8   config 2, one group per 8 slices (64 groups)
  w5_each      config 5 (1 Mi slices), one group per slice

Per shape, with events around the calls and the two taking turns after the warm-up: the resolver alone, the checker alone (in the
resolver's workspace, as the batch API runs it; it must find nothing).  There is no threshold: the figures are what DESIGN.md quotes.
--kernel-stats SHAPE=FILE (repeatable): a kernel_stats.csv of a kernel trace of this tool run with --shapes SHAPE; the average
duration of each k_estv_* kernel is added to that shape.  --merge FILE: a JSON object whose keys are added to the result (the
kernels' register figures, the bench.py runs of the same visit).  Prints one JSON line and writes it to --out.

  python tools/est_verify_bench.py [--steps 20] [--warmup 3] [--shapes w2_one,w2_groups8,w5_each] [--slices2 512] [--slices5 1048576]
                                   [--kernel-stats SHAPE=FILE] [--merge FILE] [--out FILE]
"""
import argparse
import csv
import ctypes
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_averages(path):
    """k_estv_* kernel -> average milliseconds, from a kernel_stats.csv"""
    out = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r"k_estv_\w+", r["Name"])
        if m:
            out[m.group(0)] = {"calls": int(r["Calls"]), "avg_ms": float(r["AverageNs"]) / 1e6}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="w2_one,w2_groups8,w5_each")
    ap.add_argument("--slices2", type=int, default=512)
    ap.add_argument("--slices5", type=int, default=1 << 20)
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="SHAPE=FILE")
    ap.add_argument("--merge", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import avrecode_ms_amd as avr

    if avr.device_count() < 1:
        raise SystemExit("est_verify_bench.py needs a GPU: the checker has no CPU path")
    torch.cuda.set_device(torch.device("cuda", 0))
    all_shapes = {"w2_one": (2, args.slices2, 0), "w2_groups8": (2, args.slices2, 8), "w5_each": (5, args.slices5, 1)}
    result = {"tool": "est_verify_bench", "library_sha256": avr.library_sha256(), "steps": args.steps, "warmup": args.warmup, "shapes": {}}
    L = avr.lib()
    synth = {}
    for name in args.shapes.split(","):
        workload, n, per_group = all_shapes[name]
        if (workload, n) not in synth:
            synth.clear()                                            # one workload resident at a time
            src = avr.DeviceWorkload.synth(workload, n, avr.KIND_CABAC, 0, 1000)
            synth[(workload, n)] = src._slice_major() + (src.n_bins,)
            del src
        key_flat, rec_off, n_bins = synth[(workload, n)]
        group_first = list(range(0, n, per_group)) + [n] if per_group else [0, n]
        kw = avr.DeviceWorkload.from_device_keys(key_flat, rec_off, n_bins, group_first)
        kw.status.zero_()
        kw.resolve_keys()
        p = kw._chunk_plan()
        p["ws_estv"], p["ws_estv_bytes"] = p["ws_est"], L.avr_range_keys_verify_workspace_bytes(n, kw.n_groups, ctypes.byref(p["plan"]))
        assert p["ws_estv_bytes"] <= p["ws_est_bytes"]                # the resolver's workspace handed on as it stands
        found = []

        def check():
            found.append(kw.verify_keys()[1])

        steps = {"resolve": kw.resolve_keys, "check": check}
        times = {k: [] for k in steps}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(args.warmup + args.steps):
            for k in ("resolve", "check"):                           # in turns: the checker reads what the resolver before it wrote
                ev[0].record()
                steps[k]()
                ev[1].record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times[k].append(ev[0].elapsed_time(ev[1]))
        assert not int((kw.status != 0).sum().item())
        assert all(int((f != -1).sum().item()) == 0 for f in found[-2:]), "the checker found something in the resolver's output"
        bins = int(n_bins.to(torch.int64).sum().item())
        r = {"workload": workload, "slices": n, "groups": len(group_first) - 1, "bins": bins,
             "workspace_bytes": int(p["ws_estv_bytes"]), "resolver_workspace_bytes": int(p["ws_est_bytes"])}
        for k, v in times.items():
            r[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        r["check_over_resolve"] = r["check_ms"]["median"] / r["resolve_ms"]["median"]
        r["check_gbs"] = 4 * bins / (r["check_ms"]["median"] * 1e6)   # 2 B of key record and 2 B of resolved record per bin, read once
        result["shapes"][name] = r
        del kw, found
    for item in args.kernel_stats:
        shape, path = item.split("=", 1)
        result["shapes"].setdefault(shape, {})["kernels"] = kernel_averages(path)
    if args.merge:
        result.update(json.load(open(args.merge)))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    t0 = time.time()
    main()
    print(f"est_verify_bench.py: {time.time() - t0:.1f} s", file=sys.stderr)
