"""The estimator resolver (avr_range_resolve_device: key records -> K2 range records on the device) timed on the synthetic
workloads, whose K1 records are key records as they stand:

  w2_groups8   config 2 (512 slices), one group per 8 slices
  w2_one       config 2, one group of all slices
  w5_each      config 5 (1 Mi slices), one group per slice

Per shape, with events around the calls and the steps taking turns: the resolver alone, the K2 encode of the resolved records alone
(the path bench.py --kind range takes for the shape: K2p for few long slices, pack + one lane per slice else -- what a batch cost
while the host resolved the estimators), and resolver + encode in one span.  Next to the times, the bytes the resolver must move
(2 B in and 2 B out per bin in the emit pass; 2 B per bin more in each of the count and the function pass for bins of groups that
span windows; the rows' tables) and the time the HBM rate (--hbm-gbs) would take for them.  Prints one JSON line and writes it to
--out.

  python tools/range_keys_bench.py [--steps 20] [--warmup 3] [--slices2 512] [--slices5 1048576] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avrecode_ms_amd import CHUNK_BINS  # noqa: E402  (AVR_CHUNK_BINS)

WINDOW_CHUNKS, ROW_BYTES = 16, 1028 * 6


def spanning_bins(n_bins, group_first):
    """bins and rows of the groups that cross a window of WINDOW_CHUNKS chunks (the resolver's count and function passes read them)"""
    import numpy as np
    chunks = np.maximum(1, (n_bins.astype(np.int64) + CHUNK_BINS - 1) // CHUNK_BINS)
    base = np.concatenate([[0], np.cumsum(chunks)])
    bins_c = np.concatenate([[0], np.cumsum(n_bins.astype(np.int64))])
    gf = np.asarray(group_first)
    a, b = base[gf[:-1]], base[gf[1:]]
    span = (b > a) & (a // WINDOW_CHUNKS != (b - 1) // WINDOW_CHUNKS)
    bins = int((bins_c[gf[1:]] - bins_c[gf[:-1]])[span].sum())
    rows = int(((b - 1) // WINDOW_CHUNKS - a // WINDOW_CHUNKS + 1)[span].sum())
    return bins, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slices2", type=int, default=512)
    ap.add_argument("--slices5", type=int, default=1 << 20)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM rate the floor is computed with, GB/s")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    import avrecode_ms_amd as avr

    if avr.device_count() < 1:
        raise SystemExit("range_keys_bench.py needs a GPU: the resolver has no CPU path")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    shapes = [("w2_groups8", 2, args.slices2, 8), ("w2_one", 2, args.slices2, 0), ("w5_each", 5, args.slices5, 1)]
    result = {"tool": "range_keys_bench", "library_sha256": avr.library_sha256(), "steps": args.steps, "warmup": args.warmup,
              "hbm_gbs": args.hbm_gbs, "shapes": {}}
    synth = {}
    for name, workload, n, per_group in shapes:
        if (workload, n) not in synth:
            synth.clear()                                            # one workload resident at a time
            src = avr.DeviceWorkload.synth(workload, n, avr.KIND_CABAC, 0, 1000)
            synth[(workload, n)] = src._slice_major() + (src.n_bins,)
        key_flat, rec_off, n_bins = synth[(workload, n)]
        group_first = list(range(0, n, per_group)) + [n] if per_group else [0, n]
        kw = avr.DeviceWorkload.from_device_keys(key_flat, rec_off, n_bins, group_first)
        rw = kw.resolve_range()                                      # also the warm-up of the resolver and the packer
        torch.cuda.synchronize()
        assert not int((rw.status != 0).sum().item())
        chunked = n <= 32768 and kw.total_bins // n >= 8192          # the batch API's rule, and bench.py's
        L = avr.lib()
        sp = torch.cuda.current_stream().cuda_stream

        def encode():
            if chunked:
                rw.encode_chunked()
            else:
                rw.status.zero_()
                avr._check(L.avr_pack_tiles_device(0, sp, avr.KIND_RANGE, 0, rw.rec_flat.data_ptr(), rw.rec_off.data_ptr(), rw.n_bins.data_ptr(),
                                                   rw.order.data_ptr(), rw.n_slices, rw.tile_off.data_ptr(), rw.tiles.data_ptr(), rw.status.data_ptr()))
                rw.encode()

        def both():
            kw.resolve_keys()
            encode()

        steps = {"resolve": kw.resolve_keys, "encode": encode, "resolve_encode": both}
        times = {k: [] for k in steps}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(args.warmup + args.steps):
            for k in (list(steps) * 2)[i % 3:i % 3 + 3]:                      # the three take turns, the order rotating
                ev[0].record()
                steps[k]()
                ev[1].record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times[k].append(ev[0].elapsed_time(ev[1]))
        assert not int((rw.status != 0).sum().item())
        nb = n_bins.cpu().numpy()
        span_bins, span_rows = spanning_bins(nb, group_first)
        bins = int(nb.sum())
        must = 4 * bins + 2 * 2 * span_bins + span_rows * ROW_BYTES * 3 + 2 * 2052 * (len(group_first) - 1)
        ws = L.avr_range_resolve_workspace_bytes(n, len(group_first) - 1, __import__("ctypes").byref(kw._chunk_plan()["plan"]))
        r = {"workload": workload, "slices": n, "groups": len(group_first) - 1, "bins": bins, "k2_path": "k2p" if chunked else "lanes",
             "spanning_bins": span_bins, "rows": span_rows, "workspace_bytes": int(ws),
             "bytes_must_move": must, "hbm_floor_ms": must / (args.hbm_gbs * 1e6)}
        for k, v in times.items():
            r[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        r["resolve_gbs"] = must / (r["resolve_ms"]["median"] * 1e6)
        r["resolve_over_encode"] = r["resolve_ms"]["median"] / r["encode_ms"]["median"]
        result["shapes"][name] = r
        del kw, rw
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    t0 = time.time()
    main()
    print(f"range_keys_bench.py: {time.time() - t0:.1f} s", file=sys.stderr)
