"""One-byte key records (AVR_KIND_RANGE_KEYS8) against two-byte ones (AVR_KIND_RANGE_KEYS) on the same streams, in one visit.

The streams are the synthetic workloads' K1 records with their keys folded into 0..127 (record & 0xff): as two-byte key records and,
byte for byte the same values, as one-byte ones, at the same rec_off (multiples of 16: records for the one, bytes for the other).

  resolver   avr_range_resolve_device against avr_range_resolve8_device, the two taking turns, events around each call:
               w2_one      config 2 (512 slices), one group of all slices
               w2_groups64 config 2, 64 groups of 8 slices
               w5_each     config 5 (1 Mi slices), one group per slice
             with the workspaces both quote.  The outputs are compared once (records and est_out[:128] identical).
  batch      a RANGE_KEYS8 batch against a RANGE_KEYS batch of the same slices (--batch-slices of config 2, one group), the two taking
             turns on objects that are reused: Batch.timings()["h2d_ms"] and the wall time of submit + wait.

A few warm-ups, then medians with min and max.  Prints one JSON line and writes it to --out.

  python tools/range_keys8_bench.py [--steps 20] [--warmup 3] [--slices2 512] [--slices5 1048576] [--batch-slices 128] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def folded_streams(avr, torch, workload, n):
    """(two-byte key records, one-byte key records, rec_off, n_bins) of a synthetic workload, keys folded into 0..127"""
    src = avr.DeviceWorkload.synth(workload, n, avr.KIND_CABAC, 0, 1000)
    dev = src.n_bins.device
    nb = src.n_bins.to(torch.int64)
    rec_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((nb + 15) // 16 * 16, 0)])
    flat = torch.empty(int(rec_off[-1]) + 16, dtype=torch.int16, device=dev)
    avr._check(avr.lib().avr_synth_generate_slices_device(0, torch.cuda.current_stream().cuda_stream, ctypes.byref(src.cfg), avr.KIND_CABAC, n,
                                                          rec_off.data_ptr(), flat.data_ptr(), None))
    flat &= 0xff
    torch.cuda.synchronize()
    return flat, flat.to(torch.uint8), rec_off, src.n_bins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slices2", type=int, default=512)
    ap.add_argument("--slices5", type=int, default=1 << 20)
    ap.add_argument("--batch-slices", type=int, default=128)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    import avrecode_ms_amd as avr

    if avr.device_count() < 1:
        raise SystemExit("range_keys8_bench.py needs a GPU: the resolver has no CPU path")
    torch.cuda.set_device(0)
    L = avr.lib()
    result = {"tool": "range_keys8_bench", "library_sha256": avr.library_sha256(), "steps": args.steps, "warmup": args.warmup,
              "shapes": {}, "batch": {}}
    shapes = [("w2_one", 2, args.slices2, 0), ("w2_groups64", 2, args.slices2, max(1, args.slices2 // 64)), ("w5_each", 5, args.slices5, 1)]
    streams, batch_slices = {}, None
    for name, workload, n, per_group in shapes:
        if (workload, n) not in streams:
            streams.clear()                                          # one workload resident at a time
            streams[(workload, n)] = folded_streams(avr, torch, workload, n)
        flat16, flat8, rec_off, n_bins = streams[(workload, n)]
        if workload == 2 and batch_slices is None:                   # the batch measurement's slices, on the host
            k = min(args.batch_slices, n)
            off, nb = rec_off[:k + 1].cpu().numpy(), n_bins[:k].cpu().numpy()
            host8 = flat8[:int(off[-1])].cpu().numpy()
            batch_slices = [host8[int(off[i]):int(off[i]) + int(nb[i])] for i in range(k)]
        gf = list(range(0, n, per_group)) + [n] if per_group else [0, n]
        kw16 = avr.DeviceWorkload.from_device_keys(flat16, rec_off, n_bins, gf)
        kw8 = avr.DeviceWorkload.from_device_keys8(flat8, rec_off, n_bins, gf)
        for kw in (kw16, kw8):
            kw.rec_flat.zero_()
            kw.resolve_keys()
        torch.cuda.synchronize()
        assert not int((kw16.status != 0).sum().item()) and not int((kw8.status != 0).sum().item())
        assert torch.equal(kw16.rec_flat[:int(rec_off[-1])], kw8.rec_flat[:int(rec_off[-1])]), "the two widths resolve different records"
        assert torch.equal(kw16.est_out.view(-1, avr.EST_KEYS, 2)[:, :avr.EST_KEYS8], kw8.est_out.view(-1, avr.EST_KEYS8, 2))
        steps = {"two_byte": kw16.resolve_keys, "one_byte": kw8.resolve_keys}
        times = {k: [] for k in steps}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(args.warmup + args.steps):
            for k in (list(steps) * 2)[i % 2:i % 2 + 2]:              # the two take turns, the order alternating
                ev[0].record()
                steps[k]()
                ev[1].record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times[k].append(ev[0].elapsed_time(ev[1]))
        plan = ctypes.byref(kw8._chunk_plan()["plan"])
        r = {"workload": workload, "slices": n, "groups": len(gf) - 1, "bins": int(n_bins.to(torch.int64).sum().item()),
             "total_chunks": int(kw8._chunk_plan()["plan"].total_chunks),
             "workspace_bytes": {"two_byte": int(L.avr_range_resolve_workspace_bytes(n, len(gf) - 1, plan)),
                                 "one_byte": int(L.avr_range_resolve8_workspace_bytes(n, len(gf) - 1, plan))},
             "checker_workspace_bytes": {"two_byte": int(L.avr_range_keys_verify_workspace_bytes(n, len(gf) - 1, plan)),
                                         "one_byte": int(L.avr_range_keys8_verify_workspace_bytes(n, len(gf) - 1, plan))},
             "resolve_ms": {k: spread(v) for k, v in times.items()}}
        r["one_over_two"] = r["resolve_ms"]["one_byte"]["median"] / r["resolve_ms"]["two_byte"]["median"]
        result["shapes"][name] = r
        del kw16, kw8
    streams.clear()

    # the batch API end to end: the same slices as one group, one byte a record against two
    total = sum(len(s) for s in batch_slices)
    wide = [s.astype(np.uint16) for s in batch_slices]
    objs = {"one_byte": avr.Batch(0, len(batch_slices), total + 8), "two_byte": avr.Batch(0, len(batch_slices), total + 8)}
    times = {k: {"h2d_ms": [], "run_wall_ms": [], "resolve_pack_ms": [], "encode_ms": []} for k in objs}
    outs = {}
    for i in range(args.warmup + args.steps):
        for k in (list(objs) * 2)[i % 2:i % 2 + 2]:
            b = objs[k]
            b.reset()
            for s in (batch_slices if k == "one_byte" else wide):
                b.add_slice_range_keys8(s) if k == "one_byte" else b.add_slice_range_keys(s)
            t0 = time.perf_counter()
            b.submit()
            b.wait()
            wall = (time.perf_counter() - t0) * 1e3
            ms = b.timings()
            if i >= args.warmup:
                times[k]["h2d_ms"].append(ms["h2d_ms"]); times[k]["resolve_pack_ms"].append(ms["pack_ms"]); times[k]["encode_ms"].append(ms["encode_ms"])
                times[k]["run_wall_ms"].append(wall)
            outs[k] = [b.get(j) for j in range(len(batch_slices))]
    assert outs["one_byte"] == outs["two_byte"], "the two batches code different bytes"
    result["batch"] = {"workload": 2, "slices": len(batch_slices), "bins": total, "chunked": objs["one_byte"].run_info()["chunked"],
                       "h2d_bytes": {"one_byte": sum((len(s) + 15) // 16 * 16 for s in batch_slices),
                                     "two_byte": sum((len(s) + 7) // 8 * 16 for s in batch_slices)}}
    for k in objs:
        result["batch"][k] = {m: spread(v) for m, v in times[k].items()}
        objs[k].close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    t0 = time.time()
    main()
    print(f"range_keys8_bench.py: {time.time() - t0:.1f} s", file=sys.stderr)
