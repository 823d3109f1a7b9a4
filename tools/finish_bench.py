"""What finishing a device-resident batch on the device costs beside compacting it: avr_finish_device and avr_compact_device over the
same coded output, on two of the synthetic workloads at their full slice counts:

  w2   config 2 (512 long slices)      w5   config 5 (1 Mi short slices)

  compact       avr_compact_device: the scan over the lengths and the copy
  finish_plain  avr_finish_device with no slice escaped (every word patches the tail): the counting pass, the scan, the copy by words
  finish_escaped  ... with every slice escaped: the counting pass walks the bytes, the copy goes by bytes

Arrays and workspaces are allocated before the clock starts; the three take turns after the warm-up, each timed by events around
the call (the device's share) and by the host's clock around the call and a synchronisation.  There is no threshold: the medians are
what DESIGN.md quotes.  Prints one JSON line and writes it to --out.

  python tools/finish_bench.py [--steps 20] [--warmup 3] [--only w5] [--out profiles/finish_device.json]
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
SHAPES = (("w2", 2, 512), ("w5", 5, 1 << 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import avrecode_ms_amd as avr
    from avrecode_ms_amd.device import finish_capacity, finish_word

    if avr.device_count() < 1:
        raise SystemExit("finish_bench.py needs a GPU: the epilogue kernels have no CPU path")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = avr.lib()
    result = {"tool": "finish_bench", "library_sha256": avr.library_sha256(), "steps": args.steps, "warmup": args.warmup, "shapes": {}}
    for name, workload, n in SHAPES:
        if args.only and args.only != name:
            continue
        w = avr.DeviceWorkload.synth(workload, n, avr.KIND_CABAC, 0, 1000)
        chunked = n <= 32768 and w.total_bins // n >= 8192               # the batch API's rule, and bench.py's
        (w.encode_chunked if chunked else w.encode)()
        torch.cuda.synchronize()
        w.settle()
        torch.cuda.synchronize()
        assert not int((w.status != 0).sum().item())
        sp = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        regions = int(w.out_off[-1].item())
        capacity = finish_capacity(regions, n)
        dense = torch.empty(capacity, dtype=torch.uint8, device=dev)
        dense_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ws_bytes = max(L.avr_plan_workspace_bytes(n), L.avr_finish_workspace_bytes(n))
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=dev)
        ws_ptr = (ws.data_ptr() + 255) // 256 * 256
        words = {"finish_plain": torch.full((n,), finish_word(0x01, 0, True, False, 0), dtype=torch.int32, device=dev),
                 "finish_escaped": torch.full((n,), finish_word(0x01, 0, True, True, 2), dtype=torch.int32, device=dev)}

        def compact():
            assert L.avr_compact_device(0, sp(), w.out.data_ptr(), w.out_off.data_ptr(), w.out_len.data_ptr(), n, dense.data_ptr(), capacity,
                                        dense_off.data_ptr(), ws_ptr, ws_bytes) == 0

        def finish(which):
            def call():
                assert L.avr_finish_device(0, sp(), w.out.data_ptr(), w.out_off.data_ptr(), w.out_len.data_ptr(), w.status.data_ptr(), n,
                                           words[which].data_ptr(), dense.data_ptr(), capacity, dense_off.data_ptr(), ws_ptr, ws_bytes) == 0
            return call

        steps = {"compact": compact, "finish_plain": finish("finish_plain"), "finish_escaped": finish("finish_escaped")}
        wall, event, total = {k: [] for k in steps}, {k: [] for k in steps}, {}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(args.warmup + args.steps):
            for k, fn in steps.items():                                  # in turns
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ev[0].record()
                fn()
                ev[1].record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                total[k] = int(dense_off[-1].item())
                if i >= args.warmup:
                    wall[k].append((t1 - t0) * 1e3)
                    event[k].append(ev[0].elapsed_time(ev[1]))
        coded = w.output_bytes()
        assert total["compact"] == coded and total["finish_escaped"] >= total["finish_plain"] and max(total.values()) <= capacity
        r = {"workload": workload, "slices": n, "coded_bytes": coded, "region_bytes": regions, "finish_workspace_bytes": L.avr_finish_workspace_bytes(n)}
        for k in steps:
            med = statistics.median(event[k])
            r[k] = {"bytes_out": total[k], "event_ms": {"median": med, "min": min(event[k]), "max": max(event[k])},
                    "wall_ms": {"median": statistics.median(wall[k]), "min": min(wall[k]), "max": max(wall[k])},
                    "gb_per_s": (coded + total[k]) / (med * 1e-3) / 1e9}          # read once, written once (the counting pass's read not counted)
        result["shapes"][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        del w, dense, ws
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    t0 = time.time()
    main()
    print(f"finish_bench.py: {time.time() - t0:.1f} s", file=sys.stderr)
