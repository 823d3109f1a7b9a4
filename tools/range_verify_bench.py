"""The K2 verifier (avr_range_verify_tiles_device / avr_range_verify_slices_device: every coded slice decoded back on the device against
its records) timed beside the encode of the same batch, on the synthetic workloads:

  w5_tiles   config 5 (1 Mi slices): one lane per slice over tiles -- encode avr_range_encode_tiles_device, verifier over the same tiles
  w2_k2p     config 2 (512 slices): K2p (avr_range_encode_chunked_device), verifier one lane per slice over the slice-major records

Per shape, with events around the calls and the two steps taking turns after the warm-up: the encode alone, the verifier alone (on the
bytes the encode just wrote; it must find nothing).  There is no threshold: the figures are what README.md and DESIGN.md quote.
--merge FILE: a JSON object whose keys are added to the result (where the kernel's register figures and the bench.py runs of the same
visit are recorded).  Prints one JSON line and writes it to --out.

  python tools/range_verify_bench.py [--steps 20] [--warmup 3] [--slices5 1048576] [--slices2 512] [--merge FILE] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slices5", type=int, default=1 << 20)
    ap.add_argument("--slices2", type=int, default=512)
    ap.add_argument("--merge", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import avrecode_ms_amd as avr

    if avr.device_count() < 1:
        raise SystemExit("range_verify_bench.py needs a GPU: the verifier has no CPU path")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    result = {"tool": "range_verify_bench", "library_sha256": avr.library_sha256(), "steps": args.steps, "warmup": args.warmup, "shapes": {}}
    for name, workload, n, chunked in (("w5_tiles", 5, args.slices5, False), ("w2_k2p", 2, args.slices2, True)):
        w = avr.DeviceWorkload.synth(workload, n, avr.KIND_RANGE, 0, 1000)
        assert chunked == (n <= 32768 and w.total_bins // n >= 8192)      # the batch API's rule, and bench.py's
        encode = w.encode_chunked if chunked else w.encode
        found = []

        def verify():
            found.append(w.verify())

        steps = {"encode": encode, "verify": verify}
        times = {k: [] for k in steps}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(args.warmup + args.steps):
            for k in ("encode", "verify"):                               # in turns: the verifier reads what the encode before it wrote
                ev[0].record()
                steps[k]()
                ev[1].record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times[k].append(ev[0].elapsed_time(ev[1]))
            assert int((found.pop() != -1).sum().item()) == 0            # AVR_VERIFY_NONE everywhere
        assert not int((w.status != 0).sum().item())
        r = {"workload": workload, "slices": n, "bins": w.total_bins, "coded_bytes": w.output_bytes(),
             "k2_path": "k2p" if chunked else "lanes", "verifier": "slice-major" if chunked else "tiles"}
        for k, v in times.items():
            r[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        r["verify_over_encode"] = r["verify_ms"]["median"] / r["encode_ms"]["median"]
        result["shapes"][name] = r
        del w
    if args.merge:
        with open(args.merge) as f:
            result.update(json.load(f))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    t0 = time.time()
    main()
    print(f"range_verify_bench.py: {time.time() - t0:.1f} s", file=sys.stderr)
