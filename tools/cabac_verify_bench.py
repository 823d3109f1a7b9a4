"""The K1 verifier (avr_cabac_verify_*_device / avr_cabac8_verify_*_device: every coded slice decoded back on the device, as the CABAC
stream it is, against its records or codes) timed beside the encode of the same batch, on the synthetic workloads:

  w5_tiles     config 5 (1 Mi slices): one lane per slice over two-byte tiles -- encode(), verifier over the same tiles
  w5_tiles8    the same slices densified and narrowed: one-byte tiles, avr_cabac8_encode_tiles_device, verifier over the same tiles
  w2_k1p       config 2 (512 slices): K1p (encode_chunked()), verifier one lane per slice over the slice-major records
  w2_codes     config 2 from resolved codes: K1p phases B-D (encode_resolved()), verifier one lane per slice over the codes

Per shape, with events around the calls and the two steps taking turns after the warm-up: the encode alone, the verifier alone (on the
bytes the encode just wrote, with the encoder's final states to compare where the form has states; it must find nothing).  There is no
threshold: the figures are a cost to report, and what README.md and DESIGN.md quote.
--merge FILE: a JSON object whose keys are added to the result (where the kernel's register figures and the bench.py runs of the same
visit are recorded).  Prints one JSON line and writes it to --out.

  python tools/cabac_verify_bench.py [--steps 20] [--warmup 3] [--slices5 1048576] [--slices2 512] [--only NAME] [--merge FILE] [--out FILE]
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
    ap.add_argument("--only", default="")
    ap.add_argument("--merge", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import avrecode_ms_amd as avr

    if avr.device_count() < 1:
        raise SystemExit("cabac_verify_bench.py needs a GPU: the verifier has no CPU path")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    result = {"tool": "cabac_verify_bench", "library_sha256": avr.library_sha256(), "steps": args.steps, "warmup": args.warmup, "shapes": {}}
    for name, workload, n, form in (("w5_tiles", 5, args.slices5, "two-byte tiles"), ("w5_tiles8", 5, args.slices5, "one-byte tiles"),
                                    ("w2_k1p", 2, args.slices2, "slice-major records"), ("w2_codes", 2, args.slices2, "codes")):
        if args.only and args.only != name:
            continue
        w = avr.DeviceWorkload.synth(workload, n, avr.KIND_CABAC, 0, 1000)
        chunked = workload == 2
        assert chunked == (n <= 32768 and w.total_bins // n >= 8192)      # the batch API's rule, and bench.py's
        if name == "w5_tiles8":
            w.densify()
            w = w.to_cabac8(narrow_tiles=True)
        if name == "w2_codes":
            codes = w.resolve()
            encode = lambda: w.encode_resolved(codes)
        else:
            encode = w.encode_chunked if chunked else w.encode
        found = []

        def verify():
            found.append(w.verify_k1())

        steps = {"encode": encode, "verify": verify}
        times = {k: [] for k in steps}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(args.warmup + args.steps):
            for k in ("encode", "verify"):                               # in turns: the verifier reads what the encode before it wrote
                ev[0].record()
                steps[k]()
                ev[1].record()
                torch.cuda.synchronize()
                if k == "encode" and name != "w2_codes":
                    w.settle()                                           # (a run sized by a guess: what it left is done before the verifier)
                if i >= args.warmup:
                    times[k].append(ev[0].elapsed_time(ev[1]))
            assert int((found.pop() != -1).sum().item()) == 0            # AVR_VERIFY_NONE everywhere
        assert not int((w.status != 0).sum().item())
        r = {"workload": workload, "slices": n, "bins": w.total_bins, "coded_bytes": w.output_bytes(), "n_states": w.n_states,
             "k1_path": "k1p" if chunked else "lanes", "verifier": form}
        for k, v in times.items():
            r[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        r["verify_over_encode"] = r["verify_ms"]["median"] / r["encode_ms"]["median"]
        result["shapes"][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
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
    print(f"cabac_verify_bench.py: {time.time() - t0:.1f} s", file=sys.stderr)
