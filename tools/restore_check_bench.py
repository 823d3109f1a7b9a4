"""The restore check (avr_restore_check_device: every coded K1 slice through the decompressor's epilogue rule against the payload it is
to restore) timed beside the encode of the same batch, on the synthetic workloads:

  w5   config 5 (1 Mi short slices): one lane per slice over two-byte tiles -- encode(), then the check, a wave per slice
  w2   config 2 (512 long slices): K1p (encode_chunked()), then the check

The expectations are made on the device from the bytes the encode wrote: slice i expects its own coded bytes without the stop byte, at
the region's offset in a copy of `out` (regions start at multiples of 8, as expectations must) -- a payload the rule restores exactly,
so the check walks every byte of every slice and must find nothing.  Per shape, with events around the calls and the two steps taking
turns after the warm-up: the encode alone, the check alone.  Beside the times, what the command line's route adds over PCIe per bin:
one code byte a bin and the payload, against the two bytes a bin of key or range records the compress direction sends anyway.
There is no threshold: the figures are a cost to report, and what README.md and DESIGN.md quote.
--merge FILE: a JSON object whose keys are added to the result.  Prints one JSON line and writes it to --out.

  python tools/restore_check_bench.py [--steps 20] [--warmup 3] [--slices5 1048576] [--slices2 512] [--only NAME] [--merge FILE] [--out FILE]
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

    import ctypes
    import torch
    import avrecode_ms_amd as avr

    if avr.device_count() < 1:
        raise SystemExit("restore_check_bench.py needs a GPU: the check has no CPU path")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = avr.lib()
    result = {"tool": "restore_check_bench", "library_sha256": avr.library_sha256(), "steps": args.steps, "warmup": args.warmup, "shapes": {}}
    for name, workload, n in (("w5", 5, args.slices5), ("w2", 2, args.slices2)):
        if args.only and args.only != name:
            continue
        w = avr.DeviceWorkload.synth(workload, n, avr.KIND_CABAC, 0, 1000)
        chunked = workload == 2
        assert chunked == (n <= 32768 and w.total_bins // n >= 8192)      # the batch API's rule, and bench.py's
        encode = w.encode_chunked if chunked else w.encode
        encode()
        torch.cuda.synchronize()
        w.settle()
        torch.cuda.synchronize()
        assert not int((w.status != 0).sum().item())
        # the expectations: the coded bytes without the stop byte, where they lie in a copy of out
        expect = w.out.clone()
        expect_off = w.out_off[:-1].clone()
        lens = w.out_len.to(torch.int64)
        last = w.out[(w.out_off[:-1] + (lens - 1).clamp(min=0)).to(torch.int64)]
        expect_len = (lens - ((lens > 0) & (last == 0x80)).to(torch.int64)).to(torch.int32)
        first_diff = torch.empty(n, dtype=torch.int32, device=dev)

        def check():
            sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc = L.avr_restore_check_device(0, sp, w.out.data_ptr(), w.out_off.data_ptr(), w.out_len.data_ptr(), n, expect.data_ptr(),
                                            expect_off.data_ptr(), expect_len.data_ptr(), w.status.data_ptr(), first_diff.data_ptr())
            assert rc == 0, L.avr_last_error().decode()

        steps = {"encode": encode, "check": check}
        times = {k: [] for k in steps}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(args.warmup + args.steps):
            for k in ("encode", "check"):                                # in turns: the check reads what the encode before it wrote
                ev[0].record()
                steps[k]()
                ev[1].record()
                torch.cuda.synchronize()
                if k == "encode":
                    w.settle()                                           # (a run sized by a guess: what it left is done before the check)
                if i >= args.warmup:
                    times[k].append(ev[0].elapsed_time(ev[1]))
            assert int((first_diff != -1).sum().item()) == 0             # AVR_VERIFY_NONE everywhere
        assert not int((w.status != 0).sum().item())
        coded, payload = w.output_bytes(), int(expect_len.to(torch.int64).sum().item())
        r = {"workload": workload, "slices": n, "bins": w.total_bins, "coded_bytes": coded, "payload_bytes": payload,
             "k1_path": "k1p" if chunked else "lanes"}
        for k, v in times.items():
            r[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        r["check_over_encode"] = r["check_ms"]["median"] / r["encode_ms"]["median"]
        r["check_read_gb_per_s"] = (coded + payload) / (r["check_ms"]["median"] * 1e-3) / 1e9       # both strings once, over the check's time
        # what AVR_VERIFY_RESTORE=1 adds over PCIe per bin: one resolved code a bin, and the payload as the expectation
        r["cli_added_pcie_bytes_per_bin"] = {"codes": 1.0, "payload": payload / w.total_bins, "total": 1.0 + payload / w.total_bins}
        result["shapes"][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        del w, expect
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
    print(f"restore_check_bench.py: {time.time() - t0:.1f} s", file=sys.stderr)
