"""One-byte K1 records on the one-lane-per-slice path: the two-byte route against the one-byte tiles, on config 5 densified and
narrowed on the device (BASELINE.json configs[4]; 1 Mi slices at full size).

  two-byte  avr_pack_tiles8_device (widen + validate + transpose)  ->  avr_cabac_encode_tiles_device_hinted, with a settled hint
  narrow    avr_pack_tiles8_narrow_device (validate + transpose)   ->  avr_cabac8_encode_tiles_device

The two routes take turns, step by step; pack and encode are timed apart with events (status is zeroed before each step, outside
the timed span).  Afterwards both routes run once more into zeroed outputs, and every slice's bytes, final states and statuses
must be identical.  Prints one JSON line and writes it to --out.

  python tools/cabac8_tiles_bench.py [--slices N] [--steps 20] [--warmup 3] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import avrecode_ms_amd as avr

    L = avr.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    t0 = time.time()
    w = avr.DeviceWorkload.synth(5, args.slices, avr.KIND_CABAC, 0, 1000)
    w.densify()
    narrow = w.to_cabac8(narrow_tiles=True)
    del w
    two = avr.DeviceWorkload._pack8(0, narrow.rec8_flat, narrow.rec8_off, narrow.n_bins, narrow.init_states, narrow.n_states, False)
    torch.cuda.synchronize()
    setup_s = time.time() - t0
    n, ns = narrow.n_slices, narrow.n_states
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    counts = torch.zeros(2, dtype=torch.int32).pin_memory()
    hint = [0]

    def pack(x):
        f = L.avr_pack_tiles8_narrow_device if x is narrow else L.avr_pack_tiles8_device
        rc = f(0, sp, ns, x.rec8_flat.data_ptr(), x.rec8_off.data_ptr(), x.n_bins.data_ptr(), x.order.data_ptr(), n,
               x.tile_off.data_ptr(), x.tiles.data_ptr(), x.status.data_ptr())
        assert rc == 0, L.avr_last_error().decode()

    def encode(x):
        a = (0, sp, x.tiles.data_ptr(), x.tile_off.data_ptr(), x.n_bins.data_ptr(), x.order.data_ptr(), n, x.init_states.data_ptr(), ns,
             x.out.data_ptr(), x.out_off.data_ptr(), x.out_len.data_ptr(), x.status.data_ptr(), x.final_states.data_ptr())
        rc = L.avr_cabac8_encode_tiles_device(*a) if x is narrow else L.avr_cabac_encode_tiles_device_hinted(*a, hint[0], counts.data_ptr())
        assert rc == 0, L.avr_last_error().decode()

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    times = {"two_byte": {"pack": [], "encode": []}, "narrow": {"pack": [], "encode": []}}
    for step in range(args.warmup + args.steps):
        for name, x in (("two_byte", two), ("narrow", narrow)) if step % 2 == 0 else (("narrow", narrow), ("two_byte", two)):
            x.status.zero_()
            ev[0].record()
            pack(x)
            ev[1].record()
            encode(x)
            ev[2].record()
            torch.cuda.synchronize()
            if x is two:                                    # the hint settles as avr_batch and DeviceWorkload.settle() settle it
                rows = int(counts[0])
                if rows:
                    hint[0] = min(ns, rows + 8)
            if step >= args.warmup:
                times[name]["pack"].append(ev[0].elapsed_time(ev[1]))
                times[name]["encode"].append(ev[1].elapsed_time(ev[2]))

    # every slice's bytes, final states and statuses: both routes once more into zeroed outputs
    for x in (two, narrow):
        x.out.zero_(); x.out_len.zero_(); x.final_states.zero_(); x.status.zero_()
        pack(x)
        encode(x)
    torch.cuda.synchronize()
    identical = bool(torch.equal(two.out_len, narrow.out_len) and torch.equal(two.status, narrow.status)
                     and torch.equal(two.final_states, narrow.final_states) and torch.equal(two.out_off, narrow.out_off)
                     and torch.equal(two.out, narrow.out))
    bad_status = int((narrow.status != 0).sum())

    def summ(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}

    res = {
        "what": "config 5 (densified, narrowed to one-byte records): two-byte route vs one-byte tiles, one lane per slice",
        "cmd": "python tools/cabac8_tiles_bench.py " + " ".join(sys.argv[1:]),
        "slices": n, "bins": narrow.total_bins, "n_states": ns, "setup_s": round(setup_s, 1),
        "two_byte_route": "avr_pack_tiles8_device + avr_cabac_encode_tiles_device_hinted (rows_hint %d)" % hint[0],
        "narrow_route": "avr_pack_tiles8_narrow_device + avr_cabac8_encode_tiles_device",
        "tiles_bytes": {"two_byte": int(two.tile_off[-1]) * 16, "narrow": int(narrow.tile_off[-1]) * 16},
        "two_byte": {k: summ(v) for k, v in times["two_byte"].items()},
        "narrow": {k: summ(v) for k, v in times["narrow"].items()},
        "all_slices_identical": identical, "slices_not_ok": bad_status,
        "output_bytes": narrow.output_bytes(),
    }
    for r in ("two_byte", "narrow"):
        res[r]["step_median_ms"] = statistics.median(p + e for p, e in zip(times[r]["pack"], times[r]["encode"]))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not identical or bad_status:
        sys.exit(1)


if __name__ == "__main__":
    main()
