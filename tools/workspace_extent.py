"""How far into the workspaces they quote K1p and K2p really write: profiles/workspace_extent.json.

For BASELINE.json configs 2 and 4 at their own size: the workspace(s) of encode_chunked() in guarded buffers of exactly the quoted size
(tests/guarded.py), filled with a poison byte, one run, and the offset one past the last byte that no longer holds the poison -- under
two different poisons (a byte a kernel happens to write with the poison's value hides from one, not from both); the larger is the
extent.  A by-product of tests/test_gpu_workspace.py: nothing asserts on these numbers; they are what shrinking a region needs first.

    python tools/workspace_extent.py [--out profiles/workspace_extent.json] [--configs 2,4]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SLICES = {2: 512, 3: 4096, 4: 16384}


def measure(avr, guarded, torch, workload, kind):
    w = avr.DeviceWorkload.synth(workload, SLICES[workload], kind, 0, 1000)
    if kind == avr.KIND_CABAC:
        w.set_parts(0)
    bufs = guarded.install(avr, w)
    spaces = {k: g for k, g in bufs.workspaces().items() if not (k == "ws" and getattr(w, "_parts", None))}
    extent = {k: [] for k in spaces}
    for poison in (0xFF, 0x00):
        bufs.poison(poison, w)
        w.status.zero_()
        w.rows_hint = 0
        w.encode_chunked()
        torch.cuda.synchronize()
        assert not w.settle()["redone"] and not w.status.any()
        bufs.check()
        for k, g in spaces.items():
            extent[k].append(g.extent(poison))
    return {k: {"quoted_bytes": g.n, "touched_bytes": max(extent[k]), "touched_under": {"0xff": extent[k][0], "0x00": extent[k][1]}}
            for k, g in spaces.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "workspace_extent.json"))
    ap.add_argument("--configs", default="2,4")
    a = ap.parse_args()
    import torch
    import avrecode_ms_amd as avr
    import guarded
    report = {"what": "one past the last byte of each quoted workspace that a run changes (tools/workspace_extent.py); "
                      "K1p: avr_cabac_encode_chunked_device_parts, a workspace per part; K2p: avr_range_encode_chunked_device",
              "library_sha256": avr.library_sha256(), "configs": {}}
    for c in (int(x) for x in a.configs.split(",")):
        report["configs"][str(c)] = {"n_slices": SLICES[c],
                                     "k1p": measure(avr, guarded, torch, c, avr.KIND_CABAC),
                                     "k2p": measure(avr, guarded, torch, c, avr.KIND_RANGE)}
        print(json.dumps({c: report["configs"][str(c)]}), flush=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
