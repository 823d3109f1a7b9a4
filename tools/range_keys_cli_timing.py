"""AVR_DEVICE_ESTIMATORS on the command line, timed: `AVR_TIMING=1 recode compress <clip>` (its phases from stderr) and
`recode test <dir>` over 16 copies of each golden clip (wall time), medians of --runs runs, the variants taking turns:

  baseline   --baseline-recode PATH, another build of the command to compare with (optional), variable unset
  unset      this build, variable unset
  set        this build, AVR_DEVICE_ESTIMATORS=1

Every variant's compressed file must be the same bytes.  Prints one JSON line and writes it to --out.

  python tools/range_keys_cli_timing.py [--runs 5] [--baseline-recode PATH] [--clip cockatoo.mp4] [--out FILE]
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--baseline-recode", default="")
    ap.add_argument("--clip", default="cockatoo.mp4")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import avrecode_ms_amd as avr
    variants = {"unset": (avr.RECODE_PATH, {}), "set": (avr.RECODE_PATH, {"AVR_DEVICE_ESTIMATORS": "1"})}
    if args.baseline_recode:
        variants = {"baseline": (args.baseline_recode, {}), **variants}
    result = {"tool": "range_keys_cli_timing", "library_sha256": avr.library_sha256(), "runs": args.runs, "clip": args.clip,
              "compress": {}, "test_dir": {}}
    with tempfile.TemporaryDirectory() as tmp:
        clip = os.path.join(GOLD, args.clip)
        phases = {v: {} for v in variants}
        files = {}
        for run in range(args.runs + 1):                             # the first round is the warm-up
            for v, (exe, extra) in variants.items():
                out = os.path.join(tmp, v + ".recode")
                env = dict(os.environ, AVR_TIMING="1", **extra)
                env.pop("AVR_DEVICE_ESTIMATORS", None) if not extra else None
                t0 = time.perf_counter()
                r = subprocess.run([exe, "compress", clip, out], capture_output=True, text=True, env=env, timeout=600)
                wall = 1e3 * (time.perf_counter() - t0)
                if r.returncode != 0:
                    raise SystemExit(f"{v}: recode compress failed: {r.stderr[-500:]}")
                files[v] = open(out, "rb").read()
                if run == 0:
                    continue
                phases[v].setdefault("wall", []).append(wall)
                for what, ms in re.findall(r"\[timing\] (.*?)\s+([0-9.]+) ms", r.stderr):
                    phases[v].setdefault(what.strip(), []).append(float(ms))
        if len(set(files.values())) != 1:
            raise SystemExit("the variants' compressed files differ")
        for v in variants:
            result["compress"][v] = {k: {"median_ms": statistics.median(x), "min_ms": min(x), "max_ms": max(x)} for k, x in phases[v].items()}
        walls = {v: [] for v in variants}
        for run in range(args.runs + 1):
            for v, (exe, extra) in variants.items():
                d = os.path.join(tmp, f"dir_{v}")
                shutil.rmtree(d, ignore_errors=True)
                os.makedirs(d)
                for k in range(16):
                    for name in ("realshort.mp4", "cockatoo.mp4"):
                        shutil.copy(os.path.join(GOLD, name), os.path.join(d, f"{k:02d}_{name}"))
                env = dict(os.environ, **extra)
                env.pop("AVR_DEVICE_ESTIMATORS", None) if not extra else None
                t0 = time.perf_counter()
                r = subprocess.run([exe, "test", d], capture_output=True, text=True, env=env, timeout=1800)
                wall = 1e3 * (time.perf_counter() - t0)
                if r.returncode != 0 or "failed on" in r.stdout:
                    raise SystemExit(f"{v}: recode test failed: {r.stderr[-500:]}")
                if run:
                    walls[v].append(wall)
        for v in variants:
            result["test_dir"][v] = {"files": 32, "wall_ms": {"median": statistics.median(walls[v]), "min": min(walls[v]), "max": max(walls[v])}}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
