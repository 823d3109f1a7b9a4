"""Records tests/golden/device_api_refusals.json: what every stateless *_device entry point answers to each case of
tests/device_api_refusals.py, on a machine without a GPU (a call that passes its checks then gets AVR_ERR_NO_DEVICE).

    python tests/golden/make_device_api_refusals.py [path/to/libavrecode_hip.so]

The table pins the refusals as they were BEFORE the launchers took structs: it was recorded from the library built at the commit in
front of that change, and is recorded again only when a refusal is changed on purpose -- then from a build of the commit that
changes it, never to make a failing test pass."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import avrecode_ms_amd as avr          # noqa: E402
import device_api_refusals as cases    # noqa: E402

if __name__ == "__main__":
    if avr.device_count() > 0:
        sys.exit("a GPU is visible: sound calls would reach it with pointers that are not device memory; record where there is none")
    handle = avr._load(sys.argv[1]) if len(sys.argv) > 1 else avr.lib()
    table = cases.table(handle)
    with open(cases.GOLDEN, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{cases.GOLDEN}: {sum(map(len, table.values()))} cases of {len(table)} entry points")
