"""Every stateless *_device entry point refuses what it refused before its arguments travelled to the launchers as structs: the same
arguments, the same return code, the same avr_last_error() text.  The cases are device_api_refusals.py's; the expected table
(golden/device_api_refusals.json) was recorded from the library of the commit in front of that change, never from the code under test.
No call here may touch a device: the checks run in front of select_device, and a call that passes them all is made only where no GPU
is visible (it returns AVR_ERR_NO_DEVICE there)."""
import json

import pytest

import device_api_refusals as cases


@pytest.fixture(scope="module")
def expected():
    with open(cases.GOLDEN) as f:
        return json.load(f)


def _gpu_visible():
    import torch
    return torch.cuda.is_available()


def test_the_table_covers_every_entry_point_and_every_case(avr, expected):
    points = cases.entry_points()
    assert len(points) >= 34 and cases.PARTS in points
    assert sorted(expected) == sorted(points)
    for fn, params in points.items():
        assert sorted(expected[fn]) == sorted(label for label, _ in cases.cases(avr.lib(), fn, params)), fn
        assert expected[fn]["sound"] == [cases.NO_DEVICE, "no HIP device visible; this library has no CPU coding path"], fn


@pytest.mark.parametrize("build", ["product", "hooks"])
def test_every_refusal_is_the_recorded_one(avr, expected, build):
    # with a GPU visible, what the recorded library let through to the device is not called at all: the pointers are not device memory
    skip = (lambda fn, label: expected[fn][label][0] == cases.NO_DEVICE) if _gpu_visible() else (lambda fn, label: False)
    if build == "hooks":
        with avr.test_hooks() as handle:
            got = cases.table(handle, skip)
    else:
        got = cases.table(avr.lib(), skip)
    wrong = [(fn, label, got[fn][label], expected[fn][label]) for fn in got for label in got[fn] if got[fn][label] != expected[fn][label]]
    assert not wrong, f"{len(wrong)} answers differ from the recorded ones (function, case, got, recorded): {wrong[:10]}"
    refused = sum(1 for fn in got for label in got[fn] if got[fn][label][0] != cases.NO_DEVICE)
    assert refused >= 350                                        # the table is about refusals, not about one answer given 800 times
