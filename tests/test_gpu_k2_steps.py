"""GPU: one bin of the K2 coders on the device itself, held to plain 64-bit integers (tests/k2_steps_cases.h, see
tests/test_k2_steps.py for the cases).  tests/k2_steps_dev.hip runs the `__device__` side of csrc/avr_div.h and csrc/avr_k2p.h, one
lane a case: the reciprocals by gfx950's FP64 division, range_step and bin<true> over avr_div.h's quotient, range_step_fp one step at a
time and in chains.  The program only returns raw results; the comparison happens on the host."""
import subprocess
import time

import pytest

import test_k2_steps as steps

pytestmark = pytest.mark.gpu

# Measured on an MI355X: the child takes 0.9 to 1.1 s from start to exit (four runs: alone, inside the whole suite, first in a fresh session), the
# making of the 4.36 M cases and their comparison on the host included.  The limit is ten times the slowest (as
# tests/test_gpu_threads.py has it for its children); a child that runs into it counts as hung.
MEASURED_S = 1.1
LIMIT_S = 10 * MEASURED_S


def test_device_side_is_exact():
    program = steps.build_dev()
    t0 = time.perf_counter()
    child = subprocess.run([program], capture_output=True, text=True, timeout=LIMIT_S)
    print(f"tests/_k2_steps_dev took {time.perf_counter() - t0:.1f} s, exit status {child.returncode}")
    print(child.stderr[-3000:])
    steps.assert_clean(child)
