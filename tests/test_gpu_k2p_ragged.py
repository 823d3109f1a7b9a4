"""GPU: pass 1 of K2p where lanes and waves share a launch (k_k2p_ranges_hybrid), on the batches of tests/k2p_ragged.py -- built
around the cut, a list that fills the grid to its last block, a block whose lanes all stand aside, and, on both sides of the cut,
the whole (pos, neg) domain, the hand-over to the integer walk, certain records and malformed ones (tests/test_k2p_ragged.py holds the
batches to that on the CPU).  Everywhere else in the suite the hybrid is forced on a few dozen slices, where every slice is long and
the lanes only ever see empty slices; here the batches take their form by their shape, as every realistic compress batch does.

Every run: bytes, length and status per slice are the oracle's, exactly (a slice the oracle does not code: its status).  And after
every run of the hybrid, what k_k2p_threshold left in the workspace -- threshold, count, the listed slices as a set -- is read back
and must be what k2p_ragged.cut() says: no hook tells who walked what, but a slice that neither half walks leaves its notes to what
the workspace held, which the dirty-workspace runs fill with 0xA5.  The region's offset is the stand-alone layout program's
(tests/layout_check.cpp, the k2p line).

Durations on an MI355X (pytest --durations; the whole module 3.8 s and 5.8 s in two runs), the oracle's answers -- once per batch,
shared -- included in the first test that needs them:
  test_form_by_shape     mixed 0.8 to 2.4 s (the process's first device work; and 1.4 to 1.8 s of setup: the libraries, the layout
                         program), wide 0.30 s, wide_plus_one 0.13 s, edge_1025 0.09 s, edge_61441 0.08 s, cut4 0.05 s, brim and both
                         brim_plus_one 0.04 s, edge_1024 0.01 s
  test_segments          mixed 0.02 s (seg_len 1) and 0.01 s, cut4 0.01 s, brim 0.01 s and less
  test_dirty_workspace   0.01 s each
  test_reuse             0.02 s
  test_short_regions     0.01 s each
  test_batch_api         0.01 s"""
import ctypes
import subprocess

import numpy as np
import pytest

import bad_records as br
import k2p_ragged as kr
from test_gpu_bad_records import POISON_LEN, regions
from test_gpu_carry import SENTINEL, assert_untouched
from test_gpu_range_domain import check, run_batch
from test_layouts import EXE, layouts                            # noqa: F401 (the fixture that builds tests/_layout_check)

pytestmark = pytest.mark.gpu

DIRT = 0xA5
_wants = {}


def wants_of(name, oracle):
    """The oracle's answers for a batch, computed once and left unchanged."""
    if name not in _wants:
        _wants[name] = kr.wants(name, oracle)
    return _wants[name]


def workload(avr, name):
    """The batch on the device; the status zeroed (K2p's own validation, not the packer's verdict), out and out_len as no path leaves them."""
    slices, _ = kr.BATCHES[name][0]()
    w = avr.DeviceWorkload.from_host(avr.KIND_RANGE, slices, None, 0)
    fresh(w)
    return w


def fresh(w):
    w.out.fill_(SENTINEL)
    w.out_len.fill_(POISON_LEN)
    w.status.zero_()


def quote(avr, w):
    p = w._chunk_plan()
    return avr.lib().avr_range_chunked_workspace_bytes(w.n_slices, ctypes.byref(p["plan"]), int(w.out_off[-1].item()))


def own_workspace(avr, w, n_bytes=None, fill=None):
    """A K2p workspace of the caller's making, as encode_chunked() would allocate it: filled beforehand, or sized for another batch."""
    import torch
    n = quote(avr, w)
    ws = torch.empty(max(n, n_bytes or 0) + 256, dtype=torch.uint8, device=w.out.device)
    if fill is not None:
        ws.fill_(fill)
    p = w._chunk_plan()
    p["ws_k2"], p["ws_k2_bytes"] = ws, max(n, n_bytes or 0)
    return ws


def long_list(avr, w):
    """(threshold, count, the listed slices) as the run left them in the workspace."""
    import torch
    torch.cuda.synchronize()
    p = w._chunk_plan()
    plan = p["plan"]
    shape = f"{w.n_slices} 0 1 {plan.res_total} {plan.dig_total} {plan.total_chunks} {plan.total_blocks} {p['out_total']}\n"
    out = subprocess.run([EXE], input=shape, capture_output=True, text=True, check=True).stdout.split("\n")
    k2p = [int(x) for x in next(line for line in out if line.startswith("k2p ")).split()[1:]]
    assert k2p[-1] == avr.lib().avr_range_chunked_workspace_bytes(w.n_slices, ctypes.byref(plan), p["out_total"]) <= p["ws_k2_bytes"]
    ws = p["ws_k2"]
    start = (ws.data_ptr() + 255) // 256 * 256 - ws.data_ptr() + k2p[4]          # device.py's _aligned, then long_chunks
    words = ws[start:start + k2p[5] - k2p[4]].cpu().numpy().view(np.uint32)
    threshold, count = int(words[0]), int(words[1])
    assert count <= words.size - 2
    return threshold, count, words[2:2 + count].tolist()


def check_list(avr, w, name, what):
    slices, _ = kr.BATCHES[name][0]()
    assert kr.shape(len(slices))[2] == "hybrid"
    threshold, long_ = kr.cut_of(slices)
    assert (threshold, len(long_)) == kr.BATCHES[name][1:]
    got_t, got_n, got = long_list(avr, w)
    assert (got_t, got_n) == (threshold, len(long_)), f"{what}: threshold and count {got_t}, {got_n}; the rule's {threshold}, {len(long_)}"
    assert len(set(got)) == got_n and set(got) == set(long_), f"{what}: the listed slices are not the rule's"


def run(avr, oracle, name, what, w=None, lists=True):
    """encode_chunked(), the answers against the oracle's, the list against the rule: the bytes per slice."""
    w = w or workload(avr, name)
    w.encode_chunked()
    got, status = w.results()
    check(got, status, wants_of(name, oracle), f"{name}, {what}")
    lens = w.out_len.cpu().numpy()
    for i, (_, st) in enumerate(wants_of(name, oracle)):
        if st == br.SLICE_BAD_RECORD:
            assert lens[i] == 0, f"{name}, {what}: slice {i}: a malformed slice with {lens[i]} bytes"
    if lists:
        check_list(avr, w, name, what)
    return got, status


# ------------------------------------------------------------------ the product library: every form by shape alone

@pytest.mark.parametrize("name", kr.BATCHES)
def test_form_by_shape(avr, oracle, layouts, name):              # noqa: F811
    """No hook: lanes plus waves for 1 025 .. 61 440 slices.  The 1 024-slice batch (a wave per slice) and the 61 441-slice batch (a lane
    per slice) stand on the other side of each boundary; those forms write no list."""
    run(avr, oracle, name, "by shape", lists=kr.BATCHES[name][1] is not None)


# ------------------------------------------------------------------ segments

@pytest.mark.parametrize("seg_len", [1, 3])
@pytest.mark.parametrize("name", ["mixed", "cut4", "brim"])
def test_segments(avr, oracle, hooks, layouts, name, seg_len):   # noqa: F811
    """k2p_seg_len 1 and 3, the form still by shape: lanes and waves pick up at the same seams from the notes the segment before left,
    one-chunk slices end in segment 0 while their block's long neighbours walk on into the open-ended last segment, and the long
    side's malformed records sit in a later segment."""
    hooks(k2p_seg_len=seg_len)
    run(avr, oracle, name, f"seg_len {seg_len}")


# ------------------------------------------------------------------ the workspace

@pytest.mark.parametrize("name", ["mixed", "brim"])
def test_dirty_workspace(avr, oracle, layouts, name):            # noqa: F811
    """Every byte of the workspace 0xA5 beforehand: the same bytes, and the list is the rule's -- every slice was walked by one half."""
    w = workload(avr, name)
    own_workspace(avr, w, fill=DIRT)
    run(avr, oracle, name, "dirty workspace", w)


def test_reuse(avr, oracle, layouts):                            # noqa: F811
    """mixed, brim_plus_one (nothing long), mixed -- through one workspace sized for the larger: the list is written anew each time
    (a count of 0 after the middle run), and the third run equals the first."""
    a, b = workload(avr, "mixed"), workload(avr, "brim_plus_one")
    ws = own_workspace(avr, a, n_bytes=quote(avr, b), fill=DIRT)
    pb = b._chunk_plan()
    pb["ws_k2"], pb["ws_k2_bytes"] = ws, a._chunk_plan()["ws_k2_bytes"]
    first = run(avr, oracle, "mixed", "first run", a)
    run(avr, oracle, "brim_plus_one", "the run in between", b)
    assert long_list(avr, b)[:2] == (4, 0)
    fresh(a)
    assert run(avr, oracle, "mixed", "third run", a) == first


# ------------------------------------------------------------------ output regions

@pytest.mark.parametrize("seg_len", [0, 3])
def test_short_regions(avr, oracle, hooks, layouts, seg_len):    # noqa: F811
    """Regions at 8 mod 16 in a buffer full of the sentinel, and the region of one clean lane slice and of one clean wave slice cut to
    64 bytes: both end AVR_SLICE_OVERFLOW, every other slice is the oracle's, nothing outside any slice's bytes is written."""
    hooks(k2p_seg_len=seg_len)
    slices, special = kr.mixed()
    wants = wants_of("mixed", oracle)
    lane, wave = kr.short_region_picks(slices, special, wants)
    w = workload(avr, "mixed")
    off = regions(w, {lane: 64, wave: 64})
    w.encode_chunked()
    got, status = w.results()
    assert [status[lane], status[wave]] == [avr.SLICE_OVERFLOW] * 2
    keep = [i for i in range(len(slices)) if i not in (lane, wave)]
    check([got[i] for i in keep], [status[i] for i in keep], [wants[i] for i in keep], f"short regions, seg_len {seg_len}")
    assert_untouched(w, off, overflowed=[lane, wave])
    check_list(avr, w, "mixed", f"short regions, seg_len {seg_len}")


# ------------------------------------------------------------------ the batch API

def test_batch_api(avr, oracle, hooks):
    """avr.Batch on its chunked path (hook k1_path = 2, as test_range_chunked_random_and_extremes forces it): 1 100 slices take
    the hybrid by shape there too.  The same bytes and statuses."""
    hooks(k1_path=2)
    slices, _ = kr.mixed()
    got, status, _ = run_batch(avr, slices, verify=False)
    check(got, status, wants_of("mixed", oracle), "avr.Batch, chunked")
