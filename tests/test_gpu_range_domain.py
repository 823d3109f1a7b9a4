"""GPU: every library path that reads a K2 record, on streams that hold every (pos, neg) the ABI accepts (tests/range_domain.py;
tests/test_range_domain.py holds the streams to their preconditions on the CPU).  The random streams of the other GPU tests stop at
pos, neg < 0x60 and totals of 0x60; here totals reach 254, so that the upper quarter of every reciprocal table the kernels fill for
themselves -- by total, by 2 total + bin, by the record's low byte -- is read, and renormalisations by 16 bits are common.  Bytes,
lengths and statuses are the oracle's, exactly.  The collapse batch plants `bin 0, pos p, neg 0` (the new range is range mod p: the
double-precision walk of K2p hands the slice to the integer one, and a remainder of 0 is AVR_SLICE_ZERO_PROB) at the seams of chunks
and segments."""
import ctypes

import pytest

import range_domain as rd
from verify_streams import VERIFY_NONE

pytestmark = pytest.mark.gpu

SEED_DOMAIN, SEED_COLLAPSE = 2054, 2055                          # tests/test_range_domain.py checks these very batches
K2P = [(seg_len, pass1) for seg_len in (0, 1, 3) for pass1 in ("wave", "lane", "both")]
K2P_IDS = [f"seg{seg_len}-{pass1}" for seg_len, pass1 in K2P]
BATCH_PATHS = {"serial": 1, "chunked": 2}


@pytest.fixture(scope="module")
def domain(oracle):
    """(slices, the oracle's (bytes, status) per slice): every status is 0."""
    slices = rd.domain_batch(SEED_DOMAIN)
    wants = [oracle.range_encode(s) for s in slices]
    assert [st for _, st in wants] == [0] * len(slices)
    return slices, wants


@pytest.fixture(scope="module")
def collapse(oracle):
    """(slices, the oracle's (bytes, status) per slice): both a coded collapse and a bin of probability zero occur."""
    slices, planted = rd.collapse_batch(SEED_COLLAPSE)
    wants = [oracle.range_encode(s) for s in slices]
    hit = [st for (_, st), at in zip(wants, planted) if at is not None]
    assert set(hit) == {0, rd.ZERO_PROB} and all(st == 0 for (_, st), at in zip(wants, planted) if at is None)
    return slices, wants


def k2p_hooks(hooks, seg_len, pass1, **more):
    lane = {"k2p_wave": 2} if pass1 == "lane" else {"k2p_wave": 3} if pass1 == "both" else {}
    hooks(k2p_seg_len=seg_len, **lane, **more)


def check(got, status, wants, what):
    """Status for status; bytes (and with them the length) for every slice the oracle coded."""
    assert len(got) == len(status) == len(wants)
    for i, (data, st) in enumerate(wants):
        assert status[i] == st, f"{what}: slice {i}: status {status[i]}, the oracle's {st}"
        if st == 0:
            assert got[i] == data, f"{what}: slice {i}: {len(got[i])} bytes differ from the oracle's {len(data)}"


def check_workload(w, wants, what):
    got, status = w.results()
    check(got, status, wants, what)
    return got


def clear(w):
    w.out.zero_(); w.out_len.zero_(); w.status.zero_()


def workload(avr, slices):
    w = avr.DeviceWorkload.from_host(avr.KIND_RANGE, slices, None, 0)
    assert w.status.cpu().numpy().tolist() == [0] * len(slices)  # the packer refuses none of these records
    return w


def run_batch(avr, slices, verify, b=None):
    """The slices through avr.Batch: (bytes per slice, statuses, get_verify per slice)."""
    own = b is None
    if own:
        b = avr.Batch(0, len(slices), sum(len(s) for s in slices) + 8)
    try:
        b.set_verify(verify)
        for i, s in enumerate(slices):
            assert b.add_slice_range(s) == i
        b.run()
        out = [b.get(i) for i in range(len(slices))]
        return [o[0] for o in out], [o[1] for o in out], [b.get_verify(i) for i in range(len(slices))]
    finally:
        if own:
            b.close()


# ------------------------------------------------------------------ the domain batch

def test_one_lane_per_slice_tiles_and_slice_major(avr, domain):
    """The packer and k_range_encode over tiles, then the slice-major entry the batch API takes on its serial path."""
    slices, wants = domain
    w = workload(avr, slices)
    w.encode()
    check_workload(w, wants, "tiles")
    clear(w)
    w.encode_slice_major()
    check_workload(w, wants, "slice major")


@pytest.mark.parametrize("seg_len,pass1", K2P, ids=K2P_IDS)
def test_k2p(avr, domain, hooks, seg_len, pass1):
    """The hooks of test_range_chunked_random_and_extremes (tests/test_gpu_k1p.py): pass 1 by a wave, a lane or both per slice, the
    passes in one piece and in segments of 1 and 3 chunks."""
    k2p_hooks(hooks, seg_len, pass1)
    slices, wants = domain
    w = workload(avr, slices)
    w.encode_chunked()
    check_workload(w, wants, f"seg_len {seg_len} pass1 {pass1}")


@pytest.mark.parametrize("path", BATCH_PATHS)
def test_batch_api_with_the_device_decoder_behind_it(avr, domain, hooks, path):
    """set_verify on: k_range_verify (csrc/avr_verify.h) decodes every slice back with the same divisors and finds nothing; the bytes
    are the oracle's and those of the run without it."""
    hooks(k1_path=BATCH_PATHS[path])
    slices, wants = domain
    plain, status, found = run_batch(avr, slices, verify=False)
    check(plain, status, wants, f"{path}, verify off")
    assert found == [VERIFY_NONE] * len(slices)
    checked, status, found = run_batch(avr, slices, verify=True)
    check(checked, status, wants, f"{path}, verify on")
    assert found == [VERIFY_NONE] * len(slices), [(i, f) for i, f in enumerate(found) if f != VERIFY_NONE][:8]
    assert checked == plain


@pytest.mark.parametrize("how", ["workspace", "batch"])
def test_reuse_after_the_collapse_batch(avr, domain, collapse, hooks, how):
    """The domain batch, the collapse batch (larger; slices handed over, slices in error), the domain batch again -- through one K2p
    workspace sized for the larger, and through one avr.Batch on its chunked path: the third run equals the first."""
    import torch
    slices, wants = domain
    c_slices, c_wants = collapse
    if how == "batch":
        hooks(k1_path=2)
        with avr.Batch(0, len(c_slices), sum(len(s) for s in c_slices) + 8) as b:
            first = run_batch(avr, slices, False, b)
            check(first[0], first[1], wants, "first run")
            b.reset()
            middle = run_batch(avr, c_slices, False, b)
            check(middle[0], middle[1], c_wants, "the collapse batch in between")
            b.reset()
            third = run_batch(avr, slices, False, b)
        assert third == first
        return
    w, wc = workload(avr, slices), workload(avr, c_slices)
    plans = [x._chunk_plan() for x in (w, wc)]
    need = [avr.lib().avr_range_chunked_workspace_bytes(x.n_slices, ctypes.byref(plans[k]["plan"]), int(x.out_off[-1].item())) for k, x in enumerate((w, wc))]
    assert need[1] > need[0]
    shared = torch.empty(need[1] + 256, dtype=torch.uint8, device=w.out.device)
    for p in plans:
        p["ws_k2"], p["ws_k2_bytes"] = shared, need[1]
    w.encode_chunked()
    first = check_workload(w, wants, "first run")
    wc.encode_chunked()
    check_workload(wc, c_wants, "the collapse batch in between")
    clear(w)
    w.encode_chunked()
    assert check_workload(w, wants, "third run") == first


# ------------------------------------------------------------------ the collapse batch

@pytest.mark.parametrize("seg_len,pass1", K2P, ids=K2P_IDS)
def test_k2p_collapse(avr, collapse, hooks, seg_len, pass1):
    assert avr.SLICE_ZERO_PROB == rd.ZERO_PROB               # the library's status and the oracle's are the same number
    k2p_hooks(hooks, seg_len, pass1)
    slices, wants = collapse
    w = workload(avr, slices)
    w.encode_chunked()
    check_workload(w, wants, f"seg_len {seg_len} pass1 {pass1}")


@pytest.mark.parametrize("path", BATCH_PATHS)
def test_batch_api_collapse(avr, collapse, hooks, path):
    hooks(k1_path=BATCH_PATHS[path])
    slices, wants = collapse
    got, status, _ = run_batch(avr, slices, verify=False)
    check(got, status, wants, path)
