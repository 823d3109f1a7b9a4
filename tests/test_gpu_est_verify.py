"""GPU: the estimator checker (avr_range_keys_verify_device, csrc/avr_est_verify.hip) over the resolver's output -- sound, altered
on the device one record at a time, with a malformed group -- through the device call, the batch API with its test hook, and the
command line.  Every expected answer is tests/est_verify_ref.py's: the five conditions stated plainly, for the whole batch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import est_verify_ref as evr
import guarded
import range_keys as rk

pytestmark = pytest.mark.gpu

NONE, BAD_RECORD, VERIFY_FAILED = evr.VERIFY_NONE, rk.BAD_RECORD, 4
CHUNK, SPAN = 1024, 16


def chunk_base(slices):
    return np.concatenate([[0], np.cumsum([max(1, -(-len(s) // CHUNK)) for s in slices])]).astype(np.int64)


class Resolved:
    """Key records on the device, resolved there; the checker's caller-owned buffers guarded and of exactly the quoted sizes."""

    def __init__(self, avr, slices, gf, tables=None, gap=1):
        import torch
        self.avr, self.slices, self.gf = avr, slices, list(gf)
        self.w = w = avr.DeviceWorkload.from_host_keys(slices, gf, tables, gap=gap)
        self.tables = None if tables is None else np.stack(tables)
        w.status.zero_()
        w.resolve_keys()
        torch.cuda.synchronize()
        dev = w.n_bins.device
        self.status0 = w.status.clone()
        self.keys = w.key_flat.cpu().numpy().view(np.uint16)
        self.recs = w.rec_flat.cpu().numpy().view(np.uint16).copy()
        self.est_out = w.est_out.cpu().numpy().reshape(-1, rk.N_KEYS, 2).copy()
        self.rec_off, self.n_bins = w.rec_off.cpu().numpy(), w.n_bins.cpu().numpy()
        p = w._chunk_plan()
        self.ws_bytes = avr.lib().avr_range_keys_verify_workspace_bytes(w.n_slices, w.n_groups, ctypes.byref(p["plan"]))
        self.g_ws = guarded.Guarded(self.ws_bytes, dev, "ws_estv")
        self.g_fb = guarded.Guarded(4 * w.n_slices, dev, "first_bad")
        self.g_st = guarded.Guarded(4 * w.n_slices, dev, "status")
        self.stream = torch.cuda.Stream()

    def verify(self, recs=None, est_out=None, status=None, poison=0xFF, with_est_out=True):
        """The device call on the caller's own stream: (status list, first_bad list); keys, records and tables must come back untouched."""
        import torch
        w, L = self.w, self.avr.lib()
        dev = w.n_bins.device
        d_recs = w.rec_flat.clone() if recs is None else torch.from_numpy(np.ascontiguousarray(recs).view(np.int16)).to(dev)
        d_eo = w.est_out.clone() if est_out is None else torch.from_numpy(np.ascontiguousarray(est_out, np.uint8).reshape(-1)).to(dev)
        keys0, recs0, eo0 = w.key_flat.clone(), d_recs.clone(), d_eo.clone()
        st = self.g_st.as_dtype(torch.int32)
        st.copy_(self.status0 if status is None else torch.tensor(status, dtype=torch.int32, device=dev))
        if isinstance(poison, int):
            self.g_ws.view.fill_(poison)
        else:
            self.g_ws.view.copy_(torch.from_numpy(np.random.default_rng(poison[1]).integers(0, 256, self.ws_bytes, dtype=np.uint8)).to(dev))
        self.g_fb.view.fill_(0x5A)
        torch.cuda.synchronize()
        p = w._chunk_plan()
        with torch.cuda.stream(self.stream):
            rc = L.avr_range_keys_verify_device(
                0, ctypes.c_void_p(self.stream.cuda_stream), w.key_flat.data_ptr(), d_recs.data_ptr(), w.rec_off.data_ptr(), w.n_bins.data_ptr(),
                w.n_slices, w.group_first.data_ptr(), w.n_groups, w.est_in.data_ptr() if w.est_in is not None else None,
                d_eo.data_ptr() if with_est_out else None, ctypes.byref(p["plan"]), self.g_ws.view.data_ptr(), self.ws_bytes,
                st.data_ptr(), self.g_fb.view.data_ptr())
            assert rc == 0, L.avr_last_error().decode()
            self.stream.synchronize()
        for g in (self.g_ws, self.g_fb, self.g_st):
            g.check()
        assert torch.equal(w.key_flat, keys0) and torch.equal(d_recs, recs0) and torch.equal(d_eo, eo0)
        return st.cpu().numpy().tolist(), self.g_fb.as_dtype(torch.int32).cpu().numpy().view(np.uint32).tolist()

    def expect(self, recs=None, est_out=None, status=None, with_est_out=True):
        status = self.status0.cpu().numpy() if status is None else status
        eo = (self.est_out if est_out is None else est_out) if with_est_out else None
        want = evr.expect(self.keys, self.recs if recs is None else recs, self.rec_off, self.n_bins, self.gf, self.tables, eo, status)
        return want, evr.expect_status(want, status)

    def agree(self, **kw):
        want, want_status = self.expect(**{k: v for k, v in kw.items() if k != "poison"})
        status, first = self.verify(**kw)
        diff = [i for i in range(len(first)) if first[i] != want[i][1]]
        assert not diff, f"slice {diff[0]}: first_bad {first[diff[0]]}, the reference's {want[diff[0]][1]} ({len(diff)} slices differ)"
        assert status == want_status
        return want


# ------------------------------------------------------------------ 1. sound: the resolver's output for a mixed batch

def test_sound_resolver_output_has_no_finding_on_poisoned_exact_buffers(avr):
    rng = np.random.default_rng(7100)
    small = rk.tiny_slices(rng, 9)                                                  # groups inside a span
    over3 = [rk.random_keys(rng, n, "skew") for n in (20000, 17000, 3000)]         # 20 + 17 + 3 chunks from chunk 9 on: spans 0 .. 3
    rows, rows_gf = rk.row_block_case("rows65mid")                                  # a chain of 65 pieces: longer than a block
    emp, emp_gf = rk.empties_case(np.random.default_rng(7101))
    slices = small + over3 + rows + emp
    gf = [0, 4, 9, 12] + [12 + g for g in rows_gf[1:]] + [12 + len(rows) + g for g in emp_gf[1:]]
    tables = [rk.random_table(rng) for _ in range(len(gf) - 1)]
    r = Resolved(avr, slices, gf, tables, gap=1)
    plan = rk.row_plan(slices, gf)
    assert 65 in plan["rows"] and len(plan["rows"]) >= 4                            # the piece chains this batch is here for
    assert not r.status0.any()
    for poison in (0x00, 0xFF, ("random", 7102)):
        want = r.agree(poison=poison)
        assert not any(f for f, _ in want)
    r.agree(with_est_out=False)
    # fresh tables (est_in NULL), through the Python method on a workspace of its own
    import torch
    r2 = Resolved(avr, slices[:30], [0, 4, 9, 12, 30], None, gap=0)
    status, first = r2.w.verify_keys()
    torch.cuda.synchronize()
    assert not status.any() and (first.cpu().numpy().view(np.uint32) == NONE).all()
    want = r2.agree()
    assert not any(f for f, _ in want)


# ------------------------------------------------------------------ 2. single records altered on the device

@pytest.fixture(scope="module")
def altered_case(avr):
    """Group 0: three short slices.  Group 1: 30000 + 20000 + 1500 bins from chunk 4 on (spans 0 .. 3).  Group 2: two short slices.
    Key 1001 occurs in group 1 only in its fourth piece; key 1003 nowhere."""
    rng = np.random.default_rng(7200)
    slices = [rk.random_keys(rng, n, "skew") for n in (700, 0, 1301, 30000, 20000, 1500, 77, 900)]
    for s in slices:
        s[(s >> 1) == 1001] = 1002 << 1
        s[(s >> 1) == 1003] = 1004 << 1
    base = chunk_base(slices)
    late = (3 * SPAN - int(base[4])) * CHUNK + 333                                   # slice 4, inside the span that begins at chunk 48
    assert base[3] < SPAN and base[4] <= 3 * SPAN < base[5] and 0 < late < late + 2000 < 20000
    slices[4][late] = (1001 << 1) | 1
    slices[4][late + 2000] = 1001 << 1
    gf = [0, 3, 6, 8]
    return Resolved(avr, slices, gf, [rk.random_table(rng) for _ in range(3)], gap=1), base, late


def place(r, i, j):
    return int(r.rec_off[i]) + j


def test_single_altered_records_are_found_where_the_reference_says(avr, altered_case):
    r, base, late = altered_case
    assert not any(f for f, _ in r.agree())
    keys = [s >> 1 for s in r.slices]
    # the bin after a halving of the hottest key of slice 3, and the second of two adjacent equal keys inside one step
    hot = int(np.bincount(keys[3]).argmax())
    at = np.flatnonzero(keys[3] == hot)
    rec3 = r.recs[place(r, 3, 0):place(r, 3, 0) + 30000].astype(np.int64)
    tot = ((rec3 >> 1) & 0x7F) + (rec3 >> 8)
    halved = [int(at[k]) for k in range(1, at.size) if tot[at[k]] == 49 and tot[at[k - 1]] == 96]
    twins = [j for j in range(1, 30000) if keys[3][j] == keys[3][j - 1] and j % 64]
    assert halved and twins
    boundary = (SPAN - int(base[3])) * CHUNK                                        # bin 0 of global chunk 16, inside slice 3
    assert 0 < boundary < 30000
    spots = {
        "a group's first bin": (3, 0, 2), "a batch's first bin": (0, 0, 0x100),
        "first bin of a piece that comes in from the left": (3, boundary, 0x100),
        "a key's first bin in a late piece": (4, late, 2),
        "a group's last bin": (5, 1499, 0x100), "the last group's last bin": (7, 899, 2),
        "the bin after a halving": (3, halved[len(halved) // 2], 0x100),
        "the second of two adjacent equal keys": (3, twins[len(twins) // 2], 2),
    }
    for what, (i, j, add) in spots.items():
        recs = r.recs.copy()
        recs[place(r, i, j)] += add
        want = r.agree(recs=recs)
        assert want[i] == (True, j), what
    recs = r.recs.copy()                                                              # a bin bit
    recs[place(r, 4, 7777)] ^= 1
    assert r.agree(recs=recs)[4] == (True, 7777)
    recs = r.recs.copy()                                                              # a padding record (1301 bins: three of them)
    recs[place(r, 2, 1302)] = 0x0101
    assert r.agree(recs=recs)[2] == (True, 1301)
    for g, k, last in ((1, hot, 5), (1, 1003, 5), (0, 1003, 2)):                      # est_out of a met key and of unmet ones
        eo = r.est_out.copy()
        eo[g, k, 1] += 1
        want = r.agree(est_out=eo)
        assert [f for f, _ in want] == [i == last for i in range(8)] and want[last][1] == int(r.n_bins[last])
    # a key's last bin in slice 3 altered: reported there, AND the key's next bin, in slice 4, is held to the altered value
    both = [int(k) for k in np.unique(keys[3]) if (keys[4] == k).any()]
    assert both
    j, nxt = int(np.flatnonzero(keys[3] == both[0])[-1]), int(np.flatnonzero(keys[4] == both[0])[0])
    recs = r.recs.copy()
    recs[place(r, 3, j)] += 2
    want = r.agree(recs=recs)
    assert want[3] == (True, j) and want[4] == (True, nxt)


def test_a_malformed_group_is_checked_up_to_its_bad_slice(avr):
    rng = np.random.default_rng(7300)
    slices = [rk.random_keys(rng, n, "skew") for n in (500, 18000, 9000, 2100, 300, 800)]
    slices[3][1234] = 0x9001                                                          # malformed: slice 3 and slice 4 of group [1, 5)
    gf = [0, 1, 5, 6]
    r = Resolved(avr, slices, gf, [rk.random_table(rng) for _ in range(3)], gap=1)
    assert r.status0.cpu().numpy().tolist() == [0, 0, 0, BAD_RECORD, BAD_RECORD, 0]
    want = r.agree()
    assert not any(f for f, _ in want)
    recs, eo = r.recs.copy(), r.est_out.copy()
    recs[place(r, 2, 8999)] += 2                                                      # found, before the bad slice
    recs[place(r, 3, 10)] ^= 0x7FFE                                                   # not looked at
    eo[1] = 0xCC                                                                      # a wrong table of that group is not reported
    want = r.agree(recs=recs, est_out=eo)
    assert want[2] == (True, 8999) and [f for f, _ in want] == [False, False, True, False, False, False]
    status, first = r.verify(recs=recs, est_out=eo)
    assert status == [0, 0, VERIFY_FAILED, BAD_RECORD, BAD_RECORD, 0] and first[3] == first[4] == NONE


# ------------------------------------------------------------------ 3. the batch API and its hook

def run_batch(avr, keys, gf, verify):
    with avr.Batch(0, len(keys), sum(len(s) for s in keys) + 8) as b:
        if verify is not None:
            b.set_verify(verify)
        for i, s in enumerate(keys):
            if i in gf[:-1]:
                b.begin_group()
            b.add_slice_range_keys(s)
        b.submit()
        b.wait()
        n = range(len(keys))
        return dict(got=[b.get(i) for i in n], chunked=b.run_info()["chunked"], ms=b.verify_ms(), est_ms=b.verify_est_ms(),
                    fb=[b.get_verify(i) for i in n], est=[b.get_verify_est(i) for i in n])


@pytest.mark.parametrize("form", ["keys_lanes", "keys_k2p"])
def test_batch_runs_the_checker_and_the_hook_shows_what_only_it_can_see(avr, oracle, hooks, form):
    from test_gpu_range_verify import batch_case
    keys, recs, gf = batch_case(form)
    n = len(keys)
    want = [oracle.range_encode(r) for r in recs]
    off, on = run_batch(avr, keys, gf, None), run_batch(avr, keys, gf, True)
    assert off["chunked"] == on["chunked"] == int(form == "keys_k2p")
    assert off["got"] == want and on["got"] == want
    assert on["est"] == off["est"] == on["fb"] == [NONE] * n
    assert on["est_ms"] > 0.0 and off["est_ms"] == 0.0 and on["ms"] > 0.0
    # one estimator altered between the resolver and the encode
    k = 78 if form == "keys_lanes" else 4
    while len(keys[k - 1]) < 50:
        k += 1
    m = 37 if form == "keys_lanes" else 12345
    altered = [r.copy() for r in recs]
    altered[k - 1][m] += 0x100
    _, tabs = rk.resolve(keys, gf)
    flat_keys, rec_off, n_bins = rk.layout(keys)
    flat_recs, _ = rk.expected_layout(altered, rec_off, n_bins)
    answer = evr.expect(flat_keys, flat_recs, rec_off, n_bins, gf, None, np.stack(tabs))
    assert answer[k - 1] == (True, m)
    hooks(est_flip=k, est_flip_bin=m)
    run = run_batch(avr, keys, gf, True)
    assert run["fb"] == [NONE] * n                                                    # the decoder is content everywhere: the hole
    assert run["est"] == [f for _, f in answer]
    assert run["est"][k - 1] == m
    for i in range(n):
        data, st = oracle.range_encode(altered[i])                                    # the oracle's coding of the altered records
        assert st == 0
        assert run["got"][i] == (data, VERIFY_FAILED if answer[i][0] else 0), f"slice {i}"
    hooks(est_flip=0)
    run = run_batch(avr, keys, gf, True)
    assert run["got"] == want and run["est"] == [NONE] * n
    hooks(est_flip=k, est_flip_bin=m)                                                 # with verify off the hook is not read
    run = run_batch(avr, keys, gf, False)
    assert run["got"] == want and run["est"] == [NONE] * n and run["est_ms"] == 0.0


def test_batches_of_other_kinds_have_no_checker(avr):
    import oracle_lib
    rng = np.random.default_rng(7400)
    with avr.Batch(0, 4, 1 << 16) as b:
        b.set_verify(True)
        b.add_slice_range(oracle_lib.random_range_stream(rng, 300, adaptive=False))
        b.run()
        assert b.get(0)[1] == 0 and b.get_verify_est(0) == NONE and b.verify_est_ms() == 0.0 and b.verify_ms() > 0.0
        with pytest.raises(avr.AvrError, match="out of range"):
            b.get_verify_est(1)


# ------------------------------------------------------------------ 4. the command line

def test_cli_compress_with_verify_and_device_estimators_reports_the_checker(avr, tmp_path):
    from test_h264 import clip
    recode = avr.build_recode()
    files, err = {}, {}
    for name, env in (("plain", {}), ("verify", {"AVR_VERIFY": "1", "AVR_TIMING": "1"}),
                      ("verify_est", {"AVR_VERIFY": "1", "AVR_DEVICE_ESTIMATORS": "1", "AVR_TIMING": "1"})):
        out = tmp_path / f"{name}.recode"
        run = subprocess.run([recode, "compress", clip("realshort.mp4"), str(out)], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, **env))
        assert run.returncode == 0, run.stderr
        files[name], err[name] = out.read_bytes(), run.stderr
    assert len(files["plain"]) > 0 and files["verify"] == files["plain"] and files["verify_est"] == files["plain"]
    assert "GPU verify estimators" in err["verify_est"] and "GPU verify (a5)" in err["verify_est"]
    assert "GPU verify estimators" not in err["verify"] and "GPU verify estimators" not in err["plain"]
