"""GPU: key records (AVR_KIND_RANGE_KEYS) -- the compress direction's estimators resolved on the device -- against the plain
restatement of the update rule in tests/range_keys.py and the oracle's range coder.  Every comparison is exact: records with their
padding, bytes, lengths, statuses, estimator tables."""
import time

import numpy as np
import pytest

import range_keys as rk

pytestmark = pytest.mark.gpu

FILL = 0xABCD


@pytest.fixture(scope="module", autouse=True)
def report_time(request):
    t0 = time.time()
    yield
    with request.config.pluginmanager.getplugin("capturemanager").global_and_fixture_disabled():
        print(f"\ntests/test_gpu_range_keys.py: {time.time() - t0:.1f} s")


def device_resolve(avr, slices, group_first, tables=None, gap=0):
    """avr_range_resolve_device on a recs_out preset to FILL: (recs_out, status, est_out, rec_off, n_bins)."""
    import torch
    w = avr.DeviceWorkload.from_host_keys(slices, group_first, tables, 0, gap)
    w.rec_flat.fill_(np.array(FILL, np.uint16).view(np.int16).item())
    w.est_out.fill_(0xCC)
    w.resolve_keys()
    torch.cuda.synchronize()
    return (w.rec_flat.cpu().numpy().view(np.uint16), w.status.cpu().numpy(), w.est_out.cpu().numpy().reshape(-1, rk.N_KEYS, 2),
            w.rec_off.cpu().numpy(), w.n_bins.cpu().numpy())


def check_device(avr, slices, group_first, tables=None, gap=0):
    want, want_tabs = rk.resolve(slices, group_first, tables)
    out, status, est_out, rec_off, n_bins = device_resolve(avr, slices, group_first, tables, gap)
    exp, mask = rk.expected_layout(want, rec_off, n_bins, FILL)
    diff = np.flatnonzero((out != exp) & mask)
    assert diff.size == 0, f"first difference at record {diff[0]}: {out[diff[0]]:#x} != {exp[diff[0]]:#x} ({diff.size} in all)"
    assert status.tolist() == [rk.BAD_RECORD if w is None else 0 for w in want]
    for g, t in enumerate(want_tabs):
        if t is not None:
            assert np.array_equal(est_out[g], t), f"table of group {g}"
    return est_out


def test_many_short_slices_each_its_own_group(avr):
    rng = np.random.default_rng(8101)
    slices = [rk.random_keys(rng, int(rng.integers(0, 1500)), "skew") for _ in range(700)]
    check_device(avr, slices, list(range(701)))
    check_device(avr, slices, list(range(701)), [rk.random_table(rng) for _ in range(700)], gap=1)


def test_few_long_slices_in_one_group(avr):
    rng = np.random.default_rng(8102)
    slices = [rk.random_keys(rng, int(rng.integers(60000, 120000)), "skew") for _ in range(5)]
    check_device(avr, slices, [0, 5])
    check_device(avr, slices, [0, 5], [rk.random_table(rng)])
    one = [rk.random_keys(rng, 70000, "one") for _ in range(3)]                   # every bin on one key: rows of hundreds of halvings
    check_device(avr, one, [0, 3], [rk.random_table(rng)])


def test_mixed_groups_gaps_and_empty_slices(avr):
    rng = np.random.default_rng(8103)
    lens = [0, 5, 20000, 0, 0, 33000, 1024, 1023, 1025, 16384, 16 * 1024 + 1, 7, 0, 40000, 300, 0]
    slices = [rk.random_keys(rng, n, "skew" if i % 3 else "flat") for i, n in enumerate(lens)]
    for gf in ([0, 1, 4, 5, 9, 10, 16], [0, 16], list(range(17)), [0, 3, 3, 12, 16]):
        for gap in (0, 3):
            tables = None if gap else [rk.random_table(rng) for _ in range(len(gf) - 1)]
            check_device(avr, slices, gf, tables, gap)


def test_chaining_est_out_into_est_in(avr):
    rng = np.random.default_rng(8104)
    slices = [rk.random_keys(rng, int(rng.integers(100, 50000)), "skew") for _ in range(8)]
    start = rk.random_table(rng)
    whole = check_device(avr, slices, [0, 8], [start])
    first = check_device(avr, slices[:3], [0, 3], [start])
    second = check_device(avr, slices[3:], [0, 5], [first[0]])
    assert np.array_equal(second[0], whole[0])
    want, _ = rk.resolve(slices, [0, 8], [start])
    out, _, _, rec_off, n_bins = device_resolve(avr, slices[3:], [0, 5], [first[0]])
    for i in range(5):
        assert np.array_equal(out[int(rec_off[i]):int(rec_off[i]) + int(n_bins[i])], want[3 + i])


# ------------------------------------------------------------------ the batch API

SHAPES = {"lanes": [(300, 0, 4000)], "k2p": [(6, 20000, 60000)]}             # (slices, shortest, longest): either side of the batch API's rule


def shape_slices(rng, path):
    (n, lo, hi), = SHAPES[path]
    slices = [rk.random_keys(rng, int(rng.integers(lo, hi)), "skew") for _ in range(n)]
    if path == "lanes":
        slices[5] = slices[5][:0]
    return slices


def run_keys(avr, slices, group_first, tables=None):
    with avr.Batch(0, len(slices), sum(len(s) for s in slices) + 8) as b:
        g = 0
        for i, s in enumerate(slices):
            while g < len(group_first) - 1 and group_first[g] == i:
                assert b.begin_group(None if tables is None else tables[g]) == g
                g += 1
            assert b.add_slice_range_keys(s) == i
        b.submit()
        b.wait()
        res = [b.get(i) for i in range(len(slices))]
        return res, b.run_info()["chunked"], [b.get_estimators(k) for k in range(len(group_first) - 1)], b.timings()


def run_range(avr, recs):
    with avr.Batch(0, len(recs), sum(len(s) for s in recs) + 8) as b:
        for r in recs:
            b.add_slice_range(r)
        b.run()
        return [b.get(i) for i in range(len(recs))]


@pytest.mark.parametrize("path", ["lanes", "k2p"])
def test_batch_of_key_records_equals_the_oracle_on_both_k2_paths(avr, oracle, path):
    rng = np.random.default_rng(8200 + len(path))
    slices = shape_slices(rng, path)
    n = len(slices)
    for gf in (list(range(n + 1)), [0, n], [0, n // 3, n // 2, n]):
        tables = [rk.random_table(rng) for _ in range(len(gf) - 1)] if len(gf) == 4 else None
        want, want_tabs = rk.resolve(slices, gf, tables)
        got, chunked, tabs, _ = run_keys(avr, slices, gf, tables)
        assert chunked == (path == "k2p")                          # the path this shape is meant to take did run
        for i in range(n):
            assert got[i] == oracle.range_encode(want[i]), f"slice {i} of {n}, groups {gf[:4]}..."
        for g in range(len(gf) - 1):
            assert np.array_equal(tabs[g], want_tabs[g])
        assert got == run_range(avr, want)                         # ... and the bytes of an AVR_KIND_RANGE batch fed the restated records


@pytest.mark.parametrize("path", ["lanes", "k2p"])
def test_group_split_across_two_batches(avr, oracle, path):
    rng = np.random.default_rng(8300 + len(path))
    slices = shape_slices(rng, path)
    n, cut = len(slices), len(slices) // 2
    start = rk.random_table(rng)
    whole, _, whole_tabs, _ = run_keys(avr, slices, [0, n], [start])
    first, _, first_tabs, _ = run_keys(avr, slices[:cut], [0, cut], [start])
    second, _, second_tabs, _ = run_keys(avr, slices[cut:], [0, n - cut], [first_tabs[0]])
    assert first + second == whole
    assert np.array_equal(second_tabs[0], whole_tabs[0])
    want, want_tabs = rk.resolve(slices, [0, n], [start])
    assert np.array_equal(whole_tabs[0], want_tabs[0])
    assert whole == [oracle.range_encode(w) for w in want]


@pytest.mark.parametrize("path", ["lanes", "k2p"])
def test_malformed_record_ends_its_group_and_nothing_else(avr, oracle, path):
    rng = np.random.default_rng(8400 + len(path))
    slices = shape_slices(rng, path)
    n = len(slices)
    gf = [0, n // 3, n // 3 * 2, n] if path == "lanes" else [0, 2, 5, 6]
    clean, chunked, _, _ = run_keys(avr, slices, gf)
    assert chunked == (path == "k2p")
    k = gf[1] + 1                                                  # the second slice of the second group
    for bad in (0x1000, 0x8001, 1026 << 1, (2047 << 1) | 1):
        s = [x.copy() for x in slices]
        assert s[k].size
        s[k][int(rng.integers(0, s[k].size))] = bad
        got, chunked, _, _ = run_keys(avr, s, gf)
        assert chunked == (path == "k2p")
        for i in range(n):
            if k <= i < gf[2]:
                assert got[i] == (b"", rk.BAD_RECORD), f"slice {i}"
            else:
                assert got[i] == clean[i], f"slice {i}"


def test_batch_refusals(avr):
    rng = np.random.default_rng(8500)
    keys = rk.random_keys(rng, 100, "flat")
    L = avr.lib()
    with avr.Batch(0, 8, 4096) as b:
        for entry in ((0, 1), (1, 0), (0x30, 0x31), (0x60, 1)):
            t = rk.fresh_table()
            t[517] = entry
            with pytest.raises(avr.AvrError, match="start table entry 517"):
                b.begin_group(t)
        t = rk.fresh_table()
        t[3] = (0x5f, 1)                                           # pos + neg = 0x60: the largest valid total
        assert b.begin_group(t) == 0
        b.add_slice_range_keys(keys)
        with pytest.raises(avr.AvrError, match="one kind"):
            b.add_slice_range(np.zeros(4, np.uint16))
        b.submit()
        with pytest.raises(avr.AvrError, match="in flight"):
            b.begin_group()
        with pytest.raises(avr.AvrError, match="in flight"):
            b.add_slice_range_keys(keys)
        b.wait()
        with pytest.raises(avr.AvrError, match="out of range"):
            b.get_estimators(1)
        b.reset()
        b.add_slice_range(np.zeros(0, np.uint16))
        with pytest.raises(avr.AvrError, match="one kind"):
            b.begin_group()
        with pytest.raises(avr.AvrError, match="one kind"):
            b.add_slice_range_keys(keys)
        b.run()
        with pytest.raises(avr.AvrError, match="not a batch of key records"):
            b.get_estimators(0)
        b.reset()
        idx, view = b.reserve(avr.KIND_RANGE_KEYS, keys.size)     # the first slice opens a fresh group by itself
        view[:] = keys
        b.run()
        want, tabs = rk.resolve([keys], [0, 1])
        import oracle_lib
        assert b.get(0) == oracle_lib.load_oracle().range_encode(want[0])
        assert np.array_equal(b.get_estimators(0), tabs[0])


# ------------------------------------------------------------------ real clips: the batch API and the command line

@pytest.mark.parametrize("name", ["realshort.mp4", "cockatoo.mp4"])
def test_real_clips_through_the_batch_api(avr, oracle, name):
    """The clip's K1 records (residual hooks off) as key records, one group: per-slice bytes equal the oracle's coding of the K2
    records the host recorder makes with its own estimators."""
    from test_h264 import CLIPS, _stream_records, clip
    from test_host import host as host_fixture
    host = host_fixture.__wrapped__(avr)
    data = open(clip(name), "rb").read()
    k2, payloads, offered = _stream_records(host, data, 0, 0)
    want = [oracle.range_encode(r) for r in k2]
    assert len(want) == CLIPS[name][0] and all(st == 0 for _, st in want)
    k1, _ = _stream_records(host, data, 0, 1, [c for c, _ in want], offered)
    got, _, _, _ = run_keys(avr, k1, [0, len(k1)])
    for i in range(len(k1)):
        assert got[i] == want[i], f"{name} slice {i}"


@pytest.fixture(scope="module")
def recode(avr):
    return avr.build_recode()


@pytest.mark.parametrize("name", ["realshort.mp4", "cockatoo.mp4"])
def test_cli_compress_is_byte_identical_with_device_estimators(recode, tmp_path, name):
    import os
    import subprocess
    from test_h264 import clip
    files = {}
    for on in ("0", "1"):
        out = tmp_path / f"{name}.{on}.recode"
        run = subprocess.run([recode, "compress", clip(name), str(out)], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, AVR_DEVICE_ESTIMATORS=on))
        assert run.returncode == 0, run.stderr
        files[on] = out.read_bytes()
    assert files["0"] == files["1"] and len(files["0"]) > 0
    env = dict(os.environ, AVR_DEVICE_ESTIMATORS="1")
    rt = subprocess.run([recode, "roundtrip", clip(name), str(tmp_path / "rt.recode")], capture_output=True, text=True, timeout=600, env=env)
    assert rt.returncode == 0 and "Compress-decompress roundtrip succeeded:" in rt.stderr, rt.stderr
    assert (tmp_path / "rt.recode").read_bytes() == files["0"]
    # with the residual hooks on the variable has no effect, and the command says so once
    both = subprocess.run([recode, "compress", clip(name), str(tmp_path / "hooks1.recode")], capture_output=True, text=True, timeout=600,
                          env=dict(env, AVR_MODEL_HOOKS="1"))
    hooks = subprocess.run([recode, "compress", clip(name), str(tmp_path / "hooks0.recode")], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, AVR_MODEL_HOOKS="1"))
    assert both.returncode == 0 and hooks.returncode == 0
    assert both.stderr.count("AVR_DEVICE_ESTIMATORS has no effect") == 1 and "AVR_DEVICE_ESTIMATORS" not in hooks.stderr
    assert (tmp_path / "hooks1.recode").read_bytes() == (tmp_path / "hooks0.recode").read_bytes()


def test_cli_test_directory_is_identical_with_device_estimators(recode, tmp_path):
    """`recode test <dir>` over the directory of test_recode_test_directory_batches_across_files (16 copies of each clip): the same
    output files with AVR_DEVICE_ESTIMATORS=1 -- every file a group of its own in the batch of all files' slices -- as without."""
    import os
    import shutil
    import subprocess
    from test_h264 import CLIPS, clip
    a, b = tmp_path / "host", tmp_path / "device"
    for d in (a, b):
        d.mkdir()
        for k in range(16):
            for name in CLIPS:
                shutil.copy(clip(name), d / f"{k:02d}_{name}")
    for d, on in ((a, "0"), (b, "1")):
        out = subprocess.run([recode, "test", str(d)], capture_output=True, text=True, timeout=1800, env=dict(os.environ, AVR_DEVICE_ESTIMATORS=on))
        assert out.returncode == 0 and "failed on" not in out.stdout, out.stderr + out.stdout
    names = sorted(p.name for p in a.iterdir() if p.is_file())
    assert len(names) == 16 * len(CLIPS)
    for name in names:
        got, want = (b / "output" / name).read_bytes(), (a / "output" / name).read_bytes()
        assert got == want and len(got) > 0, name
    assert (b / "output" / "log.txt").read_text().count("Compress-decompress roundtrip succeeded:") == len(names)
