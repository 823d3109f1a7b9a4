"""avr_last_error() "gives the message for the calling thread" (include/avrecode_ms_amd.h, Threading): four host threads provoke four
different refusals at the same moment -- the argument checks tests/test_cabi.py provokes, which run before anything touches a device
-- and each reads its own message behind a barrier, while a fifth thread, which has provoked nothing, reads the empty string.  ctypes
releases the interpreter lock around every call, so the calls do run side by side.

That this can fail was shown once on a build with `thread_local` taken off the message buffer (csrc/avr_api.cpp): every thread then
reads the message of whichever call came last, and the quiet thread reads it too."""
import ctypes
import threading

ROUNDS = 200
TIMEOUT = 60.0


def refusals(avr):
    """[(call, the message it must leave)]: four refusals with four texts; the last one names a number of the caller's choosing."""
    L = avr.lib()
    parts = (avr.ChunkedPart * 2)()
    counts = (ctypes.c_uint32 * 4)()
    keep = (parts, counts)

    def no_parts(k):
        return L.avr_cabac_encode_chunked_device_parts(0, None, None, 64, None, None, 1), "1 .. %d parts" % avr.MAX_PARTS

    def part_without_counts(k):
        return L.avr_cabac_encode_chunked_device_parts(0, None, None, 64, None, ctypes.cast(keep[0], ctypes.c_void_p), 2), "part 0: null counts"

    def null_arrays(k):
        return L.avr_cabac_encode_chunked_device_hinted(0, None, None, None, None, 3, None, 64, None, None, 0, None, None, None, None, None, 0,
                                                        ctypes.cast(keep[1], ctypes.c_void_p)), "null device pointer"

    def too_many_states(k):                                      # no slice: the check of n_states is the first that fails
        n = 2000 + k
        return L.avr_cabac_encode_chunked_device(0, None, None, None, None, 0, None, n, None, None, 0, None, None, None, None, None), "n_states %d > 1024" % n
    return [no_parts, part_without_counts, null_arrays, too_many_states]


def test_each_thread_reads_its_own_message(avr):
    L = avr.lib()
    calls = refusals(avr)
    n = len(calls)
    barrier = threading.Barrier(n + 1, timeout=TIMEOUT)
    wrong, errors = [], []

    def provoke(t):
        try:
            for k in range(ROUNDS):
                barrier.wait()
                rc, want = calls[t](k)
                barrier.wait()                                   # every message is written; none is read yet
                got = L.avr_last_error().decode()
                if rc >= 0 or got != want:
                    wrong.append((t, k, rc, got, want))
                barrier.wait()
        except Exception as exc:                                 # (a broken barrier included)
            errors.append(exc)
            barrier.abort()

    def quiet():
        try:
            for k in range(ROUNDS):
                barrier.wait()
                barrier.wait()
                got = L.avr_last_error().decode()
                if got != "":
                    wrong.append(("quiet", k, 0, got, ""))
                barrier.wait()
        except Exception as exc:
            errors.append(exc)
            barrier.abort()

    threads = [threading.Thread(target=provoke, args=(t,)) for t in range(n)] + [threading.Thread(target=quiet)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(TIMEOUT)
    assert not any(th.is_alive() for th in threads)
    assert not errors, errors[:3]
    assert not wrong, "%d of %d reads gave another thread's message, the first (thread, round, rc, got, want): %r" % (len(wrong), (n + 1) * ROUNDS, wrong[:4])
    assert len({calls[t](0)[1] for t in range(n)}) == n          # four different texts
