"""A stream's per-slice records through tests/_host_api.so's recorders (t_stream_records): shared by tests/test_h264.py and
tests/test_h264_walker.py."""
import ctypes

import numpy as np

import oracle_lib


def stream_records(host, data, residual, decompress, recoded=None, offered=None):
    P = oracle_lib.ptr
    cap, slice_cap = 16 * len(data) + 4096, 4096
    recs, rec_end = np.zeros(cap, np.uint16), np.zeros(slice_cap, np.uint64)
    n = ctypes.c_uint64(0)
    pay, pay_end = np.zeros(len(data) + 64, np.uint8), np.zeros(slice_cap, np.uint64)
    first, n_states = np.zeros(slice_cap * 1024, np.uint8), np.zeros(slice_cap, np.int32)
    file = np.frombuffer(data, np.uint8).copy()
    if recoded is None:
        blob, off = np.zeros(1, np.uint8), np.zeros(1, np.uint64)
    else:
        blob = np.frombuffer(b"".join(recoded) + b"\0", np.uint8).copy()
        off = np.zeros(len(recoded) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in recoded])
    err = ctypes.create_string_buffer(512)
    flags = np.zeros(slice_cap, np.uint8)
    n_flags = ctypes.c_uint64(0)
    if offered is not None:
        flags[:len(offered)] = offered
        n_flags = ctypes.c_uint64(len(offered))
    rc = host.t_stream_records(P(file), ctypes.c_size_t(len(data)), int(residual), int(decompress), P(blob), P(off), P(recs), ctypes.c_size_t(cap),
                               P(rec_end), ctypes.c_size_t(slice_cap), ctypes.byref(n), P(pay), ctypes.c_size_t(pay.size), P(pay_end), P(first),
                               P(n_states), P(flags), ctypes.c_size_t(slice_cap), ctypes.byref(n_flags), err, ctypes.c_size_t(512))
    assert rc == 0, err.value.decode()
    ends = [0] + [int(e) for e in rec_end[:n.value]]
    slices = [recs[ends[i]:ends[i + 1]] for i in range(n.value)]
    if decompress:
        return slices, [first[1024 * i:1024 * i + int(n_states[i])] for i in range(n.value)]
    pe = [0] + [int(e) for e in pay_end[:n.value]]
    return slices, [pay[pe[i]:pe[i + 1]].tobytes() for i in range(n.value)], flags[:n_flags.value].copy()
