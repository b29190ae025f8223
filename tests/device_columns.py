"""Shared by the GPU tests of fa_decode_device: the 15 ctx-owned device columns and `status`, copied to the host."""
import ctypes as C

import numpy as np

COLUMNS = (("time_received", np.uint64, 1), ("time_flow_start", np.uint64, 1), ("sampling_rate", np.uint64, 1),
           ("bytes", np.uint64, 1), ("packets", np.uint64, 1), ("sequence_num", np.uint32, 1), ("src_as", np.uint32, 1),
           ("dst_as", np.uint32, 1), ("etype", np.uint32, 1), ("proto", np.uint32, 1), ("src_port", np.uint32, 1),
           ("dst_port", np.uint32, 1), ("sampler_address", np.uint8, 16), ("src_addr", np.uint8, 16), ("dst_addr", np.uint8, 16),
           ("status", np.uint8, 1))


def fetch_columns(cols, k):
    """The first k rows of a `Columns` result of FlowAgg.decode_device -> {name: array}."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = {}
    for name, dt, w in COLUMNS:
        a = np.zeros((k, w) if w > 1 else k, dtype=dt)
        assert hip.hipMemcpy(a.ctypes.data, getattr(cols, name), a.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        out[name] = a
    return out
