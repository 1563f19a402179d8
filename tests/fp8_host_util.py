"""The host engine's C view with GPTConfig::weightsFp8 (tests/test_fp8_host.py, tests/test_hip_host_fp8.py)."""
from ctypes import c_char_p, c_int, c_void_p

from host_util import HostEngine


class Fp8Engine(HostEngine):
    """HostEngine through tgxe_create3, which carries the flag beside the dtype"""

    def __init__(self, lib, weights_fp8, model_dir=None, synthetic=None, device="mi355x", backend_lib=None, prefix="tgx_", dtype=1, max_batch=4):
        self.lib = lib
        lib.tgxe_create3.restype = c_void_p
        lib.tgxe_create3.argtypes = [c_char_p, c_char_p, c_char_p, c_char_p, c_char_p, c_int, c_int, c_int, c_char_p, c_int]
        self.h = lib.tgxe_create3((model_dir or "").encode(), (synthetic or "").encode(), device.encode(), (backend_lib or "").encode(), prefix.encode(),
                                  0, dtype, max_batch, None, int(weights_fp8))
