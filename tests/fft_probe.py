"""Loader of the tests' probe of csrc/fft_lds.h (tests/probe/fft_probe.hip -> unet-rir_amd/libunetrir_probe.so, built by
build.build_probe() when missing or older than its sources, as _lib.lib() does for the product) and the host walk's results on the
inputs of tests/fft_lds_ref.py, computed once and shared by tests/test_fft_lds.py and tests/test_fft_lds_gpu.py."""
import ctypes as C
import functools

import numpy as np

import fft_lds_ref as FR

EXPORTS = {
    "fftprobe_host": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_long]),
    "fftprobe_device": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]),
    "fftprobe_table_host": (None, [C.c_void_p]),
    "fftprobe_table_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fftprobe_tab_host": (None, [C.c_void_p]),
}
ORDERS = (0, 1, 2)          # ascending, descending, a fixed shuffle
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        import unet_rir_amd
        build = unet_rir_amd.build
        path = build.build_probe() if build.probe_needs_build() else build.PROBE_LIB
        L = C.CDLL(path)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def host(M, mode, x, order=0, stop=-1):
    """the host walk of complex64 [n, M] -> complex64 [n, M]"""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    assert x.ndim == 2 and x.shape[1] == M
    out = np.full(x.shape, np.nan + 1j * np.nan, dtype=np.complex64)
    err = lib().fftprobe_host(M, mode, order, stop, x.ctypes.data, out.ctypes.data, x.shape[0])
    assert err == 0, err
    return out


def device(M, mode, G, x, out, stop=-1, stream=None):
    """one launch on torch's current stream (or `stream`): x and out are float32 device tensors [n, M, 2]"""
    import torch
    assert x.dtype == torch.float32 and out.dtype == torch.float32 and x.is_contiguous() and out.is_contiguous()
    assert x.shape == out.shape and x.shape[1:] == (M, 2) and x.is_cuda and out.is_cuda
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    err = lib().fftprobe_device(M, mode, G, stop, x.data_ptr(), out.data_ptr(), x.shape[0], s)
    assert err == 0, err
    return out


def table_host():
    """float32 [2, 4096, 2]: fl_w<-1>(t) and fl_w<+1>(t)"""
    out = np.full((2, 4096, 2), np.nan, dtype=np.float32)
    lib().fftprobe_table_host(out.ctypes.data)
    return out


def tab_host():
    """float32 [2048, 2]: fl_tab_host"""
    out = np.full((2048, 2), np.nan, dtype=np.float32)
    lib().fftprobe_tab_host(out.ctypes.data)
    return out


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def host_random(M, mode):
    return _ro(host(M, mode, FR.random_input(M, mode)))


@functools.lru_cache(maxsize=None)
def host_roundtrip(M):
    """mode 3 of the host walk's own mode 2 output, unscaled"""
    return _ro(host(M, 3, host_random(M, 2)))


@functools.lru_cache(maxsize=4)
def host_impulses(M, mode):
    return _ro(host(M, mode, FR.impulse_input(M, mode)))
