"""Device buffers and a stream for the tests of device forms, made by the HIP runtime libcrt.so itself is linked against.

util.hip_runtime() takes the first libamdhip64 in the process map.  torch bundles a HIP runtime of its own, and once an earlier test of
the session has imported torch after libcrt.so was loaded, two runtimes are mapped (cudaraytracing_amd/distributed.py:
_check_single_hip_runtime) and torch's comes first: a stream created by it is a foreign handle to the runtime the library calls.  Here
the runtime is reached through the library's own handle instead: a symbol looked up on a library's handle is searched in that library
and in what it depends on, so hipStreamCreate and hipMalloc are the ones libcrt.so calls, whatever else is mapped.
"""
import ctypes as C

from cudaraytracing_amd import _capi as capi
import util


def hip_runtime():
    H = C.CDLL(capi.lib()._name)   # (a second Python object for the handle libcrt.so already has: the argtypes below stay off capi.lib())
    H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    H.hipFree.argtypes = [C.c_void_p]
    H.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    H.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    H.hipStreamSynchronize.argtypes = [C.c_void_p]
    H.hipStreamDestroy.argtypes = [C.c_void_p]
    return H


class DeviceBuffers(util.DeviceBuffers):
    """util.DeviceBuffers on the library's own runtime"""

    def __init__(self, table, w, h):
        self.H, self.table, self.w, self.h = hip_runtime(), table, w, h
        self.ptrs, self._stream = {}, C.c_void_p()
