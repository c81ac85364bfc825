"""Raw device memory and a stream on the HIP runtime libcrt.so itself calls: an aid for the tests and the probes of the *_device forms, not
part of the rendering API (api.py does not use it)."""
import ctypes as C
import functools

import numpy as np

from . import _capi as capi

H2D, D2H = 1, 2   # hipMemcpyHostToDevice, hipMemcpyDeviceToHost


class HipError(RuntimeError):
    def __init__(self, call, status):
        super().__init__("%s failed with HIP status %d" % (call, status))
        self.call, self.status = call, status


@functools.lru_cache(maxsize=None)
def runtime():
    """The HIP runtime libcrt.so is linked against, through ctypes; made once per process.

    The entry points are looked up on the library's own handle: a symbol looked up on a library's handle is searched in that library and
    in what it depends on, so hipMalloc and hipStreamCreate are the ones libcrt.so calls, whatever else is mapped.  Taking a libamdhip64
    from the process map instead is wrong as soon as there are two: torch bundles a HIP runtime of its own, and once torch has been
    imported after libcrt.so was loaded both are mapped (distributed.py: _check_single_hip_runtime) and torch's comes first.  A stream
    or a device pointer made by that one is a foreign handle to the runtime the library calls, and the process aborts on its use."""
    H = C.CDLL(capi.lib()._name)   # (a second Python object for the handle libcrt.so already has: the argtypes below stay off capi.lib())
    H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    H.hipFree.argtypes = [C.c_void_p]
    H.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    H.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    H.hipStreamSynchronize.argtypes = [C.c_void_p]
    H.hipStreamDestroy.argtypes = [C.c_void_p]
    H.hipDeviceSynchronize.argtypes = []
    return H


def _call(name, *args):
    status = getattr(runtime(), name)(*args)
    if status != 0:
        raise HipError(name, status)


def device_synchronize():
    _call("hipDeviceSynchronize")


class DeviceBuffers:
    """DeviceBuffers({name: nbytes or numpy array}, stream=False): one device buffer per name.  An array's buffer has its size and its
    contents; every other buffer is filled with 0x55, so that a value the tested call fails to write shows.  ptrs: {name: raw device
    pointer}; stream: the handle of a stream of its own as an int, or None (what the *_device wrappers take).  Released by free() or on
    leaving a with block; a HIP call that fails raises HipError."""

    def __init__(self, buffers, stream=False):
        self.ptrs, self.stream, self._nbytes = {}, None, {}
        try:
            for n, b in buffers.items():
                size = b.nbytes if isinstance(b, np.ndarray) else int(b)
                p = C.c_void_p()
                _call("hipMalloc", C.byref(p), size)
                self.ptrs[n], self._nbytes[n] = p.value, size
                if isinstance(b, np.ndarray):
                    self.upload(n, b)
                else:
                    self.fill(n)
            if stream:
                s = C.c_void_p()
                _call("hipStreamCreate", C.byref(s))
                self.stream = s.value
        except BaseException:
            self.free()
            raise

    @classmethod
    def image(cls, table, w, h, stream=True):
        """The buffers of a {name: (channels, dtype)} table (capi.AOV_BUFFERS and its kin) for a w x h image, for fetch()"""
        d = cls({n: w * h * ch * np.dtype(dt).itemsize for n, (ch, dt) in table.items()}, stream=stream)
        d.table, d.w, d.h = table, w, h
        return d

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def free(self):
        H = runtime()
        if self.stream:
            H.hipStreamDestroy(self.stream)
        for p in self.ptrs.values():
            H.hipFree(p)
        self.ptrs, self.stream = {}, None

    def nbytes(self, name):
        return self._nbytes[name]

    def fill(self, name, byte=0x55):
        _call("hipMemset", self.ptrs[name], byte, self._nbytes[name])

    def upload(self, name, a, offset=None):
        """The array a into the buffer: exactly its size, or with an offset (0 included) a part from that byte on"""
        a = np.ascontiguousarray(a)
        assert a.nbytes == self._nbytes[name] if offset is None else offset + a.nbytes <= self._nbytes[name], name
        _call("hipMemcpy", self.ptrs[name] + (offset or 0), a.ctypes.data, a.nbytes, H2D)

    def download(self, name, shape=None, dtype=np.float32, out=None, offset=None):
        """The buffer as a new array of shape and dtype, or into the contiguous array out: exactly its size, or with an offset a part"""
        a = np.zeros(shape, dtype=dtype) if out is None else out
        assert a.flags.c_contiguous and (a.nbytes == self._nbytes[name] if offset is None else offset + a.nbytes <= self._nbytes[name]), name
        _call("hipMemcpy", a.ctypes.data, self.ptrs[name] + (offset or 0), a.nbytes, D2H)
        return a

    def fetch(self, names):
        """{name: (h, w, 3) or (h, w) array} of buffers of image()"""
        out = {}
        for n in names:
            ch, dt = self.table[n]
            out[n] = self.download(n, (self.h, self.w, ch) if ch == 3 else (self.h, self.w), dt)
        return out

    def synchronize(self):
        """Waits for the stream; without one, for the null stream"""
        _call("hipStreamSynchronize", self.stream)
