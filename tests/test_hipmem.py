"""cudaraytracing_amd/hipmem.py without a GPU: its runtime is the one libcrt.so calls also when torch's bundled HIP runtime is mapped
beside it and comes first in the process map, and a DeviceBuffers whose construction fails holds nothing."""
import json
import os
import subprocess
import sys

import pytest

from cudaraytracing_amd import hipmem
import util

# Run in a fresh process, which initialises no device: it only loads libraries and looks symbols up.
CHILD = r'''
import ctypes as C
import json
import sys

from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd import hipmem


def mapped():
    """the HIP runtimes mapped into this process, in the order of the map"""
    paths = []
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line and line.split()[-1] not in paths:
                paths.append(line.split()[-1])
    return paths


class DlInfo(C.Structure):
    _fields_ = [("dli_fname", C.c_char_p), ("dli_fbase", C.c_void_p), ("dli_sname", C.c_char_p), ("dli_saddr", C.c_void_p)]


capi.lib()
out = {"before": mapped()}
try:
    import torch  # noqa: F401
except ImportError:
    out["torch"] = False
else:
    out["torch"] = True
    out["after"] = mapped()
    libc = C.CDLL(None)
    libc.dladdr.argtypes = [C.c_void_p, C.POINTER(DlInfo)]
    info = DlInfo()
    assert libc.dladdr(C.cast(hipmem.runtime().hipMalloc, C.c_void_p), C.byref(info)) != 0
    out["hipMalloc"] = info.dli_fname.decode()
print(json.dumps(out))
'''


def test_runtime_is_the_librarys_own_with_torchs_runtime_mapped_first():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([util.ROOT] + os.environ.get("PYTHONPATH", "").split(os.pathsep)).rstrip(os.pathsep))
    flags = ["-s"] if sys.flags.no_user_site else []
    p = subprocess.run([sys.executable] + flags + ["-c", CHILD], capture_output=True, text=True, cwd=util.ROOT, env=env, timeout=600)
    assert p.returncode == 0, p.stderr
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(out)
    assert len(out["before"]) == 1, out            # libcrt.so alone: the runtime it is linked against
    if not out["torch"]:
        pytest.skip("torch is not installed")
    if len(out["after"]) < 2:
        pytest.skip("torch bundles no HIP runtime of its own: importing it mapped no second one")
    assert os.path.realpath(out["hipMalloc"]) == os.path.realpath(out["before"][0]), out


def test_failed_construction_releases_what_it_made():
    """The second buffer cannot be had with or without a device (2^60 bytes); without one the first cannot either."""
    d = hipmem.DeviceBuffers.__new__(hipmem.DeviceBuffers)
    with pytest.raises(hipmem.HipError) as e:
        d.__init__({"small": 64, "huge": 1 << 60}, stream=True)
    assert e.value.call == "hipMalloc" and e.value.status != 0 and "hipMalloc" in str(e.value) and str(e.value.status) in str(e.value)
    assert d.ptrs == {} and d.stream is None
