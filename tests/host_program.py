"""Builds and runs the stand-alone host programs of tools/ (each has its own main; nothing is loaded into Python): the one place in the
test-suite that states the compiler line."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudaraytracing_amd", "csrc")
CXX = "g++"
PLAIN = ["-O2"]
SANITISED = ["-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]


def build(source, exe, mode=PLAIN, extra=()):
    """tools/<source> compiled to `exe` in the plain or the sanitised form; `extra`: further flags (-pthread, -fno-fast-math, -I ..., -l ...)"""
    subprocess.run([CXX, "-std=c++17", "-ffp-contract=off", "-I" + CSRC] + list(mode) + [os.path.join(ROOT, "tools", source)] + list(extra) + ["-o", exe],
                   check=True, cwd=ROOT, timeout=600)
    return exe


def run(exe, args=(), timeout=600, env=None):
    """(exit status, stdout, the tail of stderr) of the program run from the repository root"""
    p = subprocess.run([exe] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
    return p.returncode, p.stdout, p.stderr[-8000:]  # (a sanitizer's report: its first lines say what and where, some 5 000 characters from its end)


def run_both_forms(source, tmp, job):
    """The plain and the sanitised build of tools/<source>, each run as `program job out`: [(exit status, the bytes of out, the tail
    of what it printed)] plain, sanitised"""
    res = []
    for name, mode in (("plain", PLAIN), ("sanitised", SANITISED)):
        exe = build(source, os.path.join(tmp, os.path.splitext(source)[0] + "_" + name), mode)
        outp = os.path.join(tmp, name + ".bin")
        rc, out, err = run(exe, [job, outp])
        res.append((rc, open(outp, "rb").read() if os.path.exists(outp) else b"", (out + err)[-2000:]))
    return res
