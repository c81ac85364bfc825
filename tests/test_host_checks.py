"""The self-checking host programs of tools/ that compile kernel text of csrc/ for the CPU behind tools/host_device.h: each is built
with -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all and run.  A program checks its kernels against plain
restatements on buffers of exactly their size and prints one summary line; here its exit status is 0 and that line is the expected one,
case count included, so a case list cannot shrink unnoticed and a sanitizer report is the failure's message.  CPU only.
(tools/detmath_host_check.cpp and tools/select_host_check.cpp take a job file: tests/test_device_fn.py, tests/test_filter_select.py.)"""
import pytest

import host_program as HP

PROGRAMS = {"nlm": ([], "26 cases, 0 failures"),
            "modulate": ([], "160 cases, 0 failures"),
            "upsample": ([], "171 cases in both forms, 0 failures; the largest tile: 40612 bytes of LDS"),
            "item_order": (["-pthread"], "23 cases, 0 failures"),
            "sample_map": (["-pthread"], "61 cases, 0 failures")}


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_kernel_text_on_the_host_passes_its_checks_under_the_sanitizers(tmp_path, name):
    extra, summary = PROGRAMS[name]
    exe = HP.build(name + "_host_check.cpp", str(tmp_path / (name + "_host_check")), HP.SANITISED, extra)
    rc, out, err = HP.run(exe, timeout=600)
    assert rc == 0, out[-2000:] + err
    assert out.splitlines()[-1] == summary, out[-2000:]
