"""The de-interleave of a multi-device frame on the host: tools/untile_host_check.cpp compiles csrc/crt_untile.h -- the index arithmetic
and k_untile_planes, as they are -- behind tools/host_device.h and runs it against a plain restatement of the tile layout: blocks whose
every word says (rank, slot, plane, component), destinations with guard bytes, widths and heights 1 .. 17 with 1 .. 5 ranks, every
element size, plane tables with gaps.  Plain and sanitised, as a stand-alone program with its own main.  CPU only."""
import pytest

import host_program as HP

SUMMARY = "3565 cases, 0 failures"


@pytest.fixture(scope="module")
def host_check_run(tmp_path_factory):
    """both builds of tools/untile_host_check.cpp, each run as `program - out`: [(status, bytes, printed) plain, sanitised]"""
    return HP.run_both_forms("untile_host_check.cpp", str(tmp_path_factory.mktemp("untile_host")), "-")


def test_kernel_text_on_the_host_passes_its_checks(host_check_run):
    """every destination element is the restated one, no guard byte and no plane outside the table is touched; the summary line carries
    the case count, so the case list cannot shrink unnoticed"""
    rc, raw, printed = host_check_run[0]
    assert rc == 0, printed
    assert printed.splitlines()[-1] == SUMMARY, printed
    assert len(raw) == 8


def test_kernel_text_is_clean_under_the_sanitizers(host_check_run):
    """the same program built with -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all (nothing is preloaded):
    exit status 0, the same summary and the same digest of the destination bytes -- no index outside the blocks (exactly their size) or
    the planes, no misaligned word access"""
    rc, raw, printed = host_check_run[1]
    assert rc == 0, printed
    assert printed.splitlines()[-1] == SUMMARY, printed
    assert raw == host_check_run[0][1]
