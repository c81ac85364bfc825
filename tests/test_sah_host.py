"""CPU checks of the host SAH builder (csrc/crt_accel.h) where it must agree with the device builder (csrc/crt_accel_build.hip) for the two
trees to be byte-equal (tests/test_accel_device.py): unions over +-0.0 give lo = -0.0 and hi = +0.0 whatever the leaves' order, and a range
with a denormal centroid extent is binned by the saturating sah_bin (split by centroids, not by index).  tools/sah_host_check.cpp."""
import json

import host_program as HP


def test_host_builder_orders_signed_zeros_and_bins_denormal_extents_like_the_device(tmp_path):
    exe = HP.build("sah_host_check.cpp", str(tmp_path / "sah_host_check"), extra=["-pthread"])
    rc, out, _ = HP.run(exe, timeout=300)
    r = json.loads(out.splitlines()[0])
    assert rc == 0 and r["violations"] == 0, r
    assert r["signed_zero_boxes"] == 2 * 2 * 63 and r["denormal_index_splits"] == 0 and r["denormal_nodes"] == 7, r
