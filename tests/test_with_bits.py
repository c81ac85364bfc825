"""CPU property test of crtaccel::with_bits (csrc/crt_accel.h): the nudge that hides nodes4i's child indices in the low 12 mantissa bits of
an inner child's planes (csrc/crt_scene_layout.h).  A nudge in the wrong direction makes a box too small, which the exactness proof does not
allow (crt_accel.h).  tools/with_bits_check.cpp runs every input with all 4 096 chunks, moving down and up: a result that is finite, carries
the chunk, lies on the asked side of the input and is the nearest such value; a give-up exactly when no finite such value exists."""
import json

import host_program as HP


def test_with_bits_is_the_nearest_value_with_the_chunk_on_the_asked_side(tmp_path):
    exe = HP.build("with_bits_check.cpp", str(tmp_path / "with_bits_check"), extra=["-pthread"])
    rc, out, _ = HP.run(exe, ["1000000", "7"], timeout=900)
    r = json.loads(out.splitlines()[0])
    assert rc == 0 and r["violations"] == 0, r
    assert r["calls"] == r["inputs"] * 4096 * 2 and r["inputs"] >= 1000000 + r["special"]
    # every branch was taken: results on both sides of zero, crossings of zero, and give-ups (non-finite inputs, +-FLT_MAX's neighbours)
    assert r["ok"] > 0 and r["crossed_zero"] > 0 and r["gave_up"] > 0, r
