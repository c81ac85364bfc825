"""The textured variant of the Cornell-box stand-in (scenes/gen_cornell_box.py --textured, write_textured_variant): the scene albedo
demodulation is measured on (docs/experiments.md, "Albedo demodulation").  Host layer only: no GPU."""
import os
import subprocess
import sys

import numpy as np

import cudaraytracing_amd as crt
import util

sys.path.insert(0, os.path.join(util.ROOT, "scenes"))
import gen_cornell_box  # noqa: E402

F = np.float32


def test_every_wall_cell_takes_its_own_texel(tmp_path):
    """cells 5, blobs at level 1: the loader must give the two triangles of cell (i, j) of each of the five walls the colour of texel
    (i, j) -- kd = ((k + k) + k) / 3 of that texel's k = byte / 255 (Loader.h:89,103) -- and never look at the last column or row."""
    cells = 5
    obj, mtl_dir, n = gen_cornell_box.write_textured_variant(str(tmp_path), cells, detail=(1, 1))
    assert n == 5 * 2 * cells * cells + 2 + 2 * 20 * 4
    x, y, comp, px = crt.image_load(os.path.join(mtl_dir, "walls.png"))
    assert (x, y, comp) == (cells + 1, cells + 1, 3)
    assert px.tobytes() == gen_cornell_box.wall_texels(cells)
    sc = crt.Scene(160, 120)
    sc.add_obj(obj, mtl_dir)
    sc.set_BVH(2)
    tris, mats = sc.triangles(), sc.materials()
    assert len(tris) == n
    kd = mats["kd"][tris["material"]].astype(F)
    want = {}
    for j in range(cells):
        for i in range(cells):
            k = px[j, i].astype(F) / F(255.0)
            key = (((k + k) + k) / F(3.0)).astype(F).tobytes()
            want[key] = want.get(key, 0) + 5 * 2  # five walls, two triangles per cell
    used = px[:cells, :cells].astype(int)  # the texture is there to vary the albedo from cell to cell: no two neighbours alike
    assert (np.abs(used[:, 1:] - used[:, :-1]).max(axis=2) > 0).all() and (np.abs(used[1:] - used[:-1]).max(axis=2) > 0).all()
    got = {}
    for row in kd:
        got[row.tobytes()] = got.get(row.tobytes(), 0) + 1
    shipped = {k: v for k, v in got.items() if k not in want}
    assert {k: got.get(k, 0) for k in want} == want
    assert sum(shipped.values()) == 2 + 2 * 20 * 4 and len(shipped) == 3  # the light and the two blobs keep the shipped materials
    sc.free()


def test_the_switch_writes_the_three_files(tmp_path):
    d = str(tmp_path / "tex")
    out = subprocess.run([sys.executable, os.path.join(util.ROOT, "scenes", "gen_cornell_box.py"), "--textured", d, "--cells", "3"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert sorted(os.listdir(d)) == ["cornell-box.mtl", "cornell-box.obj", "walls.png"]
    mtl = open(os.path.join(d, "cornell-box.mtl")).read()
    shipped = open(os.path.join(util.ROOT, "scenes", "cornell-box", "cornell-box.mtl")).read()
    assert mtl.startswith(shipped.rstrip("\n")) and "map_Kd walls.png" in mtl[len(shipped.rstrip("\n")):]
    assert crt.image_load(os.path.join(d, "walls.png"))[:3] == (4, 4, 3)
