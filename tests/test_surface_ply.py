"""surface.save_ply writes what its header says (no GPU)."""
import numpy as np


def test_save_ply_with_normals_and_colours(lv, tmp_path):
    from limo_velo_amd import surface

    rng = np.random.default_rng(0)
    xyz = rng.standard_normal((50, 3)).astype(np.float32)
    nrm = rng.standard_normal((50, 3)).astype(np.float32)
    rgb = rng.uniform(0, 255, (50, 3))
    for kw, names in ((dict(), "x y z"), (dict(normals=nrm), "x y z nx ny nz"), (dict(normals=nrm, rgb=rgb), "x y z nx ny nz red green blue"),
                      (dict(rgb=rgb), "x y z red green blue")):
        path = tmp_path / "m.ply"
        surface.save_ply(path, xyz, **kw)
        raw = open(path, "rb").read()
        head, body = raw.split(b"end_header\n", 1)
        lines = head.decode().split("\n")
        assert lines[0] == "ply" and "element vertex 50" in lines
        assert " ".join(l.split()[2] for l in lines if l.startswith("property")) == names
        dt = [(l.split()[2], "<f4" if l.split()[1] == "float" else "u1") for l in lines if l.startswith("property")]
        rec = np.frombuffer(body, dtype=dt)
        assert len(rec) == 50 and np.array_equal(rec["x"], xyz[:, 0])
        if "normals" in kw:
            assert np.array_equal(rec["nz"], nrm[:, 2])
        if "rgb" in kw:
            assert np.array_equal(rec["green"], np.rint(rgb[:, 1]).astype(np.uint8))
