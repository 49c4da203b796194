"""The rule of lv_tsdf_ray.hpp (the cell states, the walk that reads them through the packed volume, the depth, the normal, the
colour: what the kernels of lv_tsdf_ray.hip run) compiled with g++ and -fsanitize=address,undefined through
tests/emu/hip/hip_runtime.h and held to tests/tsdf_ray_ref.py: tests/emu/tsdf_ray_emu.cpp loads a volume and a layer, casts the
given rays and views, by the packed states and by S and W directly.  Equality on every field, normal bit and colour byte."""
import os
import subprocess

import numpy as np
import pytest

import tsdf_cases as tc
import tsdf_ray_cases as cases
import tsdf_ray_ref as trr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
F = np.float32


def _bits(values):
    return " ".join(str(int(v)) for v in np.asarray(values, F).reshape(-1).view(np.uint32))


def _ints(values):
    return " ".join(str(int(v)) for v in np.asarray(values).reshape(-1))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tsdf_ray_host") / "tsdf_ray_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "tsdf_ray_emu.cpp"), "-o",
                           str(exe)])

    def run(prm, S, W, layer, jobs):
        """jobs: ("R", min_weight, from, to) or ("V", min_weight, views); returns per job (results, normals, rgba[, stats])."""
        head = " ".join([_bits(prm["origin"]), _bits([prm["resolution"]]), str(prm["nx"]), str(prm["ny"]), str(prm["nz"]),
                         _bits([prm["min_range"], prm["max_range"]]), str(prm["trunc_cells"]), str(prm["max_weight"]), str(prm["carve"])])
        lines = [head, _ints(S), _ints(W), "0" if layer is None else "1 " + _ints(layer)]
        for job in jobs:
            if job[0] == "R":
                frm, to = (np.asarray(a, F).reshape(-1, 3) for a in job[2:])
                lines.append(f"R {int(job[1])} {len(frm)} " + _bits(np.hstack([frm, to])))
            else:
                lines.append(f"V {int(job[1])} {len(job[2])}")
                for R, t, pts in job[2]:
                    pts = np.asarray(pts, F).reshape(-1, 3)
                    lines.append(" ".join([_bits(R), _bits(t), str(len(pts)), _bits(pts)]))
        out = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
        assert out[0] == "params ok", out[0]
        got, at = [], 1
        for job in jobs:
            n = len(job[2]) if job[0] == "R" else sum(len(np.asarray(v[2]).reshape(-1, 3)) for v in job[2])
            rows = np.array([r.split() for r in out[at:at + n]], np.int64).reshape(n, 12)
            at += n
            res = np.zeros(n, trr.RESULT_DTYPE)
            for c, f in enumerate(trr.RESULT_FIELDS):
                res[f] = rows[:, c]
            nrm = rows[:, 8:11].astype(np.uint32).view(F)
            rgba = np.ascontiguousarray(rows[:, 11].astype(np.uint32)).view(np.uint8).reshape(n, 4)
            if job[0] == "R":
                got.append((res, nrm, rgba))
            else:
                got.append((res, nrm, rgba, np.array(out[at].split(), np.uint64)))
                at += 1
        assert out[at:] == [""]
        return got

    return run


def _same(got, want, what):
    for f in trr.RESULT_FIELDS:
        assert np.array_equal(got[0][f], want[0][f]), (what, f, np.nonzero(got[0][f] != want[0][f])[0][:8])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, "normals")
    assert np.array_equal(got[2], want[2]), (what, "rgba")


@pytest.mark.parametrize("name", [c["name"] for c in cases.cases()])
def test_rays_of_every_case(emu, name):
    c = cases.case(name)
    frm, to, _ = cases.all_rays(c)
    got = emu(c["prm"], c["S"], c["W"], c["layer"], [("R", mw, frm, to) for mw in c["min_weights"]])
    for res, mw in zip(got, c["min_weights"]):
        _same(res, cases.all_answers(c, mw), (name, mw))


def test_without_a_layer_every_colour_is_zero(emu):
    c = cases.case("dense-21x4x3")
    frm, to, _ = cases.all_rays(c)
    (got,) = emu(c["prm"], c["S"], c["W"], None, [("R", 1, frm, to)])
    _same(got, cases.all_answers(c, 1, coloured=False), "no layer")
    assert not got[2].any() and cases.all_answers(c, 1)[2].any()


def test_views_are_the_rays_they_imply(emu):
    rng = np.random.default_rng(11)
    c = cases.case("33x17x9-carve1-3views")
    prm = c["prm"]
    views = [tc.random_view(rng, tc.INSIDE, 600), tc.random_view(rng, tc.OUTSIDE, 600), (tc.ID, np.array([np.nan, 0, 0], F), np.ones((5, 3), F)),
             (tc.ID, np.asarray(tc.INSIDE, F), np.zeros((0, 3), F)), tc.wall_view(tc.INSIDE, 200)]
    (got,) = emu(prm, c["S"], c["W"], c["layer"], [("V", 1, views)])
    want = trr.raycast_views(prm, c["S"], c["W"], views, 1, c["layer"])
    _same(got, want, "views")
    assert np.array_equal(got[3], want[3]) and want[3][0] > 500 and np.all(want[3][1:] > 0)
    assert want[3][0] == np.sum(want[0]["status"] != trr.IGNORED) < len(want[0])   # ignored returns, and the view without evidence
