"""The rule of lv_ray.hpp (the packed states, the two quantisations of a ray's ends, the walk that reads the grid: what the kernels of
lv_ray.hip run) compiled with g++ and -fsanitize=address,undefined through tests/emu/hip/hip_runtime.h and held to
tests/occ_ray_ref.py: tests/emu/occ_ray_emu.cpp loads a grid, casts the given rays and evaluates the given views.  Equality on
every field, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import occ_ray_cases as cases
import occ_ray_ref as orr
import occupancy_ref as ocr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
F = np.float32
PRM = cases.PRM


def _bits(values):
    return " ".join(str(int(v)) for v in np.asarray(values, F).reshape(-1).view(np.uint32))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("occ_ray_host") / "occ_ray_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "occ_ray_emu.cpp"), "-o",
                           str(exe)])

    def run(prm, L, jobs):
        """jobs: ("R", stop_unknown, from, to) or ("G", views); returns one array per job."""
        head = " ".join([_bits(prm["origin"]), _bits([prm["resolution"]]), str(prm["nx"]), str(prm["ny"]), str(prm["nz"]),
                         _bits([prm[k] for k in ("min_range", "max_range", "l_hit", "l_miss", "l_min", "l_max", "l_occ", "l_free")])])
        lines = [head, _bits(L)]
        for job in jobs:
            if job[0] == "R":
                frm, to = (np.asarray(a, F).reshape(-1, 3) for a in job[2:])
                lines.append(f"R {int(job[1])} {len(frm)} " + _bits(np.hstack([frm, to])))
            else:
                lines.append(f"G {len(job[1])}")
                for R, t, pts in job[1]:
                    pts = np.asarray(pts, F).reshape(-1, 3)
                    lines.append(" ".join([_bits(R), _bits(t), str(len(pts)), _bits(pts)]))
        out = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
        assert out[0] == "params ok", out[0]
        got, at = [], 1
        for job in jobs:
            n = len(job[2]) if job[0] == "R" else len(job[1])
            rows = np.array([r.split() for r in out[at:at + n]], np.int64).reshape(n, 8 if job[0] == "R" else 4)
            at += n
            if job[0] == "R":
                res = np.zeros(n, orr.RESULT_DTYPE)
                for c, f in enumerate(orr.RESULT_FIELDS):
                    res[f] = rows[:, c]
                got.append(res)
            else:
                got.append(rows.astype(np.uint64))
        assert out[at:] == [""]
        return got

    return run


def _same(got, want):
    for f in orr.RESULT_FIELDS:
        assert np.array_equal(got[f], want[f]), (f, np.nonzero(got[f] != want[f])[0][:8])


def test_the_reference_walk_visits_the_cells_of_the_occupancy_walk():
    for name, (frm, to) in cases.rays().items():
        ok, qs, qe = orr.ends(PRM, frm, to)
        orr.check_walk(qs[ok], qe[ok])
    rng = np.random.default_rng(2)   # and from one origin, as a view's rays
    orr.check_walk(np.array([5, -300, 77]), rng.integers(-3000, 3000, (200, 3)))


def test_rays_of_every_case_both_stop_rules(emu):
    names = sorted(cases.rays())
    jobs = [("R", su) + cases.rays()[name] for name in names for su in (False, True)]
    got = emu(PRM, cases.grid(), jobs)
    want = cases.ray_answers()
    for res, (name, su) in zip(got, [(name, su) for name in names for su in (False, True)]):
        _same(res, want[(name, su)])
    # what the cases are there for does happen
    for p in range(len(cases.PLACES)):
        a, b = want[(f"random{p}", False)], want[(f"random{p}", True)]
        assert (a["status"] != orr.IGNORED).all() and (b["status"] == orr.STOPPED).sum() >= (a["status"] == orr.STOPPED).sum()
    inside = want[("random0", False)]
    assert (inside["status"] == orr.STOPPED).any() and (inside["status"] == orr.CLEAR).any() and (inside["n_unknown"] > 0).any()
    assert any((want[(f"random{p}", False)]["cell"] == -1).any() for p in range(1, 6))
    assert any(((want[(f"random{p}", False)]["status"] == orr.STOPPED) & (want[(f"random{p}", False)]["steps"] > 3)).any() for p in range(1, 6))
    same = want[("from_is_to", False)]
    assert list(same["status"]) == [1, 2, 1, 1, 1] and list(same["steps"]) == [0] * 5 and list(same["cell"][3:]) == [-1, -1]
    assert list(want[("from_is_to", True)]["status"]) == [1, 2, 2, 1, 1]
    c0 = want[("stop_in_c0", True)]
    assert np.all(c0["status"] == orr.STOPPED) and np.all(c0["steps"] == 0) and np.all(c0["axis"] == -1) and np.all(c0["num"] == 0) and np.all(c0["den"] == 1)
    assert list(want[("stop_in_c0", False)]["steps"][[0, 2]]) == [0, 0]
    ve = want[("stop_in_ve", False)]
    assert (ve["status"][0], ve["steps"][0], ve["axis"][0], ve["n_free"][0], ve["num"][0], ve["den"][0]) == (orr.STOPPED, 9, 0, 9, 8 * 256 + 128, 9 * 256)
    assert ve["cell"][0] == (4 * 13 + 6) * 19 + 11 and ve["status"][1] == orr.CLEAR and ve["n_unknown"][1] == 1 and ve["steps"][1] == 9
    ve = want[("stop_in_ve", True)]
    assert (ve["status"][1], ve["steps"][1], ve["cell"][1], ve["n_free"][1]) == (orr.STOPPED, 9, (4 * 13 + 6) * 19 + 1, 9)
    ig = want[("ignored", False)]
    assert list(ig["status"]) == [0] * 8 + [ig["status"][8]] and ig["status"][8] != 0 and np.all(ig["cell"][:8] == -1)
    assert all(np.all(ig[f][:8] == 0) for f in orr.RESULT_FIELDS if f != "cell")


def test_view_gain_of_every_case(emu):
    views, want = cases.gain_views(), cases.gain_answers()
    for name in sorted(views):
        L, vs = views[name]
        (got,) = emu(PRM, L, [("G", vs)])
        assert np.array_equal(got, want[name]), name
    assert list(want["twice"][0]) == [2, 0, 1, 6]   # the unknown voxel counts once, as do the six free ones of the row (8..14)
    assert list(want["stopped"][0][:3]) == [2, 1, 0]
    assert list(want["ranges"][0][:3]) == [2, 0, 1]           # the cut return is used and runs on through the unknown voxel
    assert np.all(want["no_evidence"][:3] == 0) and want["no_evidence"][3][0] == 2
    assert np.all(want["random"][:, 0] > 300) and np.all(want["random"][:, 1] > 0) and np.all(want["random"][0, 2:] > 50)


def test_word_tails_and_long_rows(emu):
    """x rows that end inside a 16-cell word, one cell wide, and longer than one word; rays along +-x over every word border."""
    rng = np.random.default_rng(9)
    for nx, ny, nz in ((33, 3, 2), (16, 2, 3), (1, 5, 4), (70, 3, 2)):
        prm = ocr.params(origin=(0.0, 0.0, 0.0), resolution=0.5, nx=nx, ny=ny, nz=nz, min_range=0.05, max_range=100.0)
        L = np.array([np.nan, -1.0, 1.0, 0.0], F)[rng.choice(4, size=(nz, ny, nx), p=(0.3, 0.55, 0.05, 0.1))]
        hi = np.array([nx, ny, nz]) * 0.5
        frm = (rng.uniform(-0.2, 1.2, (300, 3)) * hi).astype(F)
        to = (rng.uniform(-0.2, 1.2, (300, 3)) * hi).astype(F)
        frm[:40, 1:] = to[:40, 1:]   # along x
        jobs = [("R", su, frm, to) for su in (False, True)]
        for res, su in zip(emu(prm, L, jobs), (False, True)):
            _same(res, orr.raycast(prm, L, frm, to, su))
