"""The rule of lv_rollout.hpp (the motion model, the pose and footprint tests, one whole sequence, score and best: what the kernel of
lv_rollout.hip runs) compiled with g++ and -fsanitize=address,undefined through tests/emu/hip/hip_runtime.h and held to
tests/rollout_ref.py: tests/emu/occ_rollout_emu.cpp loads a plan and a field and rolls the given batches out.  Equality on every
field and on the bits of every pose, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import rollout_cases as cases
import rollout_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
F = np.float32
RP_FIELDS = ("fp_clear_s2", "w_cost", "w_goal", "w_stop", "min_steps", "goal_mode")


def _bits(values):
    return " ".join(str(int(v)) for v in np.asarray(values, F).reshape(-1).view(np.uint32))


def _ints(values):
    return " ".join(str(int(v)) for v in np.asarray(values).reshape(-1))


def _grid_text(g, key):
    ny, nx = g[key].shape
    return f"{_bits(g['origin'])} {_bits([g['resolution']])} {nx} {ny}"


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("occ_rollout_host") / "occ_rollout_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "occ_rollout_emu.cpp"), "-o",
                           str(exe)])

    def run(plan, field, jobs):
        """jobs: dicts(rp, start, controls, fp); returns per job the reference's dict, or the refusal's text."""
        lines = [_grid_text(plan, "cost"), _ints(plan["cost"]), _ints(plan["P"])]
        lines += ["0"] if field is None else ["1 " + _grid_text(field, "s2"), _ints(field["s2"])]
        for b in jobs:
            rp, u = b["rp"], np.asarray(b["controls"], F)
            fp = np.zeros((0, 2), F) if b["fp"] is None else np.asarray(b["fp"], F)
            lines.append(" ".join(["J", str(rp["T"]), str(rp["Tc"]), _bits([rp["dt"]]), _ints([rp[f] for f in RP_FIELDS]), _bits(b["start"]),
                                   str(len(fp)), _bits(fp), str(len(u)), str(u.size), _bits(u)]))
        out = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
        got, at = [], 0
        for b in jobs:
            head = out[at]
            at += 1
            if head != "check ok":
                got.append(head)
                continue
            K, T = len(b["controls"]), b["rp"]["T"]
            rows = [[int(t) for t in r.split()] for r in out[at:at + K]]
            assert all(len(r) == 9 + 3 * (T + 1) for r in rows)
            at += K
            res = np.zeros(K, rr.RESULT_DTYPE)
            for c, f in enumerate(rr.RESULT_FIELDS):
                res[f] = np.array([r[c] for r in rows], np.int64)
            best = np.array([int(v) for v in out[at].split()], np.int64)
            at += 1
            got.append(dict(results=res, score=np.array([r[8] for r in rows], np.uint64), best=best,
                            poses=np.array([r[9:] for r in rows], np.uint32).view(F).reshape(K, T + 1, 3)))
        assert out[at:] == [""]
        return got

    return run


def same(got, want, name=""):
    for f in rr.RESULT_FIELDS:
        assert np.array_equal(got["results"][f], want["results"][f]), (name, f, np.nonzero(got["results"][f] != want["results"][f])[0][:8])
    assert np.array_equal(got["score"], want["score"]), name
    assert np.array_equal(got["best"], want["best"]), (name, got["best"], want["best"])
    if "poses" in got:
        assert got["poses"].shape == want["poses"].shape and np.array_equal(got["poses"].view(np.uint32), want["poses"].view(np.uint32)), name


def test_every_case_against_the_reference(emu):
    cases.check_the_cases_do_what_they_are_for()
    plan, field = cases.world()
    names = sorted(cases.batches())
    got = emu(plan, field, [cases.batches()[n] for n in names])
    for name, g in zip(names, got):
        assert isinstance(g, dict), (name, g)
        same(g, cases.answers()[name], name)


def test_without_a_field_and_on_another_origin(emu):
    """n_fp = 0 reads no field (the emulator has none to read); a plan whose origin is not the cases'."""
    plan, _ = cases.world()
    moved = dict(plan, origin=(10.0, -20.0, 3.0), resolution=0.5)
    b = cases.random_batch(7, 200, 33, 33, 0)
    b["start"] = np.array([18.6, -14.0, 0.3], F)
    (got,) = emu(moved, None, [b])
    want = rr.rollout(moved, None, b["rp"], b["start"], b["controls"])
    same(got, want)
    assert len(set(want["results"]["why"])) >= 2


def test_the_limits_are_refused_by_the_shared_check(emu):
    plan, field = cases.world()
    good = cases.random_batch(1, 3, 4, 1, 2)
    bad = [("T: 1", dict(T=0)), ("T: 1", dict(T=1025, Tc=1)), ("Tc", dict(Tc=0)), ("Tc", dict(Tc=5)), ("dt", dict(dt=0.0)), ("dt", dict(dt=-1.0)),
           ("dt", dict(dt=np.nan)), ("dt", dict(dt=np.inf)), ("fp_clear_s2", dict(fp_clear_s2=0)), ("fp_clear_s2", dict(fp_clear_s2=3 * 1023 ** 2 + 1)),
           ("min_steps", dict(min_steps=-1)), ("min_steps", dict(min_steps=5)), ("goal_mode", dict(goal_mode=2)), ("goal_mode", dict(goal_mode=-1)),
           ("weights", dict(w_cost=65536)), ("weights", dict(w_goal=65536)), ("weights", dict(w_stop=2 ** 31))]
    jobs = [dict(good, rp=dict(good["rp"], **kw)) for _, kw in bad]
    jobs.append(dict(good, rp=dict(good["rp"], fp_clear_s2=3 * 1023 ** 2, w_cost=65535, w_goal=65535, w_stop=65535, min_steps=4)))
    got = emu(plan, field, jobs)
    for (what, kw), g in zip(bad, got):
        assert isinstance(g, str) and g.startswith("check bad: ") and what in g, (kw, g)
    last = jobs[-1]
    same(got[-1], rr.rollout(plan, field, last["rp"], last["start"], last["controls"], last["fp"]))
