"""The rule of lv_mcl.hpp (the limits, a beam's cost, a particle's fold, the key of `best`: what the kernel of lv_mcl.hip runs)
compiled with g++ and -fsanitize=address,undefined through tests/emu/hip/hip_runtime.h and held to tests/mcl_ref.py:
tests/emu/occ_mcl_emu.cpp loads a field and weighs the given batches.  Equality on every score, n_in and best, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import mcl_cases as cases
import mcl_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
F = np.float32


def _bits(values):
    return " ".join(str(int(v)) for v in np.asarray(values, F).reshape(-1).view(np.uint32))


def _ints(values):
    return " ".join(str(int(v)) for v in np.asarray(values).reshape(-1))


def _arr(a, floats):
    a = np.asarray(a)
    return f"{a.size} {_bits(a) if floats else _ints(a)}"


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("occ_mcl_host") / "occ_mcl_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "occ_mcl_emu.cpp"), "-o", str(exe)])

    def run(field, jobs):
        """jobs: dicts(mp, poses, beams, table) and optionally K, B, n_table (declared apart from the arrays); returns per job the
        reference's dict, or the refusal's text."""
        s2 = np.asarray(field["s2"])
        planar = s2.ndim == 2
        nz = 1 if planar else s2.shape[0]
        lines = [f"{int(planar)} {_bits(field['origin'])} {_bits([field['resolution']])} {s2.shape[-1]} {s2.shape[-2]} {nz}", _ints(s2)]
        for b in jobs:
            K, B, nt = b.get("K", len(b["poses"])), b.get("B", len(b["beams"])), b.get("n_table", len(b["table"]))
            lines.append(" ".join(["J", str(b["mp"]["out_cost"]), str(b["mp"]["min_inside"]), str(nt), _arr(b["table"], False), str(B),
                                   _arr(b["beams"], True), str(K), _arr(b["poses"], True)]))
        out = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
        got, at = [], 0
        for b in jobs:
            head = out[at]
            at += 1
            if head != "check ok":
                got.append(head)
                continue
            K = len(b["poses"])
            rows = [[int(t) for t in r.split()] for r in out[at:at + K]]
            assert all(len(r) == 2 for r in rows)
            at += K
            best = np.array([int(v) for v in out[at].split()], np.int64)
            at += 1
            got.append(dict(score=np.array([r[0] for r in rows], np.uint64), n_in=np.array([r[1] for r in rows], np.uint32), best=best))
        assert out[at:] == [""]
        return got

    return run


def same(got, want, name=""):
    assert np.array_equal(got["score"], want["score"]), (name, np.nonzero(got["score"] != want["score"])[0][:8])
    assert np.array_equal(got["n_in"], want["n_in"]), (name, np.nonzero(got["n_in"] != want["n_in"])[0][:8])
    assert np.array_equal(got["best"], want["best"]), (name, got["best"], want["best"])


def test_every_case_against_the_reference(emu):
    cases.check_the_cases_do_what_they_are_for()
    for fname in cases.DPS:
        names = sorted(n for n, b in cases.batches().items() if b["field"] == fname)
        assert names
        got = emu(cases.field(fname), [cases.batches()[n] for n in names])
        for name, g in zip(names, got):
            assert isinstance(g, dict), (name, g)
            same(g, cases.answers()[name], name)


def test_a_field_at_another_origin(emu):
    """The field of the grid recentred by (3, -2, 0) and rebuilt: the same world poses against the shifted contents."""
    for fname in ("planar", "vol"):
        f = cases.field(fname, (3, -2, 0))
        assert f["origin"] != cases.field(fname)["origin"]
        b = cases.random_batch(11, 130, 65, fname=fname, out_cost=3)
        (got,) = emu(f, [b])
        want = mr.weigh(f, b["mp"], b["poses"], b["beams"], b["table"])
        same(got, want, fname)
        assert np.any(want["score"] != mr.weigh(cases.field(fname), b["mp"], b["poses"], b["beams"], b["table"])["score"])


def test_the_limits_are_refused_by_the_shared_check(emu):
    good = cases.random_batch(1, 3, 4, n_table=6)
    none = np.zeros(0, F)
    bad = [("K: 0..2^20", dict(K=2 ** 20 + 1, poses=none)), ("B: 1..65536", dict(B=0, beams=none)), ("B: 1..65536", dict(B=65537, beams=none)),
           ("K * B", dict(K=2 ** 20, poses=none, B=1025, beams=none)), ("n_table: 1..4096", dict(n_table=0, table=np.zeros(0, np.uint32))),
           ("n_table: 1..4096", dict(n_table=4097, table=np.zeros(0, np.uint32))), ("out_cost", dict(mp=mr.mparams(out_cost=2 ** 24 + 1))),
           ("min_inside: 0..B", dict(mp=mr.mparams(min_inside=-1))), ("min_inside: 0..B", dict(mp=mr.mparams(min_inside=5))),
           ("table: every entry", dict(table=np.array([0, 1, 2, 2 ** 24 + 1, 3, 4], np.uint32)))]
    jobs = [dict(good, **kw) for _, kw in bad]
    jobs.append(dict(good, mp=mr.mparams(out_cost=2 ** 24, min_inside=4), table=np.array([2 ** 24, 0, 5, 2 ** 24, 1, 2], np.uint32)))
    got = emu(cases.field("planar"), jobs)
    for (what, kw), g in zip(bad, got):
        assert isinstance(g, str) and g.startswith("check bad: ") and what in g, (kw, g)
    last = jobs[-1]
    same(got[-1], mr.weigh(cases.field("planar"), last["mp"], last["poses"], last["beams"], last["table"]))
