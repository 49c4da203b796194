"""The rule of lv_mcl_filter.hpp (the draws, the move, the accumulation, the weights, the estimate's sums, the decision, the two-level
ancestor search, the checks and the states: what the kernels of lv_mcl_filter.hip run) compiled with g++ and
-fsanitize=address,undefined through tests/emu/hip/hip_runtime.h and held to tests/mcl_filter_ref.py: tests/emu/mcl_filter_emu.cpp
loads a field and runs sequences of set, move, weigh, resample and get on the room of tests/mcl_cases.py.  Equality on every pose bit,
acc, n_in, best, statistic and ancestor, and on the refusals' texts."""
import os
import subprocess

import numpy as np
import pytest

import mcl_cases as cases
import mcl_filter_ref as fr
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


def line_of(c):
    """A command (a tuple: its letter, then its arguments) as the emulation reads it.  K, n_table, B and n_w may be declared apart
    from the arrays (a dict of overrides as the last element)."""
    over = c[-1] if isinstance(c[-1], dict) else {}
    if c[0] == "S":
        return f"S {int(c[2])} {over.get('K', len(c[1]))} {_arr(c[1], True)}"
    if c[0] == "M":
        return f"M {_bits(c[1])} {_bits(c[2])}"
    if c[0] == "W":
        mp = c[3]
        return f"W {mp['out_cost']} {mp['min_inside']} {over.get('n_table', len(c[2]))} {_arr(c[2], False)} {over.get('B', len(c[1]))} {_arr(c[1], True)}"
    if c[0] == "R":
        p = c[2]
        return f"R {p.shift} {p.mode} {p.below_num} {p.below_den} {over.get('n_w', len(c[1]))} {_arr(c[1], False)}"
    if c[0] == "E":
        return f"E {int(c[1])} {int(c[2])}"
    return c[0]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mcl_filter_host") / "mcl_filter_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "mcl_filter_emu.cpp"), "-o", str(exe)])

    def run(field, commands, K):
        """The emulation's answers, one per command: the refusal's text, or None (S, M, E), best (W), (stats dict, ancestors) (R),
        dict(poses, acc, n_in) (G).  K: the particles a G prints."""
        s2 = np.asarray(field["s2"])
        planar = s2.ndim == 2
        nz = 1 if planar else s2.shape[0]
        lines = [f"{int(planar)} {_bits(field['origin'])} {_bits([field['resolution']])} {s2.shape[-1]} {s2.shape[-2]} {nz}", _ints(s2)]
        lines += [line_of(c) for c in commands]
        out = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
        got, at = [], 0
        for c in commands:
            head = out[at]
            at += 1
            if head != "ok":
                got.append(head)
                continue
            if c[0] == "W":
                got.append(np.array([int(v) for v in out[at].split()], np.int64))
                at += 1
            elif c[0] == "R":
                v = [int(t) for t in out[at].split()]
                at += 1
                st = dict(W=v[0], sum_w2=v[1], s_min=v[2], S=v[3:8], n_eligible=v[8], n_clamped=v[9], resampled=v[10], epoch=v[11], since_resample=v[12])
                anc = None
                if st["resampled"]:
                    anc = np.array([int(t) for t in out[at].split()], np.uint32)
                    at += 1
                got.append((st, anc))
            elif c[0] == "G":
                rows = np.array([[int(t) for t in r.split()] for r in out[at:at + K]], np.uint64).reshape(K, 6)
                at += K
                got.append(dict(poses=rows[:, :4].astype(np.uint32).view(F), acc=rows[:, 4].copy(), n_in=rows[:, 5].astype(np.uint32)))
            else:
                got.append(None)
        assert out[at:] == [""]
        return got

    return run


def reference(field, commands):
    """The same commands through RefFilterContext (refusals are not run here)."""
    ctx, out = fr.RefFilterContext(field), []
    for c in commands:
        if c[0] == "S":
            out.append(ctx.occ_mcl_filter_set(c[1], c[2]))
        elif c[0] == "M":
            out.append(ctx.occ_mcl_filter_move(c[1], c[2]))
        elif c[0] == "W":
            out.append(ctx.occ_mcl_filter_weigh(c[1], c[2], type("P", (), c[3])))
        elif c[0] == "R":
            st, anc = ctx.occ_mcl_filter_resample(c[1], c[2])
            d = fr.stats_dict(st)
            del d["origin"], d["resolution"]
            out.append((d, anc))
        elif c[0] == "G":
            out.append(ctx.occ_mcl_filter_get())
    return out


def same(got, want, commands):
    assert len(got) == len(want)
    for n, (c, g, w) in enumerate(zip(commands, got, want)):
        where = (n, c[0])
        assert not isinstance(g, str), (where, g)
        if c[0] == "W":
            assert np.array_equal(g, w), (where, g, w)
        elif c[0] == "R":
            assert g[0] == w[0], (where, g[0], w[0])
            assert (g[1] is None) == (w[1] is None) and (g[1] is None or np.array_equal(g[1], w[1])), where
        elif c[0] == "G":
            assert np.array_equal(g["poses"].view(np.uint32), w["poses"].view(np.uint32)), (where, np.nonzero(g["poses"].view(np.uint32) != w["poses"].view(np.uint32))[0][:8])
            assert np.array_equal(g["acc"], w["acc"]) and np.array_equal(g["n_in"], w["n_in"]), where


def cycles(seed, K, B, n_table, n_w, shift, mode, fname, n_cycles=3, **mp):
    """set, then n_cycles of move, weigh, get, resample, get on poses over the room."""
    b = cases.random_batch(seed, K, B, n_table=n_table, fname=fname, **mp)
    rng = np.random.default_rng(seed)
    if K <= 2:
        b["poses"][:, :3] = [4.0, 1.0, 0.2]   # (in the room: somebody is eligible)
    wtable = np.rint(1048576.0 * np.exp(-np.arange(n_w) / 40.0)).astype(np.uint32)
    out = [("S", b["poses"], seed + 1000), ("G",)]
    for k in range(n_cycles):
        delta = np.array([rng.uniform(-0.2, 0.2), rng.uniform(0.1, 0.4), rng.uniform(-0.2, 0.2)], F)
        sigma = np.array([0.05, 0.03, 0.05], F)
        out += [("M", delta, sigma), ("W", b["beams"], b["table"], b["mp"]), ("G",), ("R", wtable, fr.rparams(shift=shift, mode=mode)), ("G",)]
    return out


@pytest.mark.parametrize("K,B,fname,n_w,shift,mode", [(1, 3, "planar", 1, 0, 2), (2, 1, "vol", 2, 3, 1), (257, 65, "planar", 4096, 0, 1),
                                                      (300, 64, "vol", 4096, 3, 2), (513, 5, "planar", 64, 0, 0), (600, 33, "trunc", 4096, 0, 1)])
def test_sequences_against_the_reference(emu, K, B, fname, n_w, shift, mode):
    cmds = cycles(7 * K + B, K, B, 512, n_w, shift, mode, fname, out_cost=(0, 900)[K & 1], min_inside=min(B, K % 3))
    got = emu(cases.field(fname), cmds, K)
    want = reference(cases.field(fname), cmds)
    same(got, want, cmds)
    # (two particles never have n_eff < 1 = K / 2: that sequence runs mode 1 without a resampling)
    assert mode == 0 or K == 2 or any(w[0]["resampled"] for c, w in zip(cmds, want) if c[0] == "R")
    assert mode != 0 or not any(w[0]["resampled"] for c, w in zip(cmds, want) if c[0] == "R")


def test_degenerate_particles(emu):
    """Unusable and NaN headings before and after a move, particles far outside the field, a heading that a move makes unusable, one
    particle holding all the weight, nobody eligible, and weighing twice without a move."""
    b = cases.random_batch(5, 12, 33, out_cost=50)
    x = b["poses"].copy()
    x[:, :2] = [4.0, 1.0]
    x[:9, 3] = [0.3, 1048576.0, -1048576.0, np.nan, np.inf, -np.inf, 1048575.9375, -1048575.9375, 2.0e6]
    x[9, :3] = [1.0e9, -3.0e38, np.nan]
    x[10, :2] = [np.inf, 5000.0]
    x[11, 3] = 3.1
    d, s = np.array([0.125, 0.3, 0.05], F), np.array([0.01, 0.02, 0.01], F)
    wt = np.array([1 << 20, 5, 0], np.uint32)
    cmds = [("S", x, 3), ("M", d, s), ("G",), ("W", b["beams"], b["table"], b["mp"]), ("W", b["beams"], b["table"], b["mp"]), ("G",),
            ("R", wt, fr.rparams(mode=0)), ("M", d, s), ("W", b["beams"], b["table"], b["mp"]), ("R", wt, fr.rparams(mode=2)), ("G",),
            ("W", b["beams"], b["table"], mr.mparams(min_inside=34 - 1)), ("R", wt, fr.rparams(mode=2)), ("G",)]
    f = cases.field("planar")
    got, want = emu(f, cmds, 12), reference(f, cmds)
    same(got, want, cmds)
    moved = want[2]["poses"]
    assert np.array_equal(moved[[1, 2, 3, 4, 5, 8]].view(np.uint32), x[[1, 2, 3, 4, 5, 8]].view(np.uint32))   # untouched
    assert not mr.usable(moved[6, 3]) and moved[6, 0] == x[6, 0] and moved[6, 3] != x[6, 3]                   # a became unusable: x, y stay
    assert mr.usable(moved[7, 3]) or moved[7, 0] == x[7, 0]
    assert abs(moved[11, 3]) <= np.pi + 1e-6 and moved[11, 3] < 0                                              # wrapped
    st = want[6][0]
    assert st["n_clamped"] == 2 and st["resampled"] == 0 and 0 < st["n_eligible"] < 12 and st["since_resample"] == 2
    assert want[5]["acc"][0] == 2 * (want[5]["acc"][0] // 2) and np.sum(want[5]["acc"] == np.uint64(mr.NO_SCORE)) == 12 - st["n_eligible"]
    # all zero weight: nothing moves
    cmds2 = [("S", x, 3), ("W", b["beams"], b["table"], b["mp"]), ("R", np.zeros(4, np.uint32), fr.rparams(mode=2)), ("G",),
             ("W", b["beams"], b["table"], mr.mparams(min_inside=33, out_cost=1)), ("R", wt, fr.rparams(mode=2)), ("G",)]
    got2, want2 = emu(f, cmds2, 12), reference(f, cmds2)
    same(got2, want2, cmds2)
    assert want2[2][0]["W"] == 0 and want2[2][0]["resampled"] == 0 and want2[2][0]["s_min"] >= 0 and want2[2][1] is None
    assert np.array_equal(want2[3]["poses"].view(np.uint32), x.view(np.uint32))


def test_one_heavy_particle_takes_every_ancestor(emu):
    b = cases.random_batch(9, 300, 64)
    x = b["poses"].copy()
    x[:, :2] += F(500.0)
    x[77] = [4.5, 2.5, 0.2, 0.25]
    cmds = [("S", x, 1), ("W", b["beams"], b["table"], b["mp"]), ("R", np.array([9, 1], np.uint32), fr.rparams(mode=2)), ("G",)]
    got, want = emu(cases.field("planar"), cmds, 300), reference(cases.field("planar"), cmds)
    same(got, want, cmds)
    assert np.all(want[2][1] == 77) and want[2][0]["n_eligible"] == 1 and want[2][0]["W"] == 9
    assert np.all(want[3]["poses"].view(np.uint32) == x[77].view(np.uint32))


def test_refusals_by_the_shared_checks_and_states(emu):
    b = cases.random_batch(1, 3, 4, n_table=6)
    good_w = np.array([4, 2, 1], np.uint32)
    none_f, none_u = np.zeros(0, F), np.zeros(0, np.uint32)
    d, s = np.array([0.1, 0.2, 0.1], F), np.array([0.01, 0.01, 0.01], F)
    mp, rp = b["mp"], fr.rparams
    cmds = [
        (("G",), "state bad: no particles"), (("M", d, s), "state bad: no particles"), (("W", b["beams"], b["table"], mp), "state bad: no particles"),
        (("R", good_w, rp()), "state bad: no particles"),
        (("S", none_f, 0, dict(K=0)), "K: 1..2^20"), (("S", none_f, 0, dict(K=2 ** 20 + 1)), "K: 1..2^20"),
        (("S", b["poses"], 5), None),
        (("M", np.array([np.nan, 0, 0], F), s), "delta: finite"), (("M", np.array([0, np.inf, 0], F), s), "delta: finite"),
        (("M", d, np.array([0, -1e-3, 0], F)), "sigma"), (("M", d, np.array([0, 0, np.inf], F)), "sigma"), (("M", d, np.array([np.nan, 0, 0], F)), "sigma"),
        (("W", none_f, b["table"], mp, dict(B=0)), "B: 1..65536"), (("W", none_f, b["table"], mp, dict(B=65537)), "B: 1..65536"),
        (("W", b["beams"], none_u, mp, dict(n_table=0)), "n_table: 1..4096"), (("W", b["beams"], none_u, mp, dict(n_table=4097)), "n_table: 1..4096"),
        (("W", b["beams"], b["table"], mr.mparams(out_cost=2 ** 24 + 1)), "out_cost"), (("W", b["beams"], b["table"], mr.mparams(min_inside=-1)), "min_inside"),
        (("W", b["beams"], b["table"], mr.mparams(min_inside=5)), "min_inside"),
        (("W", b["beams"], np.array([0, 2 ** 24 + 1], np.uint32), mp), "table: every entry"),
        (("R", good_w, rp(shift=-1)), "shift: 0..63"), (("R", good_w, rp(shift=64)), "shift: 0..63"), (("R", good_w, rp(mode=3)), "mode"),
        (("R", good_w, rp(mode=-1)), "mode"), (("R", good_w, rp(below_num=0)), "below"), (("R", good_w, rp(below_num=3, below_den=2)), "below"),
        (("R", good_w, rp(below_num=1, below_den=65537)), "below"), (("R", none_u, rp(), dict(n_w=0)), "n_w: 1..4096"),
        (("R", none_u, rp(), dict(n_w=4097)), "n_w: 1..4096"), (("R", np.array([1, 2 ** 20 + 1], np.uint32), rp()), "wtable: every entry"),
        (("G",), None),
        # the epoch at its end: _move and _resample are refused, _weigh is not; nothing changes
        (("E", 2 ** 32 - 1, 0), None), (("M", d, s), "state bad: the epoch has reached 2^32 - 1"), (("R", good_w, rp()), "state bad: the epoch has reached"),
        (("W", b["beams"], b["table"], mp), None), (("G",), None),
        # one before the end both still run
        (("E", 2 ** 32 - 2, 0), None), (("M", d, s), None), (("M", d, s), "state bad: the epoch"),
        # the 2^20-th weigh since the last resampling is refused; the one before it runs
        (("E", 7, 2 ** 20 - 2), None), (("W", b["beams"], b["table"], mp), None), (("W", b["beams"], b["table"], mp), "state bad: 2^20 scans"),
        (("R", np.array([1 << 20] * 3, np.uint32), rp(mode=2, below_num=65536, below_den=65536)), None), (("W", b["beams"], b["table"], mp), None),
    ]
    got = emu(cases.field("planar"), [c for c, _ in cmds], 3)
    for (c, what), g in zip(cmds, got):
        if what is None:
            assert not isinstance(g, str), (c[0], g)
        else:
            assert isinstance(g, str) and what in g and g.startswith(("check bad: ", "state bad: ")), (c[0], what, g)
    # the refused calls changed nothing: the particles after the refusals are those of the set, and the weigh at the last epoch counted
    first_get, second_get = [g for (c, w), g in zip(cmds, got) if c[0] == "G" and w is None][:2]
    assert np.array_equal(first_get["poses"].view(np.uint32), b["poses"].view(np.uint32)) and not first_get["acc"].any()
    assert np.array_equal(second_get["poses"].view(np.uint32), b["poses"].view(np.uint32))
    want = mr.weigh(cases.field("planar"), mp, b["poses"], b["beams"], b["table"])
    assert np.array_equal(second_get["acc"], want["score"]) and np.array_equal(second_get["n_in"], want["n_in"])
    st = got[-2][0]
    assert st["resampled"] == 1 and st["since_resample"] == 0 and st["epoch"] == 8


def test_the_decision_at_its_boundary(emu):
    """One eligible particle of K = 3 (the others stand far outside): W = w, sum_w2 = w^2, so mode 1 resamples iff below_den <
    3 * below_num.  At the boundary, one above it and one below it, with w = 2^20."""
    b = cases.random_batch(9, 3, 64)
    x = b["poses"].copy()
    x[:, :2] += F(500.0)
    x[1] = [4.5, 2.5, 0.2, 0.25]
    wt = np.array([1 << 20], np.uint32)
    cmds = [("S", x, 1), ("W", b["beams"], b["table"], b["mp"])]
    cmds += [("R", wt, fr.rparams(mode=1, below_num=21845, below_den=den)) for den in (65535, 65536, 65534)]
    got, want = emu(cases.field("planar"), cmds, 3), reference(cases.field("planar"), cmds)
    same(got, want, cmds)
    assert [w[0]["resampled"] for w in want[2:]] == [0, 0, 1] and want[2][0]["W"] == 1 << 20 and want[2][0]["sum_w2"] == 1 << 40
    assert np.all(want[4][1] == 1)
