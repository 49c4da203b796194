"""Host tests of the colour layer: the rule functions of limo-velo_amd/csrc/lv_colour.hpp (what the kernels of lv_colour.hip run)
compiled with g++ and held to tests/colour_ref.py on random records, equality everywhere; and the colour methods of VolumeTools
(lv_volumes.hpp) against stand-ins of the store's members: the order of judgement, the stale rows, nothing allocated before the
first lv_colour_integrate / lv_colour_load.  tests/emu/colour_emu.cpp, once plain and once under AddressSanitizer +
UndefinedBehaviorSanitizer."""
import glob
import os
import subprocess

import numpy as np
import pytest

import colour_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
BUILD_DIR = os.path.join(EMU_DIR, "_build")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
SOURCES = [os.path.join(EMU_DIR, "colour_emu.cpp"), os.path.join(EMU_DIR, "hip", "hip_runtime.h"),
           os.path.join(ROOT, "include", "limovelo_hip.h"), *sorted(glob.glob(os.path.join(CSRC, "*.hpp")))]
BUILDS = {"plain": [], "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
SCENARIOS = ["unconfigured", "no_layer", "integrate", "load_clear", "defaults"]
F = np.float32


@pytest.fixture(scope="module")
def emu_bins():
    os.makedirs(BUILD_DIR, exist_ok=True)
    bins = {b: os.path.join(BUILD_DIR, "colour_emu_" + b) for b in BUILDS}
    stale = [b for b, exe in bins.items()
             if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in SOURCES)]
    procs = [(b, subprocess.Popen(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I" + EMU_DIR, *BUILDS[b],
                                   "-o", bins[b], SOURCES[0]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
             for b in stale]
    for b, p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, f"{b} build failed:\n{out}"
    return bins


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_colour_tools_scenario(emu_bins, scenario, build):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([emu_bins[build], scenario], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, f"{scenario} ({build}) exited {r.returncode}:\n{r.stderr[-4000:]}"
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok " + scenario


def _run(emu_bins, lines):
    r = subprocess.run([emu_bins["asan"], "rule"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = r.stdout.strip().split("\n")
    assert len(out) == len(lines)
    return out


def _bits(v):
    return int(np.asarray(v, F).reshape(1).view(np.uint32)[0])


def test_candidates_centres_and_levels(emu_bins):
    rng = np.random.default_rng(11)
    n = 4000
    W = rng.integers(0, 6, n)
    band = rng.integers(1, 4097, n)
    S = rng.integers(-4096, 4097, n) * W
    edge = rng.uniform(size=n) < 0.3   # on and next to the band's edge
    S = np.where(edge, band * W * rng.choice([-1, 1], n) + rng.integers(-1, 2, n), S)
    mw = rng.integers(1, 5, n)
    S[:2], W[:2], band[:2], mw[:2] = [-(2 ** 31), 2 ** 31 - 1], [2 ** 31 - 1, 2 ** 31 - 1], [4096, 4096], [1, 1]   # (the products need 64 bits)
    out = _run(emu_bins, [f"cand {s} {w} {m} {b}" for s, w, m, b in zip(S, W, mw, band)])
    want = [cr.candidates(np.array([s]), np.array([w]), m, b)[0] for s, w, m, b in zip(S, W, mw, band)]
    assert [int(x) for x in out] == [int(x) for x in want] and 0.2 < np.mean(want) < 0.8
    # the centres: the reference's f32 steps, bit for bit
    origin = rng.uniform(-60, 60, 500).astype(F)
    res = rng.choice([0.05, 0.1, 0.2, 0.25, 0.37], 500).astype(F)
    idx = rng.integers(0, 1024, 500)
    out = _run(emu_bins, [f"centre {_bits(o)} {_bits(r)} {i}" for o, r, i in zip(origin, res, idx)])
    for o, r, i, got in zip(origin, res, idx, out):
        want_c = cr.centres((o, o, o), r, (1, 1, 1024), [i])[0, 0]
        assert int(got) == _bits(want_c)
    # the levels: every half step and its neighbours
    s = np.concatenate([np.arange(0, 256, dtype=F), np.arange(0, 255, dtype=F) + F(0.5), np.nextafter(np.arange(0, 255, dtype=F) + F(0.5), F(0)),
                        rng.uniform(0, 255, 500).astype(F)])
    out = _run(emu_bins, [f"quant {_bits(v)}" for v in s])
    assert [int(x) for x in out] == [int(x) for x in cr.quantise((s + F(0.5)).astype(np.float64) - 0.5)]


def test_fold_and_colours(emu_bins):
    rng = np.random.default_rng(12)
    n = 4000
    mw = rng.choice([1, 2, 3, 64, 65535], n)
    Wc = np.minimum(rng.integers(0, 70000, n), mw)
    Wc[rng.uniform(size=n) < 0.3] = 0
    C = np.array([rng.integers(0, 255 * w + 1) for w in Wc for _ in range(3)], np.int64).reshape(n, 3)
    full = rng.uniform(size=n) < 0.2
    C[full] = 255 * Wc[full, None]                     # C = 255 * Wc
    k = rng.integers(1, 33, n)
    at_cap = rng.uniform(size=n) < 0.3
    k = np.where(at_cap & (mw - Wc >= 1) & (mw - Wc <= 32), mw - Wc, k)   # Wn == max_weight
    dC = np.array([rng.integers(0, 255 * v + 1) for v in k for _ in range(3)], np.int64).reshape(n, 3)
    dC[full] = 255 * k[full, None]
    out = _run(emu_bins, [f"fold {m} {v} {d[0]} {d[1]} {d[2]} {c[0]} {c[1]} {c[2]} {w}" for m, v, d, c, w in zip(mw, k, dC, C, Wc)])
    got = np.array([o.split() for o in out], np.uint32)
    e = np.concatenate([C, Wc[:, None]], axis=1)
    want = np.stack([cr.fold(e[i:i + 1], k[i:i + 1], dC[i:i + 1], mw[i])[0] for i in range(n)])
    assert np.array_equal(got, want)
    assert np.all(got[:, :3] <= 255 * got[:, 3:4]) and np.all(got[:, 3] <= mw)
    assert ((Wc + k) == mw).sum() > 50 and ((Wc + k) > mw).sum() > 500 and ((Wc + k) < mw).sum() > 500
    # the voxel colour of the entries before and after
    both = np.concatenate([e, got.astype(np.int64)])
    out = _run(emu_bins, [f"voxel {c[0]} {c[1]} {c[2]} {c[3]}" for c in both])
    assert np.array_equal(np.array([o.split() for o in out], np.uint8), cr.voxel_colour(both))
    # the vertex colour: k = 0..8 coloured corners
    corners = got[rng.integers(0, n, (900, 8))].astype(np.int64)
    for v in range(900):
        corners[v, rng.permutation(8)[:8 - v % 9]] = 0
    out = _run(emu_bins, ["vertex " + " ".join(str(x) for x in c.reshape(-1)) for c in corners])
    assert np.array_equal(np.array([o.split() for o in out], np.uint8), cr.vertex_colour(corners))
    assert sorted(set((corners[:, :, 3] > 0).sum(axis=1))) == list(range(9))


def test_layer_and_parameter_checks(emu_bins):
    good = [5, 255 * 2, 0, 2, 0, 0, 0, 0, 255 * 65535, 1, 2, 65535]
    cases = [(good, 3), (good[:4] + [1, 0, 0, 0] + good[8:], 1), (good[:8] + [0, 0, 0, 65536], 2), ([0, 0, 511, 2] + good[4:], 0), ([], 0)]
    out = _run(emu_bins, [f"layer {len(c) // 4} " + " ".join(str(x) for x in c) for c, _ in cases])
    assert [int(x) for x in out] == [w for _, w in cases]
    rows = [((0, 256, 1, 64), "ok"), ((0, 1, 1, 1), "ok"), ((0, 4096, 7, 65535), "ok"),
            ((1, 256, 1, 64), "lv_colour_integrate: blend = 1: the layer takes the mean, blend 0"),
            ((0, 0, 1, 64), "lv_colour_integrate: band = 0: must be in 1..T"), ((0, 4097, 1, 64), "lv_colour_integrate: band = 4097: must be in 1..T"),
            ((0, 256, 0, 64), "lv_colour_integrate: min_weight = 0: at least 1"),
            ((0, 256, 1, 0), "lv_colour_integrate: max_weight = 0: must be in 1..65535"),
            ((0, 256, 1, 65536), "lv_colour_integrate: max_weight = 65536: must be in 1..65535"),
            ((2, 256, 1, 64), "blend = 2: must be 0 or 1")]   # (lv_map_paint's own rule comes first)
    out = _run(emu_bins, ["params " + " ".join(str(x) for x in r) for r, _ in rows])
    assert out == [w for _, w in rows]
