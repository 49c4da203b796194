"""The plain arithmetic of lv_map_planes (limo-velo_amd/csrc/lv_planes.hpp with sym3_eig / surf_sign of lv_surface.hpp) compiled
with plain g++ and -fsanitize=address,undefined into tests/emu/planes_emu.cpp and held BY BITS to the numpy / Python-int statement
of the rule in tests/planes_ref.py: the draws, the hypothesis planes with every invalid branch and both sign rules, the inlier
test, the quantisation, the 128-bit fold, the refit and the 3 x 3 eigen-solver.  plane_rule is held to the table of
tests/plane_cases.py.  Nothing is loaded into Python."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import plane_cases as pc
import planes_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
HEADER = os.path.join(ROOT, "limo-velo_amd", "csrc", "lv_planes.hpp")
F = np.float32


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("planes_host") / "planes_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(EMU_DIR, "planes_emu.cpp"), "-o", str(exe)])

    def run(lines):
        res = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert res.returncode == 0, res.stderr.decode()[-2000:]
        rows = res.stdout.decode().split("\n")
        assert rows[-1] == "" and len(rows) == len(lines) + 1
        return rows[:-1]

    return run


def _f(vals):
    return " ".join(str(int(v)) for v in pr.b32(vals).reshape(-1))


def _d(vals):
    return " ".join(str(int(v)) for v in pr.b64(vals).reshape(-1))


# ---- the draws
def test_draws(emu):
    reqs = []
    for n in (3, 4, 2**32 - 1):
        for seed in (0, 1, 0xDEADBEEFCAFEF00D, 2**64 - 1):
            for r in (0, 1, 31):
                for h in (0, 1, 255, 256, 65535):
                    for j in range(3):
                        reqs.append((seed, r, h, j, n))
    got = [int(x) for x in emu([f"draw {s} {r} {h} {j} {n}" for s, r, h, j, n in reqs])]
    want = [pr.draw(*q) for q in reqs]
    assert got == want
    assert all(0 <= w < q[4] for w, q in zip(want, reqs))
    assert len({w for w, q in zip(want, reqs) if q[4] == 2**32 - 1}) == 180         # (all distinct: the draws spread ...)
    assert {w for w, q in zip(want, reqs) if q[4] == 3} == {0, 1, 2}                # (... and reach every index of a small set)
    assert pr.mix(0) == 0xE220A8397B1DCDAF                                          # splitmix64's first output from state 0


# ---- the hypothesis planes
def _hyp_cases():
    rng = np.random.default_rng(5)
    z = (0.0, 0.0, 1.0)
    cases = []   # (p0, p1, p2, constraint, axis, cos, sin, what)
    for _ in range(200):
        p = (rng.normal(size=(3, 3)) * rng.choice([0.01, 1.0, 100.0])).astype(F)
        cases.append((p[0], p[1], p[2], 0, (0.0, 0.0, 0.0), 0.0, 0.0, "random"))
    for _ in range(100):   # far from the origin: the f64 differences of f32 points stay exact
        p = (rng.normal(size=(3, 3)) + [30000.0, -20000.0, 500.0]).astype(F)
        cases.append((p[0], p[1], p[2], 0, (0.0, 0.0, 0.0), 0.0, 0.0, "far"))
    a = np.array([1.0, 2.0, 3.0], F)
    cases.append((a, a, a, 0, z, 0.0, 0.0, "three equal points"))                   # cc = 0, uu vv = 0: invalid (0 > 0 is false)
    cases.append((a, a + F(1), a, 0, z, 0.0, 0.0, "two equal points"))
    cases.append((a, a + F(1), a + F(2), 0, z, 0.0, 0.0, "collinear"))
    cases.append((a, a + np.array([1, 0, 0], F), a + np.array([2, 1e-6, 0], F), 0, z, 0.0, 0.0, "sliver below the bound"))
    cases.append((a, a + np.array([1, 0, 0], F), a + np.array([2, 1e-5, 0], F), 0, z, 0.0, 0.0, "sliver above the bound"))
    cases.append((a, a + np.array([np.nan, 0, 0], F), a + np.array([0, 1, 0], F), 0, z, 0.0, 0.0, "NaN"))
    cases.append((a, a + np.array([np.inf, 0, 0], F), a + np.array([0, 1, 0], F), 0, z, 0.0, 0.0, "inf"))
    # the sign rules: largest component positive, ties to the lower axis; constraint 1 towards the axis, a zero dot falls back
    o = np.zeros(3, F)
    for p1, p2 in (([1, 0, 0], [0, 1, 0]), ([0, 1, 0], [1, 0, 0]), ([1, -1, 0], [0, 1, -1]), ([0, 1, -1], [1, -1, 0]),
                   ([1, 0, -1], [0, 1, -1]), ([0, 1, 1], [1, 0, 0]), ([1, 0, 0], [0, 1, 1])):
        for constraint, axis in ((0, z), (1, z), (1, (0.0, 0.0, -1.0)), (1, (1.0, 0.0, 0.0)), (2, z)):
            cases.append((o, np.array(p1, F), np.array(p2, F), constraint, axis, 0.0, 1.0, "sign"))
    # the constraints, on both sides of the threshold: a plane tilted by 20 degrees about x, thresholds at 15 / 25 degrees and
    # exactly at the tilt's own t
    t = math.radians(20.0)
    q1, q2 = np.array([1, 0, 0], F), np.array([0, math.cos(t), math.sin(t)], F)
    _, nrm = pr.hypotheses(o, q1, q2)
    own = abs(float(nrm[0, 2]))   # (about cos 20 deg; the f64 t of the rule is formed from the unrounded normal: see below)
    for constraint in (1, 2):
        for ang in (math.radians(15.0), math.radians(25.0), math.radians(65.0), math.radians(75.0)):
            cases.append((o, q1, q2, constraint, z, math.cos(ang), math.sin(ang), "constraint"))
        cases.append((o, q1, q2, constraint, z, own, own, "constraint at the normal's own value"))
    for constraint in (1, 2):   # exactly on the threshold: a z = 0 plane has t = 1 against z and t = 0 against x
        cases.append((o, np.array([1, 0, 0], F), np.array([0, 1, 0], F), constraint, z, 1.0, 1.0, "t == threshold 1"))
        cases.append((o, np.array([1, 0, 0], F), np.array([0, 1, 0], F), constraint, (1.0, 0.0, 0.0), 0.0, 0.0, "t == threshold 0"))
        cases.append((o, np.array([1, 0, 0], F), np.array([0, 1, 0], F), constraint, z, math.nextafter(1.0, 2.0), math.nextafter(1.0, 0.0), "one ulp off 1"))
    return cases


def test_hypothesis_planes(emu):
    cases = _hyp_cases()
    got = [[int(x) for x in row.split()] for row in emu([f"hyp {_f(p0)} {_f(p1)} {_f(p2)} {c} {_d(ax)} {_d(cm)} {_d(sm)}" for p0, p1, p2, c, ax, cm, sm, _ in cases])]
    seen = set()
    for (p0, p1, p2, c, ax, cm, sm, what), row in zip(cases, got):
        valid, nrm = pr.hypotheses(p0, p1, p2, c, ax, cm, sm)
        assert row == [int(valid[0])] + [int(v) for v in pr.b32(nrm[0])], (what, row)
        seen.add((what, c, bool(valid[0])))
        if valid[0]:
            assert abs(float(np.linalg.norm(nrm[0].astype(np.float64))) - 1.0) < 1e-6
    # every branch shows on both sides
    for what in ("three equal points", "two equal points", "collinear", "sliver below the bound", "NaN", "inf"):
        assert (what, 0, False) in seen, what
    assert ("sliver above the bound", 0, True) in seen and ("random", 0, True) in seen and ("far", 0, True) in seen
    for c in (1, 2):
        assert {("constraint", c, True), ("constraint", c, False)} <= seen
        assert {("t == threshold 1", c, True), ("t == threshold 0", c, True)} <= seen   # (>= and <= admit equality)
        assert ("one ulp off 1", c, False) in seen
    signs = [(c, tuple(np.sign(pr.hypotheses(p0, p1, p2, c, ax, cm, sm)[1][0]).astype(int))) for p0, p1, p2, c, ax, cm, sm, w in cases if w == "sign"]
    assert (0, (0, 0, 1)) in signs and (1, (0, 0, -1)) in signs           # z up by the component rule, z down towards a -z axis
    assert (0, (1, 1, 1)) in signs and (0, (1, -1, -1)) not in signs       # a three-way tie goes to the lower axis: x positive


# ---- the inlier test, at the threshold and one ulp beyond
def test_inlier_test(emu):
    rng = np.random.default_rng(6)
    n = rng.normal(size=(300, 3))
    n = (n / np.linalg.norm(n, axis=1)[:, None]).astype(F)
    a = (rng.normal(size=(300, 3)) * 50).astype(F)
    p = (a + rng.normal(size=(300, 3)) * rng.choice([0.05, 0.2, 5.0], size=(300, 1))).astype(F)
    s = np.array([pr.signed(n[i], a[i], p[i])[0, 0] for i in range(300)], F)
    dist = np.concatenate([np.abs(s[:100]), np.nextafter(np.abs(s[100:200]), F(0)), np.full(100, 0.1, F)]).astype(F)
    rows = emu([f"test {_f(n[i])} {_f(a[i])} {_f(p[i])} {_f(dist[i])}" for i in range(300)])
    want_in = np.abs(s) <= dist
    assert [r.split() for r in rows] == [[str(int(pr.b32(s[i])[0])), str(int(want_in[i]))] for i in range(300)]
    assert want_in[:100].all() and not want_in[100:200][np.abs(s[100:200]) > 0].any() and 0 < want_in[200:].sum() < 100


# ---- the quantisation
def test_quantisation(emu):
    a = F(0.0)
    edge = 2.0**22 / 256.0   # 16384 m
    ps = [0.0, 1.0 / 512, 3.0 / 512, 5.0 / 512, -1.0 / 512, -3.0 / 512, 0.5 / 256 + 2**-20, 0.49 / 256, 7.3, -7.3,
          edge, -edge, edge + 1.0 / 512, -(edge + 1.0 / 512), edge + 1.0 / 256, -(edge + 1.0 / 256), edge - 1.0 / 512, 3e4, -3e4, 1e30, -1e30,
          float(np.finfo(F).max), np.inf, -np.inf, np.nan]
    pairs = [(F(p), a) for p in ps] + [(F(30000.0 + p), F(30000.0)) for p in (0.0, 0.25, -0.25, 1.0 / 512)] + [(F(1e30), F(-1e30)), (F(np.inf), F(np.inf))]
    got = [[int(x) for x in r.split()] for r in emu([f"quant {_f(p)} {_f(q)}" for p, q in pairs])]
    for (p, q), row in zip(pairs, got):
        ok, gq = pr.quant(p, q)
        assert row == [int(ok), int(gq)], (p, q, row)
    by = {float(p): r for (p, q), r in zip(pairs[:len(ps)], got) if p == p}
    assert by[1.0 / 512] == [1, 0] and by[3.0 / 512] == [1, 2] and by[5.0 / 512] == [1, 2] and by[-3.0 / 512] == [1, -2]   # half to even
    assert by[edge] == [1, 2**22] and by[-edge] == [1, -2**22]                         # 2^22 itself is inside
    assert by[float(F(edge + 1.0 / 512))] == [1, 2**22]                                # 2^22 + 0.5 rounds to the even 2^22: inside
    assert by[float(F(edge + 1.0 / 256))] == [0, 0] and by[-float(F(edge + 1.0 / 256))] == [0, 0]   # 2^22 + 1: out
    assert by[np.inf] == [0, 0] and by[1e30 if False else float(F(1e30))] == [0, 0]
    assert got[len(ps) - 1] == [0, 0]                                                   # NaN


# ---- the 128-bit fold
def _fold_line(slots):
    return f"fold {len(slots)} " + " ".join(str(v) for s in slots for v in s)


def _want_fold(slots):
    t = [sum(s[k] for s in slots) for k in range(10)]
    m = pr.moment(t[0], t[1:4], t[4:10])
    return [t[0]] + [int(v) for v in pr.b64(m)] + [int(v) for v in pr.b64([float(x) for x in t[1:4]])]


def test_fold(emu):
    rng = np.random.default_rng(8)
    G = 2**22
    cases = []
    # the largest admitted sums: 2^32 points in slots of 2^19 would be 8192 slots of (2^19, +-2^41, 2^63 - ...): a slot's S2 entry is
    # at most 2^19 * 2^44 = 2^63, which int64 misses by one, so a full slot holds 2^19 - 1 points at the corner
    full = 2**19 - 1
    corner = [full, full * G, -full * G, full * G, full * G * G, -full * G * G, full * G * G, full * G * G, -full * G * G, full * G * G]
    assert max(abs(v) for v in corner) < 2**63
    mirror = [-v if k in (1, 2, 3) else v for k, v in enumerate(corner)]   # the same points reflected through the anchor
    cases.append([corner, mirror] * 4096)                          # ~2^32 points: n S2 ~ 2^108, far beyond 64 bits
    cases.append([corner] * 8192)                                  # all at one corner: S1 S1^T ~ 2^108 cancels it exactly, M = 0
    cases.append([corner, mirror])
    cases.append([[0] * 10])
    cases.append([[1, 5, -3, 2, 25, -15, 10, 9, -6, 4]])           # one point: M = 0 exactly
    for _ in range(20):
        ns = int(rng.integers(1, 6))
        slots = []
        for _ in range(ns):
            g = rng.integers(-G, G + 1, size=(int(rng.integers(1, 50)), 3))
            slots.append([len(g)] + [int(g[:, a].sum()) for a in range(3)] +
                         [int((g[:, a] * g[:, b]).sum()) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])
        cases.append(slots)
    got = [[int(x) for x in r.split()] for r in emu([_fold_line(s) for s in cases])]
    for slots, row in zip(cases, got):
        assert row == _want_fold(slots)
    big = _want_fold(cases[0])
    assert big[0] == 8192 * full and float(np.array([big[1]], np.uint64).view(np.float64)[0]) > 2.0**100
    assert got[1][1:7] == [0] * 6 and got[4][1:7] == [0] * 6


# ---- the 3 x 3 eigen-solver's port, and the refit on top of it
def _eig_inputs():
    rng = np.random.default_rng(9)
    out = []
    for _ in range(200):
        a = rng.normal(size=(3, 3)) * 10.0 ** rng.integers(-8, 30)
        c = a @ a.T
        out.append([c[0, 0], c[0, 1], c[0, 2], c[1, 1], c[1, 2], c[2, 2]])
    for _ in range(60):   # rank 2, rank 1: a plane's and a line's moment matrix
        b = rng.normal(size=(3, int(rng.integers(1, 3))))
        c = b @ b.T
        out.append([c[0, 0], c[0, 1], c[0, 2], c[1, 1], c[1, 2], c[2, 2]])
    out += [[0.0] * 6, [1.0, 0, 0, 1.0, 0, 1.0], [2.0, 0, 0, 1.0, 0, 0.0], [0.0, 0, 0, 0.0, 0, 5.0], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
            [np.inf, 0, 0, 1.0, 0, 1.0], [1e-300, 0, 0, 2e-300, 1e-301, 0.0], [2.0**108, -(2.0**107), 0, 2.0**108, 1.0, 2.0**100],
            [4.0, 0.0, 0.0, 4.0, 3.0, 4.0]]
    return out


def test_sym3_eig_port(emu):
    cs = _eig_inputs()
    got = [[int(x) for x in r.split()] for r in emu([f"eig {_d(c)}" for c in cs])]
    for c, row in zip(cs, got):
        l, v = pr.sym3_eig(c)
        assert row == [int(x) for x in pr.b64(l + v)], c
    # and the port is an eigen-solver: against numpy on the well-conditioned ones
    for c in cs[:200]:
        l, v = pr.sym3_eig(c)
        m = np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])
        w = np.linalg.eigvalsh(m)
        assert np.allclose(l, w, rtol=1e-9, atol=1e-12 * abs(w).max())


def test_refit(emu):
    rng = np.random.default_rng(10)
    reqs, wants = [], []
    z = (0.0, 0.0, 1.0)
    for k in range(40):
        n = int(rng.integers(0, 6)) if k < 8 else int(rng.integers(3, 400))
        tilt = rng.normal(size=3) * 0.2
        xy = rng.uniform(-20, 20, size=(n, 2))
        pts = np.column_stack([xy, xy @ tilt[:2] + rng.normal(size=n) * 0.01]).astype(F)
        anchor = pts[0] if n else np.zeros(3, F)
        n_fit, s1, s2 = pr.sums(pts, anchor)
        m = pr.moment(n_fit, s1, s2)
        constraint, axis = [(0, (0.0, 0.0, 0.0)), (1, z), (1, (0.0, 0.0, -1.0)), (2, z)][k % 4]
        nrm0 = np.array([0.0, 0.6, 0.8], F)
        reqs.append(f"refit {n_fit} {_d(m)} {_d([float(v) for v in s1])} {constraint} {_d(axis)} {_f(nrm0)} {_f(anchor)}")
        done, nrm, anc, rms = pr.refit(n_fit, m, s1, constraint, axis, nrm0, anchor)
        wants.append([int(done)] + [int(v) for v in pr.b32(nrm)] + [int(v) for v in pr.b32(anc)] + [int(pr.b64(rms)[0]), int(pr.b64(pr.offset(nrm, anc))[0])])
        if done and n > 50:
            assert abs(abs(float(nrm[2])) - 1.0 / math.sqrt(1.0 + tilt[0] ** 2 + tilt[1] ** 2)) < 1e-3 and 0.005 < rms < 0.02
            assert (nrm[2] < 0) == (axis[2] < 0)
    got = [[int(x) for x in r.split()] for r in emu(reqs)]
    assert got == wants
    assert {w[0] for w in wants} == {0, 1}


# ---- plane_rule against the table
def _fields(text):
    out = {}
    for tok in text.split():
        k, v = tok.split("=")
        vals = [int(x) for x in v.split(",")]
        out[k] = vals if len(vals) > 1 else vals[0]
    return out


@pytest.fixture(scope="module")
def answers(emu):
    rows = emu([pc.line(c) for c in pc.CASES])
    out = {}
    for c, row in zip(pc.CASES, rows):
        code, msg, rule = row.split("\t")
        out[c["name"]] = (int(code), msg, _fields(rule))
    assert len(out) == len(pc.CASES)   # (names are unique)
    return out


def test_every_case_answers_with_its_code_and_message(answers):
    for c in pc.CASES:
        code, msg, _ = answers[c["name"]]
        assert (code, msg) == (c["rc"], c["msg"] or ""), c["name"]


def test_every_accepted_case_resolves_to_the_rule_libm_forms(answers):
    n = 0
    for c in pc.CASES:
        if c["rc"] == pc.LV_OK:
            assert answers[c["name"]][2] == pc.expected_rule(c), c["name"]
            n += 1
    assert n >= 15
    q = pc.expected_rule(next(c for c in pc.CASES if c["name"] == "constraint_walls"))
    ax = np.array(q["axis"], np.uint64).view(np.float64)
    assert abs(float(ax @ ax) - 1.0) < 1e-15 and q["sin_max"] == pc.b64(math.sin(float(F(0.3)))) != pc.b64(math.sin(0.3))


def test_every_refusal_of_the_rule_is_reached_and_every_float_meets_nan_and_the_infinities(answers):
    src = open(HEADER).read()
    body = src[src.index("inline int plane_rule"):src.index("// ---- the draws")]
    formats = re.findall(r'set_error\("((?:[^"\\]|\\.)*)"', body)
    assert len(formats) == body.count("set_error(") == 8
    messages = [m for code, m, _ in answers.values() if code != pc.LV_OK]
    for f in formats:
        pat = "^" + ".*".join(re.escape(s) for s in re.split(r"%(?:zu|d|g|s|u)", f)) + "$"
        assert any(re.match(pat, m) for m in messages), f
    floats = [(k, i) for k, kind in pc.FIELDS.items() if kind[0] == "f" for i in range(int(kind[1:] or 1))]
    assert floats == [("distance", 0), ("axis", 0), ("axis", 1), ("axis", 2), ("max_angle", 0)]
    for k, i in floats:
        for value in (pc.NAN, pc.INF, -pc.INF):
            def meets(c):
                v = c["over"].get(k)
                v = v if isinstance(v, list) else [v]
                return len(v) > i and v[i] is not None and repr(float(v[i])) == repr(value)
            assert any(c["rc"] == pc.LV_EINVAL and not c["two"] and meets(c) for c in pc.CASES), (k, i, value)


def test_defaults_and_geometry(emu):
    fields, geometry = emu(["defaults", "geometry"])
    want = {k: [int(x) for x in pc._encode(pc.FIELDS[k], v).split(",")] for k, v in pc.DEFAULTS.items()}
    assert _fields(fields) == {k: v if len(v) > 1 else v[0] for k, v in want.items()}
    assert pc.DEFAULTS == {**pr.DEFAULTS, "axis": list(pr.DEFAULTS["axis"])}
    assert abs(math.degrees(pc.DEFAULTS["max_angle"]) - 10.0) < 1e-5
    # the binding's copy of the scoring kernel's geometry (the GPU test sizes its edge cases by it) without loading the library
    capi_src = open(os.path.join(ROOT, "limo-velo_amd", "capi.py")).read()
    chunk, tile = re.search(r"PLANE_CHUNK, PLANE_TILE = (\d+), (\d+)", capi_src).groups()
    assert [int(x) for x in geometry.split()][:2] == [int(chunk), int(tile)]
    assert 2**44 * 256 * int(geometry.split()[2]) < 2**63   # a refit workgroup's int64 sums cannot overflow


def test_a_misspelt_field_is_an_error_not_a_default(emu):
    with pytest.raises(AssertionError, match="nothing reads distnace"):
        emu(["rule distnace=3"])
