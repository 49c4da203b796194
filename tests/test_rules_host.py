"""The argument rules of the map tools (limo-velo_amd/csrc/lv_rules.hpp: what lv_map_remove_dynamic, lv_map_normals,
lv_map_remove_outliers, lv_map_cluster / lv_map_remove_clusters, lv_map_paint and lv_place_* refuse, the resolved rules they hand the
kernels, the view check they share with lv_occ_integrate / lv_occ_view_gain, and the lv_default_*) compiled with plain g++ and
-fsanitize=address,undefined and held to tests/rule_cases.py: tests/emu/rules_emu.cpp answers one case per line.  The code, the
message and every field of a resolved rule by equality, floats by their bits.  Nothing is loaded into Python."""
import os
import re
import subprocess

import pytest

import rule_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
HEADER = os.path.join(ROOT, "limo-velo_amd", "csrc", "lv_rules.hpp")
HOST_CASES = [c for c in rc.CASES if c["where"] != "api"]


def _fields(text):
    out = {}
    for tok in text.split():
        k, v = tok.split("=")
        vals = [int(x) for x in v.split(",")]
        out[k] = vals if len(vals) > 1 else vals[0]
    return out


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rules_host") / "rules_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(EMU_DIR, "rules_emu.cpp"), "-o", str(exe)])

    def run(lines):
        """[(rc, message, rule, cams)] of the input lines"""
        res = subprocess.run([str(exe)], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert res.returncode == 0, res.stderr.decode()[-2000:]
        rows = res.stdout.decode().split("\n")
        assert rows[-1] == "" and len(rows) == len(lines) + 1
        got = []
        for row in rows[:-1]:
            code, msg, *rest = row.split("\t")
            got.append((int(code), msg, _fields(rest[0]), [_fields(r) for r in rest[1:]]))
        return got

    return run


@pytest.fixture(scope="module")
def answers(emu):
    return dict(zip([c["name"] for c in HOST_CASES], emu([rc.line(c) for c in HOST_CASES])))


def test_every_case_answers_with_its_code_and_message(answers):
    for c in HOST_CASES:
        code, msg, _, _ = answers[c["name"]]
        assert (code, msg) == (c["rc"], c["msg"] or ""), c["name"]


def test_every_accepted_case_resolves_to_the_rule_numpy_forms(answers):
    seen = set()
    for c in HOST_CASES:
        if c["rc"] != rc.LV_OK:
            continue
        _, _, rule, cams = answers[c["name"]]
        want_rule, want_cams = rc.expected_rule(c)
        assert rule == want_rule, (c["name"], rule, want_rule)
        assert cams == want_cams, (c["name"], cams, want_cams)
        seen.add((c["tool"], rule.get("job")))
    assert {("vis", None), ("normals", 0), ("outliers", 1), ("outliers", 2), ("cluster", None), ("paint", None)} <= seen


def test_the_cases_decide_what_they_are_there_for():
    """On the table and numpy alone: the accepted cases make each clause of the resolved rules show."""
    by = {c["name"]: c for c in rc.CASES}
    rule, cams = rc.expected_rule(by["paint_three_views"])
    assert [(c["cw"], c["ch"]) for c in cams] == [(3, 2), (2, 2), (4, 1)]
    assert [c["tex_off"] for c in cams] == [0, 15, 31] and [c["cell_off"] for c in cams] == [0, 6, 10] and [c["raw_off"] for c in cams] == [0, 256, 512]
    assert (rule["max_pixels"], rule["max_cells"]) == (16, 6)            # the second view's pixels, the first view's cells
    assert (rule["total_pixels"], rule["total_cells"], rule["raw_bytes"]) == (45, 14, 768)
    assert rule["r2_max"] == rc.b32(rc.F(1.3) * rc.F(1.3)) != rc.b32(1.3 * 1.3) and rule["s"] == rc.b32(2.0)
    _, cams = rc.expected_rule(by["paint_raw_rounds_up_per_view"])
    assert [c["raw_off"] for c in cams] == [0, 1024, 1280]
    q, _ = rc.expected_rule(by["outliers_statistical"])
    assert (q["job"], q["k"], q["fixed_threshold"]) == (1, 8, 0)
    q, _ = rc.expected_rule(by["outliers_radius"])
    assert (q["job"], q["k"], q["min_neighbours"], q["threshold"], q["fixed_threshold"], q["max_dist"]) == (2, 0, 4, rc.b64(4.0), 1, rc.b32(0.3))
    q, _ = rc.expected_rule(by["vis_other_values"])
    assert q["inv_row"] != rc.b32(40.0 / ((15.1 - -16.3) * 3.141592653589793 / 180.0))   # (the degrees are f32 before they are f64)
    for tool in ("vis", "normals", "outliers", "cluster", "paint", "place_params"):
        assert any(c["tool"] == tool and c["two"] and c["rc"] != rc.LV_OK for c in rc.CASES), tool


def _meets(case, field, value, in_views):
    """the case sets the field (an element of it, for an array) to the value"""
    for fields in (case["views"] if in_views else [case["over"]]):
        got = fields.get(field, [])
        if any(repr(float(g)) == repr(value) for g in (got if isinstance(got, (list, tuple)) else [got])):
            return True
    return False


def test_every_field_judged_for_finiteness_meets_nan_and_both_infinities():
    """On the table alone: every float field of the tools' parameters and views is declared, and each declared one is set to NaN, to
    +inf and to -inf in a refused case that has no other fault.  t of the occupancy views is the one float not judged: accepted."""
    declared = {tool: sorted(list(f) + rc.FINITE_ARRAYS.get(tool, [])) for tool, f in rc.FINITE.items()}
    declared.update({tool: sorted(f) for tool, f in rc.FINITE_ARRAYS.items() if tool not in declared})
    floats = {tool: sorted(k for k, kind in f.items() if kind[0] in "fd") for tool, f in rc.FIELDS.items()}
    assert declared == {tool: f for tool, f in floats.items() if f}
    view_floats = sorted(k for k, kind in rc.CAMERA_FIELDS.items() if kind[0] in "fd")
    assert sorted(rc.FINITE_VIEW["paint"] + rc.FINITE_VIEW_ARRAYS["paint"]) == view_floats and rc.FINITE_VIEW_ARRAYS["vis"] == ["R", "t"]
    wanted = [(tool, f, False) for tool, fields in declared.items() for f in fields]
    wanted += [(tool, f, True) for tool, fields in list(rc.FINITE_VIEW.items()) + list(rc.FINITE_VIEW_ARRAYS.items()) for f in fields]
    assert len(wanted) == 33
    for tool, field, in_views in wanted:
        for value in (rc.NAN, rc.INF, -rc.INF):
            assert any(c["tool"] == tool and c["rc"] == rc.LV_EINVAL and not c["two"] and _meets(c, field, value, in_views) for c in rc.CASES), (tool, field, value)
    for tool in ("integrate", "gain"):
        for value in (rc.NAN, rc.INF, -rc.INF):
            assert any(c["tool"] == tool and c["rc"] == rc.LV_OK and _meets(c, "t", value, True) for c in rc.CASES), (tool, value)


def test_every_refusal_of_the_header_is_reached(answers):
    """Every set_error of lv_rules.hpp, as a pattern of its format string, matches the message of at least one refused case."""
    src = open(HEADER).read()
    formats = re.findall(r'set_error\("((?:[^"\\]|\\.)*)"', src)
    assert len(formats) == src.count("set_error(") - 1 >= 40   # (all but the declaration)
    messages = [m for code, m, _, _ in answers.values() if code != rc.LV_OK]
    for f in set(formats):
        pat = "^" + ".*".join(re.escape(s) for s in re.split(r"%(?:zu|d|g|s)", f)) + "$"
        assert any(re.match(pat, m) for m in messages), f


def test_defaults_are_the_documented_ones_and_pass_their_own_rule(emu, answers):
    tools = ("vis", "normals", "outliers", "cluster", "paint", "place_params")
    got = emu([f"defaults {t}" for t in tools])
    for tool, (code, _, fields, _) in zip(tools, got):
        want = {k: [int(x) for x in rc._encode(rc.FIELDS[tool][k], v).split(",")] for k, v in rc.DEFAULTS[tool].items()}
        want = {k: v if len(v) > 1 else v[0] for k, v in want.items()}
        assert code == 0 and fields == want, (tool, fields, want)
    for name in ("vis_defaults", "normals_defaults", "outliers_defaults", "cluster_defaults", "paint_defaults", "place_defaults"):
        c = next(c for c in rc.CASES if c["name"] == name)
        assert c["over"] == {} and answers[name][0] == rc.LV_OK
    d = rc.DEFAULTS   # (what tests/test_map_*_abi.py and tests/test_place_abi.py assert of the library's)
    assert (d["vis"]["width"], d["vis"]["height"], d["vis"]["window"], d["vis"]["min_hits"]) == (2048, 64, 1, 1)
    assert (d["paint"]["zbuf_scale"], d["paint"]["window"], d["paint"]["blend"], d["paint"]["max_depth"], d["paint"]["max_norm_radius"]) == (4, 1, 0, 60.0, 1.5)
    assert (d["place_params"]["n_rings"], d["place_params"]["n_sectors"], d["place_params"]["rmax"]) == (20, 60, 80.0)


def test_a_misspelt_field_is_an_error_not_a_default(emu):
    with pytest.raises(AssertionError, match="nothing reads widht"):
        emu(["vis widht=3"])
