"""The argument rule of lv_map_planes (plane_rule, limo-velo_amd/csrc/lv_planes.hpp) as a table of cases, in the style of
tests/rule_cases.py: what the call is given (fields set on the documented defaults), the code and the message it must answer with,
and for an accepted call every field of the resolved rule, formed here with Python floats and libm.  tests/test_planes_host.py
holds the header to it (g++, ASan / UBSan, tests/emu/planes_emu.cpp); tests/test_gpu_map_planes.py holds the entry point to it.

Nothing here comes from the code under test: the messages are written out from the rule as include/limovelo_hip.h states it.
two: the call is wrong in two ways and the message is the first refusal's."""
import math

import numpy as np

F = np.float32
NAN, INF = float("nan"), float("inf")
LV_OK, LV_EINVAL = 0, -1

FIELDS = dict(distance="f", iterations="u", max_planes="u", min_inliers="u", seed="q", constraint="i", axis="f3", max_angle="f", refine="i")
DEFAULTS = dict(distance=0.1, iterations=512, max_planes=1, min_inliers=100, seed=0, constraint=0, axis=[0.0, 0.0, 1.0],
                max_angle=float(F(10.0 * math.pi / 180.0)), refine=1)
HALF_PI_BELOW = float(np.nextafter(F(math.pi / 2), F(0)))   # the largest f32 below pi / 2 ((float)(pi / 2) itself lies above it)
HALF_PI_ABOVE = float(F(math.pi / 2))
TINY = float(np.nextafter(F(0), F(1)))                      # the smallest positive f32


def b32(x):
    return int(np.asarray(x, F).reshape(1).view(np.uint32)[0])


def b64(x):
    return int(np.asarray(x, np.float64).reshape(1).view(np.uint64)[0])


def g(x):
    """printf's %g of the f32 x (passed as a double)"""
    return "%g" % float(F(x))


def _encode(kind, v):
    if kind[0] == "f":
        vals = v if isinstance(v, (list, tuple)) else [v]
        return ",".join(str(b32(x)) for x in vals)
    return str(int(v) & ((1 << 64) - 1)) if kind == "q" else str(int(v))


def line(case):
    if case.get("null"):
        return "rule null=1"
    return "rule " + " ".join(f"{k}={_encode(FIELDS[k], v)}" for k, v in case["over"].items())


def params_of(case):
    return {**DEFAULTS, **case["over"]}


def expected_rule(case):
    """the resolved PlaneRule of an accepted case, fields as the emu prints them"""
    p = params_of(case)
    axis, cm, sm = [0.0, 0.0, 0.0], 0.0, 0.0
    if p["constraint"] != 0:
        x, y, z = (float(F(v)) for v in p["axis"])
        ln = math.sqrt((x * x + y * y) + z * z)
        a = float(F(p["max_angle"]))
        axis, cm, sm = [x / ln, y / ln, z / ln], math.cos(a), math.sin(a)
    return dict(distance=b32(p["distance"]), iterations=p["iterations"], max_planes=p["max_planes"], min_inliers=p["min_inliers"],
                seed=p["seed"], constraint=p["constraint"], refine=1 if p["refine"] else 0, axis=[b64(v) for v in axis], cos_max=b64(cm),
                sin_max=b64(sm))


def ok(name, **over):
    return dict(name=name, over=over, rc=LV_OK, msg=None, two=False)


def bad(name, msg, two=False, **over):
    return dict(name=name, over=over, rc=LV_EINVAL, msg=msg, two=two)


def _axis_msg(a):
    return f"axis ({g(a[0])}, {g(a[1])}, {g(a[2])}): finite and non-zero"


CASES = [
    ok("defaults"),
    dict(name="null_params", over={}, null=True, rc=LV_EINVAL, msg="null argument", two=False),
    # distance: > 0, finite
    ok("distance_smallest", distance=TINY),
    ok("distance_largest", distance=float(np.finfo(F).max)),
    bad("distance_zero", "distance = 0: finite and > 0", distance=0.0),
    bad("distance_negative", "distance = -0.1: finite and > 0", distance=-0.1),
    bad("distance_nan", "distance = nan: finite and > 0", distance=NAN),
    bad("distance_inf", "distance = inf: finite and > 0", distance=INF),
    bad("distance_minus_inf", "distance = -inf: finite and > 0", distance=-INF),
    # iterations: 1..65536
    ok("iterations_low", iterations=1),
    ok("iterations_high", iterations=65536),
    bad("iterations_zero", "iterations = 0: must be in 1..65536", iterations=0),
    bad("iterations_above", "iterations = 65537: must be in 1..65536", iterations=65537),
    # max_planes: 1..32
    ok("max_planes_low", max_planes=1),
    ok("max_planes_high", max_planes=32),
    bad("max_planes_zero", "max_planes = 0: must be in 1..32", max_planes=0),
    bad("max_planes_above", "max_planes = 33: must be in 1..32", max_planes=33),
    # min_inliers: >= 3
    ok("min_inliers_low", min_inliers=3),
    ok("min_inliers_high", min_inliers=0xFFFFFFFF),
    bad("min_inliers_below", "min_inliers = 2: must be >= 3", min_inliers=2),
    # seed: any
    ok("seed_all_ones", seed=(1 << 64) - 1),
    # constraint: 0, 1, 2
    ok("constraint_floor", constraint=1),
    ok("constraint_walls", constraint=2, axis=[0.3, -0.4, 1.2], max_angle=0.3),
    bad("constraint_negative", "constraint = -1: 0 (none), 1 (along the axis) or 2 (perpendicular to it)", constraint=-1),
    bad("constraint_above", "constraint = 3: 0 (none), 1 (along the axis) or 2 (perpendicular to it)", constraint=3),
    # axis: judged with a constraint only; finite, non-zero
    ok("axis_unread_without_constraint", axis=[NAN, INF, 0.0], max_angle=NAN),
    ok("axis_tiny", constraint=1, axis=[0.0, TINY, 0.0]),
    ok("axis_huge", constraint=2, axis=[float(np.finfo(F).max)] * 3),
    bad("axis_zero", _axis_msg([0.0, 0.0, 0.0]), constraint=1, axis=[0.0, 0.0, 0.0]),
    bad("axis_minus_zero", _axis_msg([-0.0, 0.0, -0.0]), constraint=2, axis=[-0.0, 0.0, -0.0]),
    *[bad(f"axis_{i}_{n}", _axis_msg([v if j == i else 1.0 for j in range(3)]), constraint=1, axis=[v if j == i else 1.0 for j in range(3)])
      for i in range(3) for n, v in (("nan", NAN), ("inf", INF), ("minus_inf", -INF))],
    # max_angle: judged with a constraint only; inside (0, pi / 2)
    ok("max_angle_smallest", constraint=1, max_angle=TINY),
    ok("max_angle_largest", constraint=2, max_angle=HALF_PI_BELOW),
    bad("max_angle_zero", "max_angle = 0: must be inside (0, pi / 2)", constraint=1, max_angle=0.0),
    bad("max_angle_half_pi", f"max_angle = {g(HALF_PI_ABOVE)}: must be inside (0, pi / 2)", constraint=1, max_angle=HALF_PI_ABOVE),
    bad("max_angle_negative", "max_angle = -0.1: must be inside (0, pi / 2)", constraint=2, max_angle=-0.1),
    bad("max_angle_nan", "max_angle = nan: must be inside (0, pi / 2)", constraint=1, max_angle=NAN),
    bad("max_angle_inf", "max_angle = inf: must be inside (0, pi / 2)", constraint=1, max_angle=INF),
    bad("max_angle_minus_inf", "max_angle = -inf: must be inside (0, pi / 2)", constraint=2, max_angle=-INF),
    # refine: any int, resolved to 0 / 1
    ok("refine_off", refine=0),
    ok("refine_negative", refine=-7),
    # the first refusal wins
    bad("two_distance_then_iterations", "distance = nan: finite and > 0", two=True, distance=NAN, iterations=0),
    bad("two_iterations_then_planes", "iterations = 0: must be in 1..65536", two=True, iterations=0, max_planes=99),
    bad("two_constraint_then_axis", "constraint = 7: 0 (none), 1 (along the axis) or 2 (perpendicular to it)", two=True, constraint=7,
        axis=[0.0, 0.0, 0.0]),
    bad("two_axis_then_angle", _axis_msg([0.0, 0.0, 0.0]), two=True, constraint=1, axis=[0.0, 0.0, 0.0], max_angle=3.0),
]
