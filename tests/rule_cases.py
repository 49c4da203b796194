"""The argument rules of the map tools (limo-velo_amd/csrc/lv_rules.hpp) as one table of cases: what each call is given, the code
and the message it must answer with, and for an accepted call every field of the resolved rule.  tests/test_rules_host.py holds the
header to it (g++, ASan / UBSan, tests/emu/rules_emu.cpp), tests/test_gpu_rules.py holds the entry points of the built library to it.

Nothing here comes from the code under test: the messages are written out from the format strings of the entry points as they stood
before the rules moved, with the values filled in, and the resolved fields are formed with numpy (f32 / f64 as the rule states them).

A case: tool, over (fields set on the tool's defaults), views (fields set on a valid default view each), n_views (default: the number
of views), null (the arguments passed as NULL), rc, msg, and where: "both", "host" (an accepted call whose views name more returns
than there is memory behind the pointer: the device test must not run it) or "api" (a check that stayed in lv_api.hip), and two: the
call is wrong in two ways and the message is the first refusal's."""
import numpy as np

F = np.float32
NAN, INF = float("nan"), float("inf")
LV_OK, LV_EINVAL, LV_ESTATE = 0, -1, -4
RETURNS = 0xFFFFFFF0            # lv_map_remove_dynamic: returns of one view / of all views
RETURNS_OCC = 0xFFFFFFF0 // 4   # lv_occ_integrate, lv_occ_view_gain

# field -> kind: i (int), u (uint32), z (size_t), p (pointer: 0 NULL, 1 valid), f / d (f32 / f64), with a count for arrays
FIELDS = {
    "vis": dict(width="i", height="i", v_min_deg="f", v_max_deg="f", min_range="f", max_range="f", margin_abs="f", margin_rel="f", window="i",
                min_hits="i", dry_run="i"),
    "normals": dict(k="i", max_dist="f", min_neighbours="i", orient="i", viewpoint="d3"),
    "outliers": dict(mode="i", k="i", max_dist="f", std_mul="f", radius="f", min_neighbours="i", dry_run="i"),
    "cluster": dict(radius="f", min_size="u", max_size="u", dry_run="i"),
    "paint": dict(min_depth="f", max_depth="f", max_norm_radius="f", zbuf_scale="i", window="i", margin_abs="f", margin_rel="f", blend="i"),
    "place_params": dict(n_rings="i", n_sectors="i", rmin="f", rmax="f", z_offset="f"),
    "place_state": dict(x="d26"),
    "place_centres": dict(centres="d*"),
    "place_query": dict(k="i"),
    "place_add_map": dict(n="z"),
    "integrate": {},
    "gain": {},
}
VIEW_FIELDS = dict(R="f9", t="f3", points="p", stride="z", n="z")
CAMERA_FIELDS = dict(R="f9", t="f3", fx="f", fy="f", cx="f", cy="f", dist="f5", width="i", height="i", format="i", image="p", row_stride="z")
RGB, BGR, MONO = 0, 1, 2
EYE = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
VIEW = dict(R=EYE, t=[0.0, 0.0, 0.0], points=0, stride=12, n=0)
CAMERA = dict(R=EYE, t=[0.0, 0.0, 0.0], fx=1.0, fy=1.0, cx=0.0, cy=0.0, dist=[0.0] * 5, width=4, height=4, format=RGB, image=1, row_stride=12)
STATE = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] + [0.0] * 15

# The defaults of lv_default_*_params, as include/limovelo_hip.h states them (and tests/test_map_*_abi.py, tests/test_place_abi.py assert)
DEFAULTS = {
    "vis": dict(width=2048, height=64, v_min_deg=-25.0, v_max_deg=3.0, min_range=1.0, max_range=80.0, margin_abs=0.3, margin_rel=0.02, window=1,
                min_hits=1, dry_run=0),
    "normals": dict(k=10, max_dist=2.0, min_neighbours=5, orient=0, viewpoint=[0.0, 0.0, 0.0]),
    "outliers": dict(mode=0, k=10, max_dist=2.0, std_mul=2.0, radius=0.5, min_neighbours=5, dry_run=0),
    "cluster": dict(radius=0.5, min_size=1, max_size=0, dry_run=0),
    "paint": dict(min_depth=0.3, max_depth=60.0, max_norm_radius=1.5, zbuf_scale=4, window=1, margin_abs=0.1, margin_rel=0.01, blend=0),
    "place_params": dict(n_rings=20, n_sectors=60, rmin=0.0, rmax=80.0, z_offset=2.0),
    "place_state": dict(x=STATE),
    "place_centres": dict(centres=[1.0, 2.0, 3.0, -4.0, 5.0, 6.5]),
    "place_query": dict(k=1),
    "place_add_map": dict(n=1),
    "integrate": {},
    "gain": {},
}
VIEW_TOOLS = {"vis": (VIEW, VIEW_FIELDS), "integrate": (VIEW, VIEW_FIELDS), "gain": (VIEW, VIEW_FIELDS), "paint": (CAMERA, CAMERA_FIELDS)}


def b32(x):
    return int(np.asarray(x, F).reshape(1).view(np.uint32)[0])


def b64(x):
    return int(np.asarray(x, np.float64).reshape(1).view(np.uint64)[0])


def params_of(case):
    return {**DEFAULTS[case["tool"]], **case["over"]}


def views_of(case):
    if case["tool"] not in VIEW_TOOLS:
        return []
    base = VIEW_TOOLS[case["tool"]][0]
    return [{**base, **v} for v in case["views"]]


def n_views_of(case):
    return len(case["views"]) if case["n_views"] is None else case["n_views"]


# ---- the resolved rules, with numpy
def vis_rule(p, n_views):
    rad = np.pi / 180.0
    lo, hi = np.float64(F(p["v_min_deg"])), np.float64(F(p["v_max_deg"]))
    return dict(width=p["width"], height=p["height"], n_views=n_views, window=p["window"], min_hits=p["min_hits"],
                inv_col=b32(F(np.float64(p["width"]) / (2.0 * np.pi))), v_min=b32(F(lo * rad)), inv_row=b32(F(np.float64(p["height"]) / ((hi - lo) * rad))),
                min_range=b32(p["min_range"]), max_range=b32(p["max_range"]), margin_abs=b32(p["margin_abs"]), margin_rel=b32(p["margin_rel"]))


def surf_rule(job=0, k=0, min_neighbours=0, orient=0, max_dist=0.0, std_mul=0.0, viewpoint=(0.0, 0.0, 0.0), threshold=0.0, fixed_threshold=0):
    return dict(job=job, k=k, min_neighbours=min_neighbours, orient=orient, max_dist=b32(max_dist), std_mul=b32(std_mul),
                viewpoint=[b64(v) for v in viewpoint], threshold=b64(threshold), fixed_threshold=fixed_threshold)


def normals_rule(p):
    return surf_rule(job=0, k=p["k"], min_neighbours=p["min_neighbours"], orient=p["orient"], max_dist=p["max_dist"], viewpoint=p["viewpoint"])


def outlier_rule(p):
    if p["mode"] == 0:
        return surf_rule(job=1, k=p["k"] + 1, max_dist=p["max_dist"], std_mul=p["std_mul"])
    return surf_rule(job=2, k=0, max_dist=p["radius"], min_neighbours=p["min_neighbours"], threshold=float(p["min_neighbours"]), fixed_threshold=1)


def cluster_rule(p):
    return dict(radius=b32(p["radius"]), min_size=p["min_size"], max_size=p["max_size"], seeded=0)


def paint_rule(p, views):
    s = p["zbuf_scale"]
    cams, pixels, cells, raw = [], 0, 0, 0
    for w in views:
        cw, ch = -(-w["width"] // s), -(-w["height"] // s)
        row = w["width"] * (1 if w["format"] == MONO else 3)
        d = w["dist"]
        cams.append(dict(R=[b32(v) for v in w["R"]], t=[b32(v) for v in w["t"]], fx=b32(w["fx"]), fy=b32(w["fy"]), cx=b32(w["cx"]), cy=b32(w["cy"]),
                         k1=b32(d[0]), k2=b32(d[1]), p1=b32(d[2]), p2=b32(d[3]), k3=b32(d[4]), wm1=b32(F(w["width"] - 1)), hm1=b32(F(w["height"] - 1)),
                         width=w["width"], height=w["height"], cw=cw, ch=ch, format=w["format"], tex_off=pixels, cell_off=cells, raw_off=raw, pad=0))
        pixels += w["width"] * w["height"]
        cells += cw * ch
        raw += (row * w["height"] + 255) // 256 * 256
    rule = dict(n_views=len(views), window=p["window"], blend=p["blend"], min_depth=b32(p["min_depth"]), max_depth=b32(p["max_depth"]),
                r2_max=b32(F(p["max_norm_radius"]) * F(p["max_norm_radius"])), s=b32(F(s)), margin_abs=b32(p["margin_abs"]), margin_rel=b32(p["margin_rel"]),
                max_pixels=max(w["width"] * w["height"] for w in views), max_cells=max(c["cw"] * c["ch"] for c in cams), total_pixels=pixels,
                total_cells=cells, raw_bytes=raw)
    return rule, cams


def expected_rule(case):
    """(rule, cams) of an accepted case: dicts of ints (floats as bit patterns), cams only for the paint rule."""
    p, tool = params_of(case), case["tool"]
    if tool == "vis":
        return vis_rule(p, n_views_of(case)), []
    if tool == "normals":
        return normals_rule(p), []
    if tool == "outliers":
        return outlier_rule(p), []
    if tool == "cluster":
        return cluster_rule(p), []
    if tool == "paint":
        return paint_rule(p, views_of(case)[:n_views_of(case)])
    return {}, []


CASES = []


def case(name, tool, rc, msg, over=None, views=None, n_views=None, null=(), where="both", two=False):
    assert name not in [c["name"] for c in CASES], name
    if views is None:
        views = [{}] if tool in VIEW_TOOLS else []
    CASES.append(dict(name=name, tool=tool, rc=rc, msg=msg, over=over or {}, views=views, n_views=n_views, null=tuple(null), where=where, two=two))


def ok(name, tool, **kw):
    case(name, tool, LV_OK, None, **kw)


def bad(name, tool, msg, **kw):
    case(name, tool, LV_EINVAL, msg, **kw)


PTS = dict(points=1, n=1)   # one return behind a valid pointer

# ---- the shared view check, in its three settings
for tool, pre, lim in (("vis", "", RETURNS), ("integrate", "", RETURNS_OCC), ("gain", "lv_occ_view_gain: ", RETURNS_OCC)):
    ok(f"{tool}_default_view", tool)
    ok(f"{tool}_two_views_with_returns", tool, views=[PTS, dict(points=1, n=2, stride=16)])
    ok(f"{tool}_null_points_without_returns", tool, views=[dict(points=0, n=0, stride=0)])
    for i, v in ((0, NAN), (4, INF), (8, -INF)):
        R = list(EYE)
        R[i] = v
        bad(f"{tool}_R{i}_{v}", tool, f"{pre}view 1: non-finite R", views=[PTS, dict(R=R)])
    bad(f"{tool}_null_points", tool, f"{pre}view 0: bad point array (stride 12)", views=[dict(points=0, n=1)])
    bad(f"{tool}_stride_11", tool, f"{pre}view 2: bad point array (stride 11)", views=[{}, PTS, dict(points=1, n=1, stride=11)])
    ok(f"{tool}_stride_12", tool, views=[dict(points=1, n=1, stride=12)])
    ok(f"{tool}_returns_at_limit", tool, views=[dict(points=1, n=lim)], where="host")
    bad(f"{tool}_returns_over_limit", tool, f"{pre}too many returns", views=[dict(points=1, n=lim + 1)])
    ok(f"{tool}_total_at_limit", tool, views=[dict(points=1, n=lim - 5), {}, dict(points=1, n=5)], where="host")
    bad(f"{tool}_total_over_limit", tool, f"{pre}too many returns", views=[dict(points=1, n=lim - 5), {}, dict(points=1, n=6)])
    bad(f"{tool}_R_before_points", tool, f"{pre}view 0: non-finite R", views=[dict(R=[NAN] * 9, points=0, n=1)], two=True)
    bad(f"{tool}_view_0_before_view_1", tool, f"{pre}view 0: bad point array (stride 3)", views=[dict(points=1, n=1, stride=3), dict(R=[INF] * 9)], two=True)
for i, v in ((0, NAN), (1, INF), (2, -INF)):
    t = [0.0, 0.0, 0.0]
    t[i] = v
    bad(f"vis_t{i}_{v}", "vis", "view 1: non-finite t", views=[PTS, dict(t=t)])
    ok(f"integrate_t{i}_{v}", "integrate", views=[PTS, dict(t=t, **PTS)])   # (a far or non-finite origin is the walk's business)
    ok(f"gain_t{i}_{v}", "gain", views=[PTS, dict(t=t, **PTS)])
bad("vis_R_before_t", "vis", "view 0: non-finite R", views=[dict(R=[NAN] * 9, t=[NAN] * 3)], two=True)
bad("vis_t_before_points", "vis", "view 0: non-finite t", views=[dict(t=[0.0, NAN, 0.0], points=0, n=3)], two=True)
# (what lv_occ_integrate / lv_occ_view_gain judge themselves before the views)
bad("integrate_null_views", "integrate", "null argument", null=["views"], where="api")
bad("integrate_n_views_0", "integrate", "n_views = 0: must be in 1..32", n_views=0, where="api")
bad("integrate_n_views_33", "integrate", "n_views = 33: must be in 1..32", n_views=33, where="api")
ok("integrate_n_views_32", "integrate", views=[{}] * 32, where="api")
bad("gain_null_views", "gain", "lv_occ_view_gain: null argument", null=["views"], where="api")
bad("gain_null_gain", "gain", "lv_occ_view_gain: null argument", null=["gain"], where="api")
bad("gain_n_views_0", "gain", "lv_occ_view_gain: n_views = 0: must be in 1..32", n_views=0, where="api")
bad("gain_n_views_33", "gain", "lv_occ_view_gain: n_views = 33: must be in 1..32", n_views=33, where="api")
bad("gain_n_views_before_views", "gain", "lv_occ_view_gain: n_views = 40: must be in 1..32", n_views=40, views=[dict(R=[NAN] * 9)], where="api", two=True)

# ---- lv_map_remove_dynamic
ok("vis_defaults", "vis")
ok("vis_other_values", "vis", over=dict(width=1800, height=40, v_min_deg=-16.3, v_max_deg=15.1, min_range=0.7, max_range=120.5, margin_abs=0.25,
                                        margin_rel=0.013, window=3, min_hits=2, dry_run=1), views=[{}, PTS, {}])
ok("vis_odd_sizes", "vis", over=dict(width=1023, height=7, v_min_deg=-0.1, v_max_deg=0.1))
bad("vis_null_views", "vis", "null argument", null=["views"])
bad("vis_null_params", "vis", "null argument", null=["params"])
bad("vis_n_views_0", "vis", "n_views = 0: must be in 1..32", n_views=0)
ok("vis_n_views_32", "vis", views=[{}] * 32, over=dict(min_hits=32))
bad("vis_n_views_33", "vis", "n_views = 33: must be in 1..32", n_views=33)
bad("vis_width_0", "vis", "image of 0 x 64 pixels: both >= 1, at most 2^20 in all", over=dict(width=0))
bad("vis_height_0", "vis", "image of 2048 x 0 pixels: both >= 1, at most 2^20 in all", over=dict(height=0))
bad("vis_width_negative", "vis", "image of -1 x 64 pixels: both >= 1, at most 2^20 in all", over=dict(width=-1))
ok("vis_one_pixel", "vis", over=dict(width=1, height=1))
ok("vis_pixels_at_limit", "vis", over=dict(width=2048, height=512))
bad("vis_pixels_one_row_more", "vis", "image of 2048 x 513 pixels: both >= 1, at most 2^20 in all", over=dict(width=2048, height=513))
bad("vis_pixels_wrap_int", "vis", "image of 65536 x 65536 pixels: both >= 1, at most 2^20 in all", over=dict(width=65536, height=65536))
bad("vis_fov_empty", "vis", "vertical field of view [3, 3] deg: v_min_deg < v_max_deg inside [-90, 90]", over=dict(v_min_deg=3.0))
ok("vis_fov_whole", "vis", over=dict(v_min_deg=-90.0, v_max_deg=90.0))
bad("vis_v_min_below", "vis", "vertical field of view [-90.5, 3] deg: v_min_deg < v_max_deg inside [-90, 90]", over=dict(v_min_deg=-90.5))
bad("vis_v_max_above", "vis", "vertical field of view [-25, 90.5] deg: v_min_deg < v_max_deg inside [-90, 90]", over=dict(v_max_deg=90.5))
bad("vis_min_range_0", "vis", "ranges [0, 80]: finite, 0 < min_range < max_range", over=dict(min_range=0.0))
bad("vis_ranges_equal", "vis", "ranges [80, 80]: finite, 0 < min_range < max_range", over=dict(min_range=80.0))
ok("vis_ranges_tiny", "vis", over=dict(min_range=1e-30, max_range=2e-30))
bad("vis_margin_abs_0", "vis", "margins 0 m, 0.02: finite and > 0", over=dict(margin_abs=0.0))
bad("vis_margin_rel_0", "vis", "margins 0.3 m, 0: finite and > 0", over=dict(margin_rel=0.0))
bad("vis_window_negative", "vis", "window = -1: must be in 0..8", over=dict(window=-1))
ok("vis_window_0", "vis", over=dict(window=0))
ok("vis_window_8", "vis", over=dict(window=8))
bad("vis_window_9", "vis", "window = 9: must be in 0..8", over=dict(window=9))
bad("vis_min_hits_0", "vis", "min_hits = 0: must be in 1..n_views", over=dict(min_hits=0))
ok("vis_min_hits_n_views", "vis", over=dict(min_hits=3), views=[{}] * 3)
bad("vis_min_hits_over_n_views", "vis", "min_hits = 4: must be in 1..n_views", over=dict(min_hits=4), views=[{}] * 3)
# two faults: the first refusal wins
bad("vis_n_views_before_width", "vis", "n_views = 0: must be in 1..32", n_views=0, over=dict(width=0), two=True)
bad("vis_margin_before_view", "vis", "margins -1 m, 0.02: finite and > 0", over=dict(margin_abs=-1.0), views=[{}, dict(R=[NAN] * 9)], two=True)
bad("vis_min_hits_before_view", "vis", "min_hits = 3: must be in 1..n_views", over=dict(min_hits=3), views=[{}, dict(t=[INF] * 3)], two=True)
bad("vis_width_before_fov_before_window", "vis", "image of 0 x 64 pixels: both >= 1, at most 2^20 in all", over=dict(width=0, v_min_deg=NAN, window=9), two=True)
bad("vis_null_before_n_views", "vis", "null argument", null=["params"], n_views=0, two=True)

# ---- lv_map_normals
ok("normals_defaults", "normals")
ok("normals_other_values", "normals", over=dict(k=17, max_dist=0.35, min_neighbours=4, orient=1, viewpoint=[1.5, -2.25e10, 1e-300]))
bad("normals_null", "normals", "null argument", null=["params"])
bad("normals_k_1", "normals", "k = 1: must be in 2..32", over=dict(k=1))
bad("normals_k_2_passes_the_k_check", "normals", "min_neighbours = 3: must be in 3..k", over=dict(k=2, min_neighbours=3))
ok("normals_k_3", "normals", over=dict(k=3, min_neighbours=3))
ok("normals_k_32", "normals", over=dict(k=32, min_neighbours=32))
bad("normals_k_33", "normals", "k = 33: must be in 2..32", over=dict(k=33))
bad("normals_max_dist_0", "normals", "max_dist = 0: finite and > 0", over=dict(max_dist=0.0))
bad("normals_min_neighbours_2", "normals", "min_neighbours = 2: must be in 3..k", over=dict(min_neighbours=2))
ok("normals_min_neighbours_k", "normals", over=dict(min_neighbours=10))
bad("normals_min_neighbours_over_k", "normals", "min_neighbours = 11: must be in 3..k", over=dict(min_neighbours=11))
bad("normals_orient_negative", "normals", "orient = -1: 0 or 1", over=dict(orient=-1))
bad("normals_orient_2", "normals", "orient = 2: 0 or 1", over=dict(orient=2))
for i, v in ((0, NAN), (1, INF), (2, -INF)):
    vp = [0.0, 0.0, 0.0]
    vp[i] = v
    bad(f"normals_viewpoint{i}_{v}", "normals", "non-finite viewpoint", over=dict(viewpoint=vp))
bad("normals_k_before_max_dist", "normals", "k = 0: must be in 2..32", over=dict(k=0, max_dist=-1.0), two=True)
bad("normals_max_dist_before_orient", "normals", "max_dist = -1: finite and > 0", over=dict(max_dist=-1.0, orient=5, viewpoint=[NAN] * 3), two=True)

# ---- lv_map_remove_outliers
ok("outliers_defaults", "outliers")
ok("outliers_statistical", "outliers", over=dict(k=7, max_dist=1.25, std_mul=-0.5, radius=NAN, min_neighbours=-3, dry_run=1))   # (mode 0 reads neither)
ok("outliers_radius", "outliers", over=dict(mode=1, radius=0.3, min_neighbours=4, k=-5, max_dist=NAN, std_mul=INF))              # (mode 1 reads none of these)
bad("outliers_null", "outliers", "null argument", null=["params"])
bad("outliers_k_0", "outliers", "k = 0: must be in 1..31", over=dict(k=0))
ok("outliers_k_1", "outliers", over=dict(k=1))
ok("outliers_k_31", "outliers", over=dict(k=31))
bad("outliers_k_32", "outliers", "k = 32: must be in 1..31", over=dict(k=32))
bad("outliers_max_dist_0", "outliers", "max_dist = 0: finite and > 0", over=dict(max_dist=0.0))
bad("outliers_radius_0", "outliers", "radius = 0: finite and > 0", over=dict(mode=1, radius=0.0))
bad("outliers_min_neighbours_0", "outliers", "min_neighbours = 0: must be >= 1", over=dict(mode=1, min_neighbours=0))
ok("outliers_min_neighbours_1", "outliers", over=dict(mode=1, min_neighbours=1))
bad("outliers_mode_2", "outliers", "mode = 2: 0 (statistical) or 1 (radius)", over=dict(mode=2))
bad("outliers_mode_negative", "outliers", "mode = -1: 0 (statistical) or 1 (radius)", over=dict(mode=-1))
bad("outliers_k_before_max_dist", "outliers", "k = 40: must be in 1..31", over=dict(k=40, max_dist=0.0, std_mul=NAN), two=True)
bad("outliers_radius_before_min_neighbours", "outliers", "radius = -2: finite and > 0", over=dict(mode=1, radius=-2.0, min_neighbours=0), two=True)

# ---- lv_map_cluster / lv_map_remove_clusters
ok("cluster_defaults", "cluster")
ok("cluster_other_values", "cluster", over=dict(radius=0.125, min_size=30, max_size=0xFFFFFFFF, dry_run=1))
ok("cluster_max_below_min", "cluster", over=dict(min_size=9, max_size=2))   # (not judged: nothing is reported)
bad("cluster_null", "cluster", "null argument", null=["params"])
bad("cluster_radius_0", "cluster", "radius = 0: finite and > 0", over=dict(radius=0.0))
bad("cluster_radius_negative", "cluster", "radius = -0.5: finite and > 0", over=dict(radius=-0.5))
bad("cluster_min_size_0", "cluster", "min_size = 0: must be >= 1", over=dict(min_size=0))
bad("cluster_radius_before_min_size", "cluster", "radius = nan: finite and > 0", over=dict(radius=NAN, min_size=0), two=True)

# ---- lv_map_paint
THREE = [dict(width=5, height=3, format=RGB, row_stride=15, R=[0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0], t=[1.0, -2.0, 0.5], fx=410.5, fy=409.25,
              cx=2.1, cy=1.2, dist=[-0.3, 0.1, 0.001, -0.002, 0.01]),
         dict(width=4, height=4, format=MONO, row_stride=4, fx=3.0, fy=3.5, cx=1.5, cy=1.75),
         dict(width=7, height=2, format=BGR, row_stride=24, t=[-3.0, 0.0, 7.0], dist=[0.0, 0.0, 0.0, 0.0, 0.25])]
ok("paint_defaults", "paint")
ok("paint_three_views", "paint", over=dict(zbuf_scale=2, min_depth=0.5, max_depth=33.3, max_norm_radius=1.3, window=2, margin_abs=0.07, margin_rel=0.004,
                                           blend=1), views=THREE)
ok("paint_raw_rounds_up_per_view", "paint", over=dict(zbuf_scale=3), views=[dict(width=100, height=3, row_stride=300), dict(width=1, height=1, format=MONO, row_stride=1),
                                                                           dict(width=86, height=1, format=BGR, row_stride=1000)])
bad("paint_null_views", "paint", "null argument", null=["views"])
bad("paint_null_params", "paint", "null argument", null=["params"])
bad("paint_n_views_0", "paint", "n_views = 0: must be in 1..32", n_views=0)
ok("paint_n_views_32", "paint", views=[{}] * 32)
bad("paint_n_views_33", "paint", "n_views = 33: must be in 1..32", n_views=33)
bad("paint_min_depth_0", "paint", "depths [0, 60]: finite, 0 < min_depth < max_depth", over=dict(min_depth=0.0))
bad("paint_depths_equal", "paint", "depths [60, 60]: finite, 0 < min_depth < max_depth", over=dict(min_depth=60.0))
bad("paint_max_norm_radius_0", "paint", "max_norm_radius = 0: finite and > 0", over=dict(max_norm_radius=0.0))
bad("paint_zbuf_scale_0", "paint", "zbuf_scale = 0: must be in 1..16", over=dict(zbuf_scale=0))
ok("paint_zbuf_scale_1", "paint", over=dict(zbuf_scale=1), views=THREE)
ok("paint_zbuf_scale_16", "paint", over=dict(zbuf_scale=16), views=THREE + [dict(width=33, height=17, row_stride=99)])
bad("paint_zbuf_scale_17", "paint", "zbuf_scale = 17: must be in 1..16", over=dict(zbuf_scale=17))
bad("paint_window_negative", "paint", "window = -1: must be in 0..8", over=dict(window=-1))
ok("paint_window_0", "paint", over=dict(window=0))
ok("paint_window_8", "paint", over=dict(window=8))
bad("paint_window_9", "paint", "window = 9: must be in 0..8", over=dict(window=9))
bad("paint_margin_abs_0", "paint", "margins 0 m, 0.01: finite and > 0", over=dict(margin_abs=0.0))
bad("paint_margin_rel_0", "paint", "margins 0.1 m, 0: finite and > 0", over=dict(margin_rel=0.0))
bad("paint_blend_negative", "paint", "blend = -1: must be 0 or 1", over=dict(blend=-1))
ok("paint_blend_1", "paint", over=dict(blend=1))
bad("paint_blend_2", "paint", "blend = 2: must be 0 or 1", over=dict(blend=2))
for i, v in ((0, NAN), (5, INF), (8, -INF)):
    R = list(EYE)
    R[i] = v
    bad(f"paint_R{i}_{v}", "paint", "view 1: non-finite R", views=[{}, dict(R=R)])
for i, v in ((0, NAN), (1, INF), (2, -INF)):
    t = [0.0, 0.0, 0.0]
    t[i] = v
    bad(f"paint_t{i}_{v}", "paint", "view 0: non-finite t", views=[dict(t=t)])
for i, v in ((0, NAN), (1, INF), (2, -INF), (3, NAN), (4, INF)):
    d = [0.0] * 5
    d[i] = v
    bad(f"paint_dist{i}_{v}", "paint", "view 0: non-finite distortion", views=[dict(dist=d)])
bad("paint_width_0", "paint", "view 0: image of 0 x 4 pixels: each side 1..8192, at most 2^24 in all", views=[dict(width=0)])
bad("paint_height_0", "paint", "view 1: image of 4 x 0 pixels: each side 1..8192, at most 2^24 in all", views=[{}, dict(height=0)])
ok("paint_width_8192", "paint", views=[dict(width=8192, height=1, row_stride=3 * 8192)])
bad("paint_width_8193", "paint", "view 0: image of 8193 x 1 pixels: each side 1..8192, at most 2^24 in all", views=[dict(width=8193, height=1, row_stride=3 * 8193)])
ok("paint_height_8192", "paint", views=[dict(width=1, height=8192, row_stride=3)])
bad("paint_height_8193", "paint", "view 0: image of 1 x 8193 pixels: each side 1..8192, at most 2^24 in all", views=[dict(width=1, height=8193, row_stride=3)])
ok("paint_pixels_at_limit", "paint", views=[dict(width=8192, height=2048, format=MONO, row_stride=8192)])
bad("paint_pixels_one_row_more", "paint", "view 0: image of 8192 x 2049 pixels: each side 1..8192, at most 2^24 in all",
    views=[dict(width=8192, height=2049, format=MONO, row_stride=8192)])
bad("paint_format_3", "paint", "view 0: format 3", views=[dict(format=3)])
bad("paint_format_negative", "paint", "view 0: format -1", views=[dict(format=-1)])
bad("paint_null_image", "paint", "view 1: null image or row_stride 12 < 12", views=[{}, dict(image=0)])
bad("paint_row_stride_rgb", "paint", "view 0: null image or row_stride 11 < 12", views=[dict(row_stride=11)])
bad("paint_row_stride_bgr", "paint", "view 0: null image or row_stride 11 < 12", views=[dict(row_stride=11, format=BGR)])
ok("paint_row_stride_mono", "paint", views=[dict(row_stride=4, format=MONO)])
bad("paint_row_stride_mono_short", "paint", "view 0: null image or row_stride 3 < 4", views=[dict(row_stride=3, format=MONO)])
BIG = dict(width=8192, height=2048, format=MONO, row_stride=8192)   # 2^24 pixels
ok("paint_total_at_limit", "paint", views=[BIG] * 4)
bad("paint_total_over_limit", "paint", "the views hold more than 2^26 pixels together", views=[BIG] * 4 + [dict(width=1, height=1)])
bad("paint_n_views_before_depths", "paint", "n_views = 99: must be in 1..32", n_views=99, over=dict(min_depth=-1.0), two=True)
bad("paint_zbuf_before_blend_before_view", "paint", "zbuf_scale = 0: must be in 1..16", over=dict(zbuf_scale=0, blend=7), views=[dict(R=[NAN] * 9)], two=True)
bad("paint_blend_before_view", "paint", "blend = 7: must be 0 or 1", over=dict(blend=7), views=[dict(R=[NAN] * 9)], two=True)
bad("paint_view_0_format_before_view_1_R", "paint", "view 0: format 9", views=[dict(format=9), dict(R=[NAN] * 9)], two=True)
bad("paint_t_before_size", "paint", "view 0: non-finite t", views=[dict(t=[NAN] * 3, width=0)], two=True)

# ---- lv_place_configure
ok("place_defaults", "place_params")
bad("place_null", "place_params", "null argument", null=["params"])
bad("place_n_rings_0", "place_params", "n_rings = 0: must be in 1..32", over=dict(n_rings=0))
ok("place_n_rings_1", "place_params", over=dict(n_rings=1))
ok("place_n_rings_32", "place_params", over=dict(n_rings=32))
bad("place_n_rings_33", "place_params", "n_rings = 33: must be in 1..32", over=dict(n_rings=33))
bad("place_n_sectors_1", "place_params", "n_sectors = 1: must be in 2..64", over=dict(n_sectors=1))
ok("place_n_sectors_2", "place_params", over=dict(n_sectors=2))
ok("place_n_sectors_64", "place_params", over=dict(n_sectors=64))
bad("place_n_sectors_65", "place_params", "n_sectors = 65: must be in 2..64", over=dict(n_sectors=65))
bad("place_rmin_negative", "place_params", "rmin -0.5, rmax 80: finite, 0 <= rmin < rmax <= 1000", over=dict(rmin=-0.5))
bad("place_radii_equal", "place_params", "rmin 80, rmax 80: finite, 0 <= rmin < rmax <= 1000", over=dict(rmin=80.0))
ok("place_rmax_1000", "place_params", over=dict(rmax=1000.0))
bad("place_rmax_just_above_1000", "place_params", "rmin 0, rmax 1000: finite, 0 <= rmin < rmax <= 1000", over=dict(rmax=float(np.nextafter(F(1000.0), F(INF)))))
bad("place_rmax_1001", "place_params", "rmin 0, rmax 1001: finite, 0 <= rmin < rmax <= 1000", over=dict(rmax=1001.0))
ok("place_z_offset_negative", "place_params", over=dict(z_offset=-1.5))
bad("place_n_rings_before_rmax", "place_params", "n_rings = 40: must be in 1..32", over=dict(n_rings=40, rmax=-1.0, z_offset=NAN), two=True)

# ---- the state of lv_place_describe / lv_place_add_scan / lv_place_query, the centres of lv_place_add_map / lv_place_load
ok("place_state_ok", "place_state")
bad("place_state_null", "place_state", "null state", null=["state"])
for i, v in ((0, NAN), (6, INF), (13, -INF), (25, NAN)):
    x = list(STATE)
    x[i] = v
    bad(f"place_state{i}_{v}", "place_state", "non-finite state", over=dict(x=x))
ok("place_centres_ok", "place_centres")
bad("place_centres_x_nan", "place_centres", "centre 0 is not finite", over=dict(centres=[NAN, 0.0, 0.0, 1.0, 1.0, 1.0]))
bad("place_centres_z_inf", "place_centres", "centre 1 is not finite", over=dict(centres=[0.0, 0.0, 0.0, 1.0, 1.0, INF]))
bad("place_centres_y_minus_inf", "place_centres", "centre 2 is not finite", over=dict(centres=[0.0] * 6 + [1.0, -INF, 0.5]))
# (what lv_place_query and lv_place_add_map judge themselves)
bad("place_query_k_0", "place_query", "k = 0: must be in 1..64", over=dict(k=0), where="api")
bad("place_query_k_65", "place_query", "k = 65: must be in 1..64", over=dict(k=65), where="api")
case("place_query_k_1", "place_query", LV_ESTATE, "the place database is empty", over=dict(k=1), where="api")
case("place_query_k_64", "place_query", LV_ESTATE, "the place database is empty", over=dict(k=64), where="api")
bad("place_add_map_n_0", "place_add_map", "n = 0: must be in 1..65536", over=dict(n=0), where="api")
bad("place_add_map_n_65537", "place_add_map", "n = 65537: must be in 1..65536", over=dict(n=65537), where="api")

# ---- every field judged for finiteness meets NaN, +inf and -inf, each as the call's only fault
# tool -> field -> (the message with the value's text left open, what else the case sets)
FINITE = {
    "vis": dict(v_min_deg=("vertical field of view [{}, 3] deg: v_min_deg < v_max_deg inside [-90, 90]", {}),
                v_max_deg=("vertical field of view [-25, {}] deg: v_min_deg < v_max_deg inside [-90, 90]", {}),
                min_range=("ranges [{}, 80]: finite, 0 < min_range < max_range", {}), max_range=("ranges [1, {}]: finite, 0 < min_range < max_range", {}),
                margin_abs=("margins {} m, 0.02: finite and > 0", {}), margin_rel=("margins 0.3 m, {}: finite and > 0", {})),
    "normals": dict(max_dist=("max_dist = {}: finite and > 0", {})),
    "outliers": dict(max_dist=("max_dist = {}: finite and > 0", {}), std_mul=("std_mul must be finite", {}), radius=("radius = {}: finite and > 0", dict(mode=1))),
    "cluster": dict(radius=("radius = {}: finite and > 0", {})),
    "paint": dict(min_depth=("depths [{}, 60]: finite, 0 < min_depth < max_depth", {}), max_depth=("depths [0.3, {}]: finite, 0 < min_depth < max_depth", {}),
                  max_norm_radius=("max_norm_radius = {}: finite and > 0", {}), margin_abs=("margins {} m, 0.01: finite and > 0", {}),
                  margin_rel=("margins 0.1 m, {}: finite and > 0", {})),
    "place_params": dict(rmin=("rmin {}, rmax 80: finite, 0 <= rmin < rmax <= 1000", {}), rmax=("rmin 0, rmax {}: finite, 0 <= rmin < rmax <= 1000", {}),
                         z_offset=("z_offset = {}: must be finite", {})),
}
# (the arrays meet the three values in the loops above, one element at a time)
FINITE_ARRAYS = {"normals": ["viewpoint"], "place_state": ["x"], "place_centres": ["centres"]}
FINITE_VIEW_ARRAYS = {"vis": ["R", "t"], "integrate": ["R"], "gain": ["R"], "paint": ["R", "t", "dist"]}
FINITE_VIEW = {"paint": ["fx", "fy", "cx", "cy"]}
NONFINITE = ((NAN, "nan"), (INF, "inf"), (-INF, "-inf"))
for tool, fields in FINITE.items():
    for f, (msg, also) in fields.items():
        for v, text in NONFINITE:
            bad(f"{tool}_{f}_{text}", tool, msg.format(text), over={**also, f: v})
for f in FINITE_VIEW["paint"]:
    for v, text in NONFINITE:
        bad(f"paint_{f}_{text}", "paint", "view 2: non-finite intrinsics", views=[{}, {}, {f: v}])


def _encode(kind, value):
    """a field's value as the emulation reads it: integers, floats as bit patterns, comma-separated"""
    vals = value if isinstance(value, (list, tuple)) else [value]
    enc = {"f": b32, "d": b64}.get(kind[0], int)
    return ",".join(str(enc(v)) for v in vals)


def line(case):
    """the case as one line of the emulation's input"""
    tool = case["tool"]
    out = [tool] + [f"null_{a}=1" for a in case["null"]]
    for k, v in case["over"].items():
        out.append(f"{k}={_encode(FIELDS[tool][k], v)}")
    if tool in VIEW_TOOLS:
        fields = VIEW_TOOLS[tool][1]
        out.append(f"n_views={n_views_of(case)}")
        for i, view in enumerate(case["views"]):
            out += [f"v{i}.{k}={_encode(fields[k], v)}" for k, v in view.items()]
    return " ".join(out)
