"""The entry points of the built library against the table tests/test_rules_host.py holds lv_rules.hpp to (tests/rule_cases.py): for
every case the real call through ctypes, on one context with no map and no scan and an 8 x 8 x 4 occupancy grid, answers with the
table's code and leaves the table's message in lv_last_error().  An accepted call finds no map and returns LV_OK (the place calls
that want a scan or a database: LV_ESTATE with their own message, after the rule).  Nothing is launched for a refusal.

The cases marked "host" are left out: they are accepted with more returns named than there is memory behind the pointer, which
lv_occ_integrate / lv_occ_view_gain would go on to read."""
import ctypes as C

import numpy as np
import pytest

import rule_cases as rc

pytestmark = pytest.mark.gpu

NO_SCAN = (rc.LV_ESTATE, "no scan: call lv_scan_set first")
NO_PLACES = (rc.LV_ESTATE, "the place database is empty")


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def ctx(capi):
    with capi.Context() as c:
        c.occ_configure(capi.default_occupancy_params(origin=(-0.8, -0.8, -0.4), resolution=0.2, nx=8, ny=8, nz=4))
        yield c


def _set(obj, fields):
    for k, v in fields.items():
        if isinstance(v, (list, tuple)):
            getattr(obj, k)[:] = [float(x) for x in v]
        else:
            setattr(obj, k, v)
    return obj


class Calls:
    """One case -> the calls that judge it: [(what, code, message)]"""

    def __init__(self, capi, ctx):
        self.capi, self.lib, self.h = capi, ctx.lib, ctx.h
        self.memory = np.zeros(16, np.float32)          # what a valid pointer points at: two returns at any stride a case accepts
        self.stats = (C.c_uint64 * 4)()
        self.gain = (C.c_uint64 * (4 * 32))()
        self.id = C.c_uint32()

    def _call(self, what, rcode):
        return what, rcode, self.lib.lv_last_error().decode()

    def _views(self, case, struct):
        fields = rc.views_of(case)
        n = rc.n_views_of(case)
        arr = (struct * max(n, len(fields), 1))()
        for i in range(len(arr)):                       # (every entry a valid view: a call that read too far would still read one)
            v = {**rc.VIEW_TOOLS[case["tool"]][0], **(case["views"][i] if i < len(fields) else {})}
            for key in ("points", "image"):
                if key in v:
                    v[key] = self.memory.ctypes.data if v[key] else None
            _set(arr[i], v)
        return (None if "views" in case["null"] else arr), n

    def _params(self, case, make):
        return None if "params" in case["null"] else C.byref(_set(make(), case["over"]))

    def run(self, case):
        capi, lib, h, tool = self.capi, self.lib, self.h, case["tool"]
        if tool == "vis":
            views, n = self._views(case, capi.View)
            return [self._call("lv_map_remove_dynamic", lib.lv_map_remove_dynamic(h, views, n, self._params(case, capi.default_visibility_params), None, None))]
        if tool == "integrate":
            views, n = self._views(case, capi.View)
            return [self._call("lv_occ_integrate", lib.lv_occ_integrate(h, views, n, self.stats))]
        if tool == "gain":
            views, n = self._views(case, capi.View)
            return [self._call("lv_occ_view_gain", lib.lv_occ_view_gain(h, views, n, None if "gain" in case["null"] else self.gain))]
        if tool == "normals":
            return [self._call("lv_map_normals", lib.lv_map_normals(h, self._params(case, capi.default_surface_params), None, None, None, None, 0))]
        if tool == "outliers":
            return [self._call("lv_map_remove_outliers", lib.lv_map_remove_outliers(h, self._params(case, capi.default_outlier_params), None, None, None))]
        if tool == "cluster":
            p = self._params(case, capi.default_cluster_params)
            return [self._call("lv_map_cluster", lib.lv_map_cluster(h, p, None, None, 0, None, 0, None)),
                    self._call("lv_map_remove_clusters", lib.lv_map_remove_clusters(h, p, None, None, None, None))]
        if tool == "paint":
            views, n = self._views(case, capi.LvCameraView)
            return [self._call("lv_map_paint", lib.lv_map_paint(h, views, n, self._params(case, capi.default_paint_params), None, None, None))]
        if tool == "place_params":
            return [self._call("lv_place_configure", lib.lv_place_configure(h, self._params(case, capi.default_place_params)))]
        if tool in ("place_state", "place_query"):
            x = np.array(rc.params_of(case).get("x", rc.STATE), np.float64)
            xp = None if "state" in case["null"] else x.ctypes.data
            assert lib.lv_place_clear(h) == rc.LV_OK
            out = [self._call("lv_place_query", lib.lv_place_query(h, xp, rc.params_of(case).get("k", 1), None, None, None, None))]
            if tool == "place_state":
                out.append(self._call("lv_place_add_scan", lib.lv_place_add_scan(h, xp, C.byref(self.id))))
            return out
        if tool in ("place_centres", "place_add_map"):
            cs = np.array(rc.DEFAULTS["place_centres"]["centres"] if tool == "place_add_map" else rc.params_of(case)["centres"], np.float64)
            n = rc.params_of(case)["n"] if tool == "place_add_map" else len(cs) // 3
            csp = cs.ctypes.data_as(C.POINTER(C.c_double))
            out = [self._call("lv_place_add_map", lib.lv_place_add_map(h, csp, n, C.byref(self.id)))]
            if tool == "place_centres":
                desc = np.zeros(n * 64 * 32, np.float32)   # (room for the largest descriptor a case may have configured)
                out.append(self._call("lv_place_load", lib.lv_place_load(h, desc.ctypes.data_as(C.POINTER(C.c_float)), csp, n)))
            return out
        raise AssertionError(tool)


def _expected(case, what):
    if case["rc"] != rc.LV_OK:
        return case["rc"], case["msg"]
    if what == "lv_place_query":
        return NO_PLACES
    if what == "lv_place_add_scan":
        return NO_SCAN
    return rc.LV_OK, None


def test_every_entry_point_answers_as_the_table_says(capi, ctx):
    calls = Calls(capi, ctx)
    ran = set()
    for case in rc.CASES:
        if case["where"] == "host":
            assert case["rc"] == rc.LV_OK and case["tool"] in ("vis", "integrate", "gain")
            continue
        if case["rc"] == rc.LV_OK:   # what an accepted call may go on to read is really there
            assert all(v.get("n", 0) <= 2 and v.get("stride", 12) <= 16 for v in case["views"]), case["name"]
        for what, code, msg in calls.run(case):
            want_code, want_msg = _expected(case, what)
            assert code == want_code and (want_msg is None or msg == want_msg), (case["name"], what, code, msg)
            ran.add(what)
    assert ran == {"lv_map_remove_dynamic", "lv_occ_integrate", "lv_occ_view_gain", "lv_map_normals", "lv_map_remove_outliers", "lv_map_cluster",
                   "lv_map_remove_clusters", "lv_map_paint", "lv_place_configure", "lv_place_query", "lv_place_add_scan", "lv_place_add_map", "lv_place_load"}
    assert ctx.map_size() == 0   # (and nothing became of the accepted calls)
