"""Generates tests/golden/store_growth.npz — the map statistics and the SHA-256 digests of map_fetch, scan_fetch and cloud_fetch
after ONE context has crossed every floor at which the map, scan and cloud stores grow (MapStore, ScanStore, CloudStore:
limo-velo_amd/csrc/lv_stores.hpp), at the smallest sizes that cross them: 4096 ids twice (4096, 8192) with the box chains and the
back-positions in place, 4096 batch points, 4096 scan points, 4096 raw points of a de-skew with 2 and with 70 motion states, 65536
points and 1 MiB of a LiDAR message, and the LiDAR buffer's move to the front and its reallocation across 2^18 points.
tests/test_gpu_store_growth.py walks the same steps, checks the map after each against a model, and holds the end to this record.
The file pins the library as built from the commit BEFORE the stores' memory moved into DevBuf / PinBuf.

Uses limo_velo_amd.capi only, so the same script records any build.  Needs an MI355X:

    python tests/golden/make_golden_growth.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

STAT_LISTS = ("pool_used", "pool_cap", "slots_used", "slots_cap")
MSG_POINTS = 70_000        # > 65536 points; 48-byte records: > 1 MiB
BUFFER_FLOOR = 1 << 18


def _slab(rng, n, lo=(-10.0, -10.0, 0.0), hi=(10.0, 10.0, 3.0)):
    return rng.uniform(lo, hi, (n, 3)).astype(np.float32)


def _states(capi, n, t0, t1):
    """n motion states at even times over [t0, t1]: a slow turn at constant speed (any path serves: the record is compared with
    the parent's bytes, not with a model)."""
    out = []
    for k in range(n):
        t = t0 + (t1 - t0) * k / (n - 1)
        a = 0.3 * (t - t0)
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
        out.append(capi.motion_state(time=t, R=R, pos=(2.0 * (t - t0), 0.5 * (t - t0), 0.0), vel=(2.0, 0.5, 0.0), w=(0.0, 0.0, 0.3)))
    return np.concatenate(out)


def steps(ctx, capi, marks):
    """Runs the scenario on ctx.  Yields (name, event) after every step; event is what the step did to the MAP — ("build", pts),
    ("add", pts, downsample), ("evict", lo, hi), or None for the scan and cloud steps — so a caller can keep a model beside it.
    marks[name] receives what a scan or cloud step left to fetch (later steps overwrite the scan and clear the buffer)."""
    import cloud_messages as cm

    rng = np.random.default_rng(58)
    base = _slab(rng, 3000)
    ctx.map_build(base)
    yield "build 3000", ("build", base)

    def revisit(n):   # a down-sampling batch: near-copies of old points (the chains decide who stays) and fresh ones
        old = ctx.map_fetch()
        near = old[rng.integers(0, len(old), n // 2)] + np.float32(0.01)
        return np.concatenate([near, _slab(rng, n - n // 2)]).astype(np.float32)

    b = revisit(200)
    ctx.map_add(b, downsample=True)
    yield "first down-sampling add", ("add", b, True)
    for floor in (4096, 8192):
        while ctx.map_stats()["ids"] <= floor:
            b = _slab(rng, 600)
            ctx.map_add(b, downsample=False)
            yield f"plain add towards {floor}", ("add", b, False)
        assert ctx.map_stats()["capacity"] == 2 * floor
        b = revisit(200)
        ctx.map_add(b, downsample=True)
        yield f"down-sampling add past {floor}", ("add", b, True)
        lo, hi = np.array([-4.0, -4.0, -1.0], np.float32) + np.float32(floor / 4096.0), np.array([-1.0, -1.0, 4.0], np.float32) + np.float32(floor / 4096.0)
        ctx.map_evict_box(lo, hi, keep_inside=False)
        yield f"evict a box of old ids past {floor}", ("evict", lo, hi)
    b = revisit(4100)
    ctx.map_add(b, downsample=True)
    yield "batch of 4100", ("add", b, True)

    for n in (4000, 4100):
        ctx.scan_set(_slab(rng, n, (-30, -30, -2), (30, 30, 6)))
        marks[f"scan_set {n}"] = ctx.scan_fetch()
        yield f"scan_set {n}", None
    for n_states in (2, 70):
        for n in (4000, 4100):
            xyz = _slab(rng, n, (-30, -30, -2), (30, 30, 6))
            times = np.sort(rng.uniform(10.001, 10.099, n))
            st = _states(capi, n_states, 10.0, 10.1)
            ctx.scan_deskew(xyz, times, st, st[-1:].copy(), downsample_prec=0.5)
            marks[f"scan_deskew {n} points, {n_states} states"] = ctx.scan_fetch()
            yield f"scan_deskew {n} points, {n_states} states", None

    def message(k, n):
        raw, f, stamp = cm.make_message("hesai", n, seed=100 + k, stamp_sec=1_700_000_000.0 + 0.1 * k + 0.05, sweep=0.09)
        fmt = capi.CloudFormat(f["point_step"], f["off_x"], f["off_y"], f["off_z"], f["off_time"], f["time_type"], f["off_intensity"],
                               f["intensity_type"], f["off_range"], f["range_type"], f["relative_time"])
        return ctx.cloud_ingest(raw, n, fmt, capi.IngestParams(stamp, 0, 0, 0.1, 1, 0.5))

    message(0, 1000)       # the message buffers and the LiDAR buffer at their floors
    yield "cloud message of 1000", None
    k = 1
    message(k, MSG_POINTS)
    yield "cloud message of 70000", None
    while ctx.cloud_size() <= BUFFER_FLOOR:   # ... until the buffer reallocates across 2^18 points (nothing cleared: head == 0)
        k += 1
        message(k, MSG_POINTS)
    marks["cloud buffer reallocated past 2^18"] = ctx.cloud_fetch(-1e300, 1e300)
    yield "cloud buffer reallocated past 2^18", None
    while ctx.cloud_size() + MSG_POINTS <= 2 * BUFFER_FLOOR:
        k += 1
        message(k, MSG_POINTS)
    # all but the last message cleared: the next one does not fit behind the living range, which moves to the front
    ctx.cloud_clear(1_700_000_000.0 + 0.1 * k + 0.045)   # (message k - 1 ends before, message k begins after)
    assert 0 < ctx.cloud_size() <= MSG_POINTS
    message(k + 1, MSG_POINTS)
    yield "cloud buffer moved to the front", None


def record(ctx, marks):
    """What the end of the scenario is held to: the statistics as one uint64 row, and the digests (with the lengths) of the three
    fetches at the end and of the marks taken on the way."""
    st = ctx.map_stats()
    names, vals = [], []
    for key, v in st.items():
        for i, x in enumerate(v if key in STAT_LISTS else [v]):
            names.append(f"{key}[{i}]" if key in STAT_LISTS else key)
            vals.append(x)
    fetched = dict(marks, map_fetch=ctx.map_fetch(), scan_fetch=ctx.scan_fetch(), cloud_fetch=ctx.cloud_fetch(-1e300, 1e300))
    digests = {k: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for k, a in fetched.items()}
    sizes = {k: len(a) for k, a in fetched.items()}
    return names, np.asarray(vals, np.uint64), digests, sizes


def main():
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi

    marks = {}
    with capi.Context() as ctx:
        for name, _ in steps(ctx, capi, marks):
            print(name, flush=True)
        names, vals, digests, sizes = record(ctx, marks)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "store_growth.npz")
    keys = sorted(digests)
    np.savez_compressed(out, stat_names=np.array(names), stats=vals, digest_names=np.array(keys),
                        digests=np.array([digests[k] for k in keys]), sizes=np.array([sizes[k] for k in keys], np.uint64))
    print("wrote", out, os.path.getsize(out), "bytes;", dict(zip(names, vals.tolist())), sizes, digests)


if __name__ == "__main__":
    main()
