"""Timing of lv_surf_merge on the default 512 x 512 x 64 volume (0.2 m).  The ten 64 x 2048 sweeps of scripts/tsdf_timing.py are fused
into the volume, a submap of 256 x 256 x 64 voxels is cut from its middle, the volume is cleared and the submap merged back:
  `cases`   at the identity; at a yaw of 30 degrees about the submap's centre plus an off-lattice translation; and with the same
            arrays declared at twice the resolution (0.4 m: a ratio of 2, the submap then covers the whole volume).  Each from a
            cleared volume: `call_ms` the host wall time of the whole call (median of `n` after a warm-up), `stats`, `box_voxels`
            the destination voxels the kernel is launched over (surf_merge_box restated here) and `box_bytes` = 8 per voxel of it.
  `kernel_ms`  with --kernel-trace CSV (the kernel_trace.csv of a `rocprofv3 --kernel-trace --stats` run of this script with
            --profiled): per case the median over its calls of surf_merge_kernel's time; `staging_upload_ms` is the rest of the
            call: the submap interleaved into pinned memory, its copy to the device, the stats' way back.
  `copy`    the floor: a plain device-to-device copy of each case's box_bytes (torch), `copy_ms`.
  `host`    the route without this call, on a volume small enough for numpy (128 x 128 x 64, a 64 x 64 x 32 submap, the yaw case):
            lv_tsdf_fetch (`fetch_ms`), the rule in numpy (tests/surf_merge_ref.py, `rule_ms`), lv_tsdf_load (`load_ms`); the
            volume it leaves must equal the call's bit for bit.
Prints one JSON line; --out writes it too.

    python scripts/surf_merge_timing.py --out plain.json
    rocprofv3 --kernel-trace --stats --output-format csv -d prof -o surf_merge -- python scripts/surf_merge_timing.py --profiled
    python scripts/surf_merge_timing.py --merge plain.json --kernel-trace prof/.../surf_merge_kernel_trace.csv --out profiles/surf_merge_timing.json"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

CASES = ("identity", "yaw30", "ratio2")
PROFILED_CALLS = 6   # per case in a --profiled run: the warm-up and five more
REPS = 20


def spread(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), n=len(ts))


def kernels_ms(path):
    """Per case, in CASES' order: surf_merge_kernel's time, the median over the calls behind the warm-up."""
    with open(path) as f:
        rows = sorted((r for r in csv.DictReader(f) if "surf_merge_kernel" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == PROFILED_CALLS * len(CASES), len(rows)
    ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows]
    return [spread(ms[k * PROFILED_CALLS + 1:(k + 1) * PROFILED_CALLS]) for k in range(len(CASES))]


def yaw_about(centre, angle, offset):
    """(t, q): a turn by `angle` about the vertical through `centre`, then `offset`."""
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    centre = np.asarray(centre, np.float64)
    return centre + offset - R @ centre, np.array([0.0, 0.0, np.sin(angle / 2), np.cos(angle / 2)])


def box_voxels(mr, p, sub, pose):
    """surf_merge_box in numpy: the destination voxels the submap's box of metres can reach."""
    R = mr.rot(pose[1])
    n = np.array(sub["S"].shape[::-1], np.float64)
    so, sr = np.asarray(sub["origin"], np.float32).astype(np.float64), float(np.float32(sub["resolution"]))
    corners = np.array([[so[b] + ((k >> b) & 1) * n[b] * sr for b in range(3)] for k in range(8)]) @ R.T + np.asarray(pose[0], np.float64)
    out = 1
    for a, dim in enumerate((p.nx, p.ny, p.nz)):
        lo, hi, o, res = corners[:, a].min(), corners[:, a].max(), float(p.origin[a]), float(p.resolution)
        slack = res + 1e-3 * (hi - lo) + 1e-3 * max(abs(lo - o), abs(hi - o))
        a0 = max(0, int(np.floor((lo - slack - o) / res - 0.5)))
        a1 = min(dim, int(np.ceil((hi + slack - o) / res - 0.5)) + 1)
        out *= max(0, a1 - a0)
    return out


def cut(vol, p, lo, shape):
    """A submap of `shape` (nz, ny, nx) voxels cut from the fetched volume at voxel `lo` (x, y, z)."""
    x, y, z = lo
    nz, ny, nx = shape
    origin = np.array([np.float32(p.origin[a]) + np.float32(lo[a]) * np.float32(p.resolution) for a in range(3)], np.float32)
    return dict(origin=origin, resolution=np.float32(p.resolution), trunc_cells=int(p.trunc_cells),
                S=np.ascontiguousarray(vol["S"][z:z + nz, y:y + ny, x:x + nx]), W=np.ascontiguousarray(vol["W"][z:z + nz, y:y + ny, x:x + nx]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--profiled", action="store_true", help="six calls of every case, nothing written: the run to put under rocprofv3")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--merge", default=None, help="the JSON of an earlier run of this script: nothing runs, --kernel-trace is added to it")
    a = ap.parse_args()
    if a.merge:
        with open(a.merge) as f:
            finish(json.load(f), a)
        return
    torch = None
    if not a.profiled:
        try:
            import torch   # (before the library: its runtime has to come first)

            torch.cuda.init()
        except Exception:
            torch = None
    import occupancy_timing

    sweeps, _ = occupancy_timing.make_sweeps(None, count_visits=False)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, mesh
    import surf_merge_ref as mr

    res = dict(what="lv_surf_merge", volume="512x512x64 @ 0.2 m (defaults), trunc_cells 3, cleared before every call",
               submap="256x256x64 cut from the middle of the volume after ten 64x2048 sweeps", cases=[], host=[])
    with capi.Context() as ctx:
        ctx.tsdf_configure()
        ctx.tsdf_integrate(sweeps)
        p = ctx.tsdf_params()
        vol = ctx.tsdf_fetch()
        sub = cut(vol, p, (128, 128, 0), (64, 256, 256))
        centre = [float(sub["origin"][a]) + 0.5 * n * float(p.resolution) for a, n in enumerate((256, 256, 64))]
        coarse = dict(sub, resolution=np.float32(0.4), origin=np.array([centre[a] - 0.5 * n * 0.4 for a, n in enumerate((256, 256, 64))], np.float32))
        calls = dict(identity=(sub, mr.IDENTITY), yaw30=(sub, yaw_about(centre, np.pi / 6, np.array([0.137, -0.211, 0.093]))), ratio2=(coarse, mr.IDENTITY))
        for name in CASES:
            s, pose = calls[name]
            ctx.tsdf_clear()
            stats = mesh.merge(ctx, s, pose)   # warm-up: the staging buffers, the code object
            if a.profiled:
                for _ in range(PROFILED_CALLS - 1):
                    ctx.tsdf_clear()
                    mesh.merge(ctx, s, pose)
                continue
            m, keep = capi.surf_submap(s["origin"], s["resolution"], s["trunc_cells"], s["S"], s["W"])
            g = mesh.pose7(pose)
            ts = []
            for _ in range(REPS):
                ctx.tsdf_clear()
                t0 = time.perf_counter()
                ctx.surf_merge(m, g, None)
                ts.append((time.perf_counter() - t0) * 1e3)
            box = box_voxels(mr, p, s, pose)
            res["cases"].append(dict(name=name, call_ms=spread(ts), stats=[int(x) for x in stats], box_voxels=box, box_bytes=8 * box,
                                     submap_bytes=8 * int(s["S"].size)))
        if a.profiled:
            return
        if not a.no_host:
            small = capi.default_tsdf_params(origin=[float(sub["origin"][0]), float(sub["origin"][1]), float(p.origin[2])], resolution=float(p.resolution),
                                             nx=128, ny=128, nz=64)
            ctx.tsdf_configure(small)
            q = ctx.tsdf_params()
            s = cut(vol, p, (160, 160, 16), (32, 64, 64))
            c = [float(s["origin"][a]) + 0.5 * n * float(p.resolution) for a, n in enumerate((64, 64, 32))]
            pose = yaw_about(c, np.pi / 6, np.array([0.137, -0.211, 0.093]))
            t0 = time.perf_counter()
            st = mesh.merge(ctx, s, pose)
            t1 = time.perf_counter()
            got = ctx.tsdf_fetch()
            ctx.tsdf_clear()
            t2 = time.perf_counter()
            v = ctx.tsdf_fetch()
            t3 = time.perf_counter()
            dest = dict(origin=np.array([float(x) for x in q.origin], np.float32), resolution=np.float32(q.resolution), trunc_cells=q.trunc_cells,
                        max_weight=q.max_weight, S=v["S"], W=v["W"])
            want = mr.merge(dest, s, pose)
            t4 = time.perf_counter()
            ctx.tsdf_load(want["S"], want["W"])
            t5 = time.perf_counter()
            equal = bool(np.array_equal(got["S"], want["S"]) and np.array_equal(got["W"], want["W"]) and np.array_equal(st, want["stats"]))
            assert equal and st[1] > 0
            res["host"].append(dict(name="yaw30", volume="128x128x64", submap="64x64x32", call_ms=(t1 - t0) * 1e3, fetch_ms=(t3 - t2) * 1e3,
                                    rule_ms=(t4 - t3) * 1e3, load_ms=(t5 - t4) * 1e3, equal_volume=equal, stats=[int(x) for x in st]))
    if torch is not None and torch.cuda.is_available():
        res["copy"] = []
        for row in res["cases"]:
            n = row["box_bytes"] // 4
            src, dst = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
            dst.copy_(src)
            torch.cuda.synchronize()
            ts = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                dst.copy_(src)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            res["copy"].append(dict(name=row["name"], bytes=4 * n, copy_ms=spread(ts)))
    finish(res, a)


def finish(res, a):
    if a.kernel_trace:
        for row, k in zip(res["cases"], kernels_ms(a.kernel_trace)):
            row["kernel_ms"] = k
            row["staging_upload_ms"] = row["call_ms"]["median"] - k["median"]
            row["box_gbps"] = row["box_bytes"] / (k["median"] * 1e-3) / 1e9
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
