"""The cases tests/test_tsdf_ref.py, tests/test_tsdf_host.py and tests/test_gpu_tsdf.py share: small grids, sweeps that reach every
branch of the rule, and the sphere pattern.  A case is dict(name, prm, calls, min_weight): calls is a list of lv_tsdf_integrate
calls, each a list of views (R, t, points).  The reference of a case is computed once (reference()) and shared."""
import functools

import numpy as np

import tsdf_ref as tr

F = np.float32
ID = np.eye(3, dtype=F)


def rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], F)


def grid_params(nx, ny, nz, **kw):
    """0.25 m voxels; min_range 0.3 m is 1.2 voxels, below T = 3 voxels: hits closer than T to the sensor exist; max_range 6 m is
    24 voxels, so rays leave the grid and long returns are CUT."""
    return tr.params(origin=(-1.0, -0.5, -0.25), resolution=0.25, nx=nx, ny=ny, nz=nz, min_range=0.3, max_range=6.0, **kw)


def random_view(rng, t, n=1000):
    """n returns round t: ranges 0.1..8 m (some below min_range, some CUT), a few non-finite."""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = (d * rng.uniform(0.1, 8.0, (n, 1))).astype(F)
    pts[3] = (np.nan, 0, 0)
    pts[77] = (0, -np.inf, 1)
    pts[500] = (np.inf, np.inf, np.inf)
    pts[10:40] *= F(0.5 / 8.0)          # a band of short hits, closer than T
    return rot(rng), np.asarray(t, F), pts


def wall_view(t, n=1000):
    """A scan of the plane x = 2.1 m from t: a surface the mesh can close cells on."""
    t = np.asarray(t, F)
    m = int(np.ceil(np.sqrt(n)))
    yy, zz = np.meshgrid(np.linspace(-0.4, 3.6, m), np.linspace(-0.2, 1.9, m))
    pts = np.stack([np.full(m * m, 2.1), yy.reshape(-1), zz.reshape(-1)], axis=1)[:n]
    return ID, t, (pts - t).astype(F)


def identical_view(t, n=4096):
    """n identical returns: one voxel takes every atomic of its ray."""
    return ID, np.asarray(t, F), np.tile(np.array([[1.3, 0.4, 0.2]], F), (n, 1))


def sphere_view(centre_vox, radius_vox, rings, azimuths, origin, resolution):
    """The sphere pattern: `rings` elevation rings at el = -pi/2 + (i + 0.5) pi / rings, each with max(4, round(azimuths cos el))
    azimuths at 2 pi (j + 0.37) / m; returns at radius_vox voxels round a sensor at voxel position centre_vox."""
    dirs = []
    for i in range(rings):
        el = -np.pi / 2 + (i + 0.5) * np.pi / rings
        m = max(4, int(round(azimuths * np.cos(el))))
        az = 2 * np.pi * (np.arange(m) + 0.37) / m
        dirs.append(np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.full(m, np.sin(el))], axis=1))
    d = np.concatenate(dirs)
    t = (np.asarray(origin, np.float64) + np.asarray(centre_vox, np.float64) * resolution).astype(F)
    return ID, t, (d * radius_vox * resolution).astype(F)


def sphere_case(n, centre_vox, radius_vox, rings, azimuths, name):
    origin, res = (-1.5, 2.0, 0.5), 0.5
    prm = tr.params(origin=origin, resolution=res, nx=n, ny=n, nz=n, min_range=res, max_range=res * 2 * n, trunc_cells=3)
    return dict(name=name, prm=prm, calls=[[sphere_view(centre_vox, radius_vox, rings, azimuths, origin, res)]], min_weight=1,
                centre=np.asarray(centre_vox, np.float64), radius=float(radius_vox))


SPHERE_SMALL = dict(n=20, centre_vox=(10.3, 9.9, 10.6), radius_vox=6.0, rings=75, azimuths=150, name="sphere-6")
SPHERE_LARGE = dict(n=64, centre_vox=(32.3, 31.9, 32.6), radius_vox=20.0, rings=210, azimuths=420, name="sphere-20")

INSIDE = (0.8, 1.1, 0.9)      # inside both grids
OUTSIDE = (-2.6, 0.3, 0.4)    # outside on -x: rays enter, miss, or leave at once
ABOVE = (1.0, 1.0, 7.0)       # far above: most rays never reach the grid


def cases():
    out = []
    for nx, ny, nz in ((33, 17, 9), (70, 37, 20)):
        for carve in (0, 1):
            rng = np.random.default_rng(1000 * nx + carve)
            prm = grid_params(nx, ny, nz, carve=carve)
            tag = "%dx%dx%d-carve%d" % (nx, ny, nz, carve)
            out.append(dict(name=tag + "-1view", prm=prm, calls=[[random_view(rng, INSIDE)]], min_weight=1))
            out.append(dict(name=tag + "-3views", prm=prm,
                            calls=[[random_view(rng, INSIDE), random_view(rng, OUTSIDE), wall_view(INSIDE)],
                                   [random_view(rng, ABOVE), (ID, np.array([np.nan, 0, 0], F), np.ones((5, 3), F)),
                                    (ID, np.asarray(INSIDE, F), np.zeros((0, 3), F))]], min_weight=1))
            out.append(dict(name=tag + "-identical", prm=prm, calls=[[identical_view(INSIDE)]], min_weight=1))
        # max_weight = 4 over three calls: the rescale branch, then a mesh of what it left, known from weight 2 on
        prm = grid_params(nx, ny, nz, carve=0, max_weight=4)
        out.append(dict(name="%dx%dx%d-maxweight4" % (nx, ny, nz), prm=prm,
                        calls=[[wall_view(INSIDE), wall_view((0.5, 0.7, 0.6))], [wall_view(INSIDE), identical_view(INSIDE, 64)],
                               [wall_view((0.2, 1.9, 1.0)), wall_view(INSIDE)]], min_weight=2))
    out.append(sphere_case(**SPHERE_SMALL))
    return out


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = {c["name"]: c for c in cases() + [sphere_case(**SPHERE_LARGE)]}[name]
    prm = case["prm"]
    S, W = tr.empty(prm)
    stats = []
    for views in case["calls"]:
        S, W, st = tr.integrate(prm, S, W, views)
        stats.append(st)
    mesh = tr.mesh(prm, S, W, case["min_weight"])
    for a in (S, W, *stats, *mesh.values()):
        a.setflags(write=False)
    return dict(S=S, W=W, stats=stats, mesh=mesh)


def reference(case):
    """dict(S, W, stats = [per call], mesh) of the case: computed once, shared, read-only."""
    return _reference(case["name"])
