"""The scene tests/test_depth_ref.py and tests/test_gpu_depth.py share: a volume of 48 x 40 x 24 voxels, a camera inside it that looks
along +x at a slanted plane with a sphere in front of it, and a block of pixels without a measurement.  One view of it reaches
every branch of the rule (tests/test_depth_ref.py holds that): voxels not projected, on an invalid pixel, beyond +T, behind -T and
inside the band on both sides of the surface.  The images are made in f64 and rounded once; the rule itself is depth_ref's."""
import numpy as np

import depth_ref as dr

F = np.float32

NX, NY, NZ = 48, 40, 24
RES = 0.1
ORIGIN = (-2.4, -2.0, -1.2)
TRUNC_CELLS = 3
WIDTH, HEIGHT, FOCAL, CX, CY = 64, 48, 40.0, 31.5, 23.5
POSE = (0.15, -0.1, (-1.9, 0.13, 0.07))                      # yaw, pitch, position
POSES = (POSE, (-0.35, 0.05, (-1.7, 1.1, 0.3)), (0.5, 0.2, (-2.0, -1.2, 0.6)))
PLANE_N, PLANE_C = (1.0, 0.2, 0.1), 1.0                      # n . x = c with n normalised
SPHERE_C, SPHERE_R = (-0.3, 0.4, 0.0), 0.45
HOLE = (slice(5, 12), slice(40, 52))                         # rows 5..11, columns 40..51: raw 0
AXES = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float64)   # camera x, y, z as world -y, -z, +x: looking along +x


def params(**kw):
    p = dict(min_depth=0.3, max_depth=5.0, max_norm_radius=1.5, carve=0)
    p.update(kw)
    return dr.Params(**p)


def rot(yaw, pitch):
    """Camera -> world [3, 3] f64: looking along +x, turned by yaw about z and by pitch about y (pitch > 0 looks down)."""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    return Rz @ Ry @ AXES


def scene_depth(R, t, width=WIDTH, height=HEIGHT, focal=FOCAL, cx=CX, cy=CY):
    """f64 [height, width]: the z-depth of the plane and the sphere along every pixel's ray; inf where it meets neither in front."""
    t = np.asarray(t, np.float64)
    vv, uu = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    d = np.stack([(uu - cx) / focal, (vv - cy) / focal, np.ones_like(uu, float)], -1) @ np.asarray(R, np.float64).T   # the rays at z = 1
    n = np.asarray(PLANE_N) / np.linalg.norm(PLANE_N)
    with np.errstate(all="ignore"):
        zp = (PLANE_C - n @ t) / (d @ n)
        oc = t - np.asarray(SPHERE_C)
        a, b, c = (d * d).sum(-1), 2 * (d @ oc), oc @ oc - SPHERE_R ** 2
        disc = b * b - 4 * a * c
        zs = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
    zp = np.where(zp > 0, zp, np.inf)
    return np.minimum(zp, np.where(zs > 0, zs, np.inf))


def frame(pose=POSE, hole=True, **kw):
    """A U16 frame in millimetres of the scene from pose (yaw, pitch, position)."""
    yaw, pitch, t = pose
    R = rot(yaw, pitch)
    zd = scene_depth(R, t)
    img = np.clip(np.rint(np.where(np.isfinite(zd), zd, 0) * 1000), 0, 65535).astype(np.uint16)
    if hole:
        img[HOLE] = 0
    f = dict(R=R.astype(F), t=np.asarray(t, F), fx=FOCAL, fy=FOCAL, cx=CX, cy=CY, depth=img, depth_scale=0.001)
    f.update(kw)
    return f


def frames3():
    return [frame(p) for p in POSES]


def frame_f32(pose=POSE):
    """The scene as 32FC1 metres with every kind of pixel that is no measurement: NaN, +inf, -inf, 0 and negatives."""
    f = frame(pose, hole=False)
    yaw, pitch, t = pose
    m = scene_depth(rot(yaw, pitch), t).astype(F)
    m[HOLE] = np.nan
    m[20:24, 10:16] = np.inf
    m[30:33, 50:60] = -np.inf
    m[40:44, 5:25] = 0.0
    m[12:18, 20:30] = -m[12:18, 20:30]
    f["depth"] = m
    del f["depth_scale"]
    return f


def frame_padded(pose=POSE):
    """The U16 frame inside a wider buffer: row_stride = 2 * (width + 7) bytes, the padding full of plausible depths."""
    f = frame(pose)
    wide = np.full((HEIGHT, WIDTH + 7), 1234, np.uint16)
    wide[:, :WIDTH] = f["depth"]
    f["depth"] = wide[:, :WIDTH]
    assert f["depth"].strides == (2 * (WIDTH + 7), 2)
    return f


def frame_distorted(pose=POSE):
    return frame(pose, dist=np.array([0.12, -0.05, 0.004, -0.003, 0.01], F))


def frames32():
    """32 views round the first pose."""
    rng = np.random.default_rng(32)
    yaw, pitch, t = POSE
    return [frame((yaw + rng.uniform(-0.4, 0.4), pitch + rng.uniform(-0.2, 0.2), tuple(np.asarray(t) + rng.uniform(-0.3, 0.3, 3)))) for _ in range(32)]


def frame_flat(t, depth_mm, yaw=0.0, pitch=0.0, width=WIDTH, height=HEIGHT, focal=FOCAL, cx=CX, cy=CY):
    """A frame whose every pixel measures depth_mm."""
    return dict(R=rot(yaw, pitch).astype(F), t=np.asarray(t, F), fx=focal, fy=focal, cx=cx, cy=cy,
                depth=np.full((height, width), depth_mm, np.uint16), depth_scale=0.001)


def frame_pixel(origin=ORIGIN, resolution=RES):
    """A 1 x 1 image: only a point exactly on the optical axis projects into it.  The camera sits on the centre line of the voxels
    (j, k) = (20, 12), axis-aligned, so that row of voxels does."""
    t = (-2.0, float(dr.centre(origin[1], resolution, 20)), float(dr.centre(origin[2], resolution, 12)))
    return frame_flat(t, 1500, width=1, height=1, cx=0.0, cy=0.0)


def frame_corner():
    """A camera outside the volume that looks at its corner (+x, +y, +z) from 0.6 m away; with max_depth 1.2 it judges that corner
    alone, so the launch covers a small box of the volume."""
    return frame_flat((2.9, 2.4, 1.3), 800, yaw=np.arctan2(-0.8, -1.0), pitch=0.25)


def frame_nothing():
    """A camera far outside that looks away."""
    return frame_flat((10.0, 10.0, 10.0), 1000)
