"""Aiding observations for the resident filter: the records `Context.observe` takes, and the host-side geometry around them.

Host side only (numpy): nothing here touches the device.  The records are `capi.Observation` (lv_observation of
include/limovelo_hip.h "Aiding observations"); the measurement models and the update rule are stated there.

    from limo_velo_amd import aiding
    yaw, t = aiding.fit_frame(map_xyz, enu_xyz)                        # once: ENU fixes -> the map frame (its heading is arbitrary)
    p = aiding.to_map(yaw, t, aiding.enu_from_lla(lat, lon, alt, origin))
    ctx.observe([aiding.position(p, cov=0.5 ** 2, lever=(0.1, 0, 0.3), gate=aiding.chi2_gate(3, 0.99))])
    ctx.observe([aiding.body_velocity((speed, 0, 0), cov=(0.05 ** 2, 0.02 ** 2, 0.02 ** 2), axes="xyz")])   # wheel + non-holonomic zeros
"""
from __future__ import annotations

import numpy as np

from .capi import OBS_ATTITUDE, OBS_POSITION, OBS_VELOCITY_BODY, OBS_VELOCITY_WORLD, Observation

S2_LEN = 98090.0 / 10000.0   # the length the filter keeps gravity at (lv_manifold.hpp)

# chi-square quantiles by rows (degrees of freedom) and probability
_CHI2 = {
    (1, 0.95): 3.841458820694124, (1, 0.99): 6.634896601021213, (1, 0.999): 10.827566170662733,
    (2, 0.95): 5.991464547107979, (2, 0.99): 9.210340371976182, (2, 0.999): 13.815510557964274,
    (3, 0.95): 7.814727903251179, (3, 0.99): 11.344866730144373, (3, 0.999): 16.26623619623813,
}


def chi2_gate(rows: int, p: float) -> float:
    """The NIS bound below which a consistent `rows`-dimensional innovation falls with probability p (0.95, 0.99 or 0.999)."""
    try:
        return _CHI2[(int(rows), float(p))]
    except KeyError:
        raise ValueError(f"chi2_gate: rows in 1..3 and p in (0.95, 0.99, 0.999), not ({rows}, {p})") from None


def _mask(axes: str) -> int:
    if not axes or len(set(axes)) != len(axes) or any(a not in "xyz" for a in axes):
        raise ValueError(f"axes: a non-empty selection of 'x', 'y', 'z', not {axes!r}")
    return sum(1 << "xyz".index(a) for a in axes)


def _cov(cov, axes: str) -> np.ndarray:
    """A scalar (times I), three variances, one variance per selected axis, or the full 3 x 3 matrix."""
    c = np.asarray(cov, np.float64)
    if c.ndim == 0:
        return np.eye(3) * float(c)
    if c.shape == (3, 3):
        return c.copy()
    if c.shape == (3,):
        return np.diag(c)
    if c.shape == (len(axes),):
        R = np.eye(3)
        for a, v in zip(axes, c):
            R["xyz".index(a)] *= v
        return R
    raise ValueError(f"cov: a scalar, 3 variances, {len(axes)} variances for axes {axes!r} or a 3 x 3 matrix, not shape {c.shape}")


def _record(kind, z, cov, axes, lever=(0.0, 0.0, 0.0), gate=None) -> Observation:
    o = Observation()
    o.kind, o.mask = kind, _mask(axes)
    zz = np.asarray(z, np.float64).ravel()
    for i, v in enumerate(zz):
        o.z[i] = float(v)
    for i, v in enumerate(_cov(cov, axes).ravel()):
        o.R[i] = float(v)
    for i, v in enumerate(np.asarray(lever, np.float64).ravel()[:3]):
        o.lever[i] = float(v)
    o.gate = 0.0 if gate is None else float(gate)
    return o


def _vec3(z, axes):
    """Three components; a shorter z gives the selected axes in the order of `axes` (a barometer: z=h, axes="z")."""
    v = np.atleast_1d(np.asarray(z, np.float64)).ravel()
    if v.size == 3:
        return v
    if v.size != len(axes):
        raise ValueError(f"{v.size} values for axes {axes!r}")
    out = np.zeros(3)
    for a, t in zip(axes, v):
        out["xyz".index(a)] = t
    return out


def position(z, cov, lever=(0, 0, 0), gate=None, axes="xyz") -> Observation:
    """A position fix of the antenna (at `lever` in the IMU frame) in the map frame.  A barometer is axes="z"."""
    return _record(OBS_POSITION, _vec3(z, axes), cov, axes, lever, gate)


def world_velocity(v, cov, gate=None, axes="xyz") -> Observation:
    """The IMU's velocity in the map frame (a GNSS Doppler velocity)."""
    return _record(OBS_VELOCITY_WORLD, _vec3(v, axes), cov, axes, gate=gate)


def zupt(cov, gate=None) -> Observation:
    """A zero-velocity update."""
    return world_velocity((0.0, 0.0, 0.0), cov, gate)


def body_velocity(v, cov, axes="x", gate=None) -> Observation:
    """The IMU's velocity in its own frame.  A wheel speed alone is axes="x"; with the non-holonomic zeros it is axes="xyz",
    v=(s, 0, 0)."""
    return _record(OBS_VELOCITY_BODY, _vec3(v, axes), cov, axes, gate=gate)


def attitude(q, cov, gate=None, axes="xyz") -> Observation:
    """An attitude (AHRS, 9-dof IMU) as a quaternion x, y, z, w, body to map; normalised here.  cov: of the rotation error in the
    body frame (rad^2)."""
    q = np.asarray(q, np.float64).ravel()
    if q.size != 4 or not np.isfinite(q).all() or not np.linalg.norm(q) > 0:
        raise ValueError("attitude: a finite non-zero quaternion x, y, z, w")
    return _record(OBS_ATTITUDE, q / np.linalg.norm(q), cov, axes, gate=gate)


# ---- GPS geometry --------------------------------------------------------------------------------------
_WGS84_A = 6378137.0
_WGS84_F = 1.0 / 298.257223563
_WGS84_E2 = _WGS84_F * (2.0 - _WGS84_F)


def _ecef(lat, lon, alt):
    lat, lon, alt = np.radians(np.asarray(lat, np.float64)), np.radians(np.asarray(lon, np.float64)), np.asarray(alt, np.float64)
    n = _WGS84_A / np.sqrt(1.0 - _WGS84_E2 * np.sin(lat) ** 2)
    return np.stack([(n + alt) * np.cos(lat) * np.cos(lon), (n + alt) * np.cos(lat) * np.sin(lon),
                     (n * (1.0 - _WGS84_E2) + alt) * np.sin(lat)], axis=-1)


def enu_from_lla(lat, lon, alt, origin) -> np.ndarray:
    """East, north, up (metres) of WGS-84 latitude / longitude (degrees) and ellipsoidal height (metres) in the tangent frame at
    origin = (lat0, lon0, alt0).  Closed form: geodetic -> ECEF -> the rotation at the origin.  Scalars or arrays ([..., 3] out)."""
    lat0, lon0, alt0 = (float(t) for t in origin)
    d = _ecef(lat, lon, alt) - _ecef(lat0, lon0, alt0)
    sp, cp, sl, cl = np.sin(np.radians(lat0)), np.cos(np.radians(lat0)), np.sin(np.radians(lon0)), np.cos(np.radians(lon0))
    Rm = np.array([[-sl, cl, 0.0], [-sp * cl, -sp * sl, cp], [cp * cl, cp * sl, sp]])
    return d @ Rm.T


def fit_frame(map_xyz, enu_xyz):
    """The yaw and translation that take ENU fixes into the map frame, from matched trajectory samples ([n, 3] each, n >= 2 and
    not all at one spot): map ~ Rz(yaw) enu + t.  Closed-form 2-D Procrustes on x, y; the height offset is the mean difference
    (both frames have z up).  Returns (yaw, t)."""
    m, e = np.asarray(map_xyz, np.float64).reshape(-1, 3), np.asarray(enu_xyz, np.float64).reshape(-1, 3)
    if m.shape != e.shape or len(m) < 2:
        raise ValueError("fit_frame: two matched [n, 3] arrays with n >= 2")
    mc, ec = m.mean(0), e.mean(0)
    dm, de = m - mc, e - ec
    s = float(np.sum(de[:, 0] * dm[:, 1] - de[:, 1] * dm[:, 0]))
    c = float(np.sum(de[:, 0] * dm[:, 0] + de[:, 1] * dm[:, 1]))
    if s == 0.0 and c == 0.0:
        raise ValueError("fit_frame: the samples do not move in the plane")
    yaw = float(np.arctan2(s, c))
    t = mc - to_map(yaw, np.zeros(3), ec)
    return yaw, t


def to_map(yaw, t, enu_xyz) -> np.ndarray:
    """Rz(yaw) enu + t: fixes in the map frame, with fit_frame's result."""
    c, s = np.cos(yaw), np.sin(yaw)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return np.asarray(enu_xyz, np.float64) @ Rz.T + np.asarray(t, np.float64)


# ---- initialisation from a stationary window -----------------------------------------------------------
def static_init(acc, gyro) -> np.ndarray:
    """An initial state (the 26 doubles of lv_state, for lv_filter_set) from a stationary window of IMU samples ([n, 3] each,
    specific force in m/s^2 and rate in rad/s, in the IMU frame).

    At rest the model's R (acc - ba) + grav is zero.  Gravity is taken as (0, 0, -9.809) in a level map frame, so R is the
    rotation that takes the mean specific force's direction to +z — the one of smallest angle: roll and pitch, no heading
    (heading is unobservable at rest).  bg is the mean rate.  ba stays zero: one window cannot tell a bias along gravity from a
    gravity of another length.  Everything else is zero / identity."""
    a, w = np.asarray(acc, np.float64).reshape(-1, 3), np.asarray(gyro, np.float64).reshape(-1, 3)
    if len(a) == 0 or len(w) == 0:
        raise ValueError("static_init: empty window")
    am = a.mean(0)
    n = np.linalg.norm(am)
    if not n > 0:
        raise ValueError("static_init: the mean specific force is zero")
    u = am / n
    # the shortest rotation u -> z: axis u x z, quaternion (axis sin, 1 + u.z) normalised; u = -z: half a turn about x
    q = np.array([u[1], -u[0], 0.0, 1.0 + u[2]])
    q = np.array([1.0, 0.0, 0.0, 0.0]) if np.linalg.norm(q) < 1e-12 else q / np.linalg.norm(q)
    x = np.zeros(26)
    x[3:7] = q
    x[10] = 1.0
    x[17:20] = w.mean(0)
    x[23:26] = (0.0, 0.0, -S2_LEN)
    return x
