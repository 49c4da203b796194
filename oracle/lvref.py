"""ctypes binding of oracle/_ref/liblvref.so — the REFERENCE's own in-tree sources (/root/reference/src) compiled in place against
stand-in headers (oracle/ref_build/).  TEST INFRASTRUCTURE ONLY: used by tests/test_oracle_ref.py to pin the oracle
(oracle/lv_oracle.cpp) to what the reference's code computes, function by function.  The reference mount exists only in the
build container; elsewhere a prebuilt library (it is not in git) is used as is.  Without either, every call is answered from
tests/golden/ref_calls.npz: what the library returned for the same call (same function, configuration, map contents and
arguments, bit for bit) when the tests last ran against it.  The answers of the functions in DIGESTED, which the tests only
compare bit for bit, are recorded as their SHA-256 digests and replayed as Pinned objects (same_bits compares either form).
With the library present its outputs are checked against that record; LV_REF_RECORD=1 in the environment records them
instead, merged into that file at exit (LV_REF_RECORD=<path>: into the file <path>)."""
from __future__ import annotations

import atexit
import ctypes as C
import functools
import hashlib
import io
import json
import lzma
import os
import subprocess

import numpy as np

import lvoracle as lo

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "_ref", "liblvref.so")
REFERENCE = os.environ.get("LV_REFERENCE_DIR", "/root/reference")


def build() -> str | None:
    """make -C oracle/ref_build when the reference mount is there; the path of the library, or None when it cannot exist."""
    if os.path.isdir(os.path.join(REFERENCE, "src")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "ref_build"), f"REF={REFERENCE}"])
    return _LIB_PATH if os.path.exists(_LIB_PATH) else None


class Config(C.Structure):
    _fields_ = [("estimate_extrinsics", C.c_int), ("max_num_iters", C.c_int), ("num_match_points", C.c_int), ("max_points2match", C.c_int),
                ("max_dist_plane", C.c_double), ("planes_threshold", C.c_float), ("lidar_noise", C.c_double), ("degeneracy_threshold", C.c_double),
                ("limits", C.c_double * 23), ("initial_gravity", C.c_float * 3), ("I_Rotation_L", C.c_float * 9), ("I_Translation_L", C.c_float * 3),
                ("cov_acc", C.c_double), ("cov_gyro", C.c_double), ("cov_bias_acc", C.c_double), ("cov_bias_gyro", C.c_double),
                ("full_rotation_time", C.c_double), ("imu_rate", C.c_double), ("real_time_delay", C.c_double), ("min_dist", C.c_double),
                ("offset_beginning", C.c_int), ("stamp_beginning", C.c_int), ("downsample_rate", C.c_int), ("lidar_type", C.c_int),
                ("downsample_prec", C.c_float)]


LIDAR = {"velodyne": 0, "hesai": 1, "ouster": 2, "custom": 3}
_lib = None


def lib():
    global _lib
    if _lib is None:
        path = build()
        if path is None:
            raise RuntimeError("oracle/_ref/liblvref.so is not built and the reference mount is absent")
        _lib = C.CDLL(path)
        for f in ("lvr_map_size", "lvr_match", "lvr_deskew", "lvr_path", "lvr_cloud_ingest", "lvr_buffer_window"):
            getattr(_lib, f).restype = C.c_size_t
        _lib.lvr_plane.restype = C.c_int
        _lib.lvr_update.restype = C.c_int
    return _lib


def default_config(**kw) -> Config:
    """config/params.yaml defaults of the keys the compiled sources read (params.yaml:17-53)."""
    c = Config()
    c.estimate_extrinsics, c.max_num_iters, c.num_match_points, c.max_points2match = 0, 3, 5, 10
    c.max_dist_plane, c.planes_threshold, c.lidar_noise, c.degeneracy_threshold = 2.0, 0.05, 1e-3, 5.0
    for i in range(23):
        c.limits[i] = 1e-3
    c.initial_gravity[:] = [0.0, 0.0, -9.807]
    c.I_Rotation_L[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    c.I_Translation_L[:] = [0, 0, 0]
    c.cov_acc, c.cov_gyro, c.cov_bias_acc, c.cov_bias_gyro = 1e-2, 1e-4, 1e-4, 1e-5
    c.full_rotation_time, c.imu_rate, c.real_time_delay, c.min_dist = 0.1, 400.0, 1.0, 3.0
    c.offset_beginning, c.stamp_beginning, c.downsample_rate, c.lidar_type, c.downsample_prec = 0, 0, 1, 0, 0.2
    for k, v in kw.items():
        if k in ("limits", "initial_gravity", "I_Rotation_L", "I_Translation_L"):
            getattr(c, k)[:] = list(v)
        elif k == "lidar_type" and isinstance(v, str):
            c.lidar_type = LIDAR[v]
        else:
            setattr(c, k, v)
    return c


def set_config(c: Config | None = None, **kw):
    c = c or default_config(**kw)
    _state["config"] = hashlib.sha256(bytes(c)).hexdigest()
    if live():
        lib().lvr_set_config(C.byref(c))
    return c


def reset():
    _state["map"] = ""
    if live():
        lib().lvr_reset()


def state_to_pose(state) -> np.ndarray:
    out = np.zeros(24, np.float32)
    lib().lvr_state_to_pose(lo._p(lo._f64(state), C.c_double), lo._p(out, C.c_float))
    return out


def transform(state, scan_xyz) -> np.ndarray:
    p = lo._f32(scan_xyz).reshape(-1, 3)
    out = np.empty_like(p)
    lib().lvr_transform(lo._p(lo._f64(state), C.c_double), lo._p(p, C.c_float), C.c_size_t(len(p)), lo._p(out, C.c_float))
    return out


def map_add(xyz, time=0.0, downsample=False):
    p = lo._f32(xyz).reshape(-1, 3)
    h = hashlib.sha256(_state["map"].encode())
    _hash_arg(h, (p, time, downsample))
    _state["map"] = h.hexdigest()
    if not live():
        return
    lib().lvr_map_add(lo._p(p, C.c_float), C.c_size_t(len(p)), C.c_double(time), C.c_int(int(downsample)))


def map_size() -> int:
    return int(lib().lvr_map_size())


def map_fetch() -> np.ndarray:
    out = np.zeros((map_size(), 3), np.float32)
    lib().lvr_map_fetch(lo._p(out, C.c_float))
    return out


def match(state, scan_xyz) -> dict:
    p = lo._f32(scan_xyz).reshape(-1, 3)
    n = len(p)
    src, pw, abcd, dist = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.float32)
    k = lib().lvr_match(lo._p(lo._f64(state), C.c_double), lo._p(p, C.c_float), C.c_size_t(n), lo._p(src, C.c_uint32), lo._p(pw, C.c_float),
                        lo._p(abcd, C.c_float), lo._p(dist, C.c_float))
    return dict(src=src[:k].copy(), p_world=pw[:k].copy(), abcd=abcd[:k].copy(), dist=dist[:k].copy())


def plane(near_xyz, sq_dists):
    p = lo._f32(near_xyz).reshape(-1, 3)
    sq = lo._f32(sq_dists)
    abcd = np.zeros(4, np.float32)
    ok = lib().lvr_plane(lo._p(p, C.c_float), lo._p(sq, C.c_float), C.c_int(len(p)), lo._p(abcd, C.c_float))
    return bool(ok), abcd


def estimate_plane(near_xyz) -> np.ndarray:
    p = lo._f32(near_xyz).reshape(-1, 3)
    abcd = np.zeros(4, np.float32)
    lib().lvr_estimate_plane(lo._p(p, C.c_float), C.c_int(len(p)), lo._p(abcd, C.c_float))
    return abcd


def calculate_H(state, p_world, abcd):
    pw, ab = lo._f32(p_world).reshape(-1, 3), lo._f32(abcd).reshape(-1, 4)
    n = len(pw)
    H, h, dist = np.zeros((n, 12)), np.zeros(n), np.zeros(n, np.float32)
    lib().lvr_calculate_H(lo._p(lo._f64(state), C.c_double), C.c_size_t(n), lo._p(pw, C.c_float), lo._p(ab, C.c_float), lo._p(H, C.c_double),
                          lo._p(h, C.c_double), lo._p(dist, C.c_float))
    return H, h, dist


def update(state, P, scan_xyz):
    x = lo._f64(state).copy()
    Pm = lo._f64(P).copy()
    p = lo._f32(scan_xyz).reshape(-1, 3)
    sums = (lo.IterOut * 16)()
    tr = np.zeros((16, 26))
    n = lib().lvr_update(lo._p(x, C.c_double), lo._p(Pm, C.c_double), lo._p(p, C.c_float), C.c_size_t(len(p)), sums, lo._p(tr, C.c_double))
    return x, Pm.reshape(23, 23), int(n), tr[:n].copy(), [sums[i].as_dict() for i in range(n)]


def initialize(a, w, q_xyzw, t):
    x, P = np.zeros(26), np.zeros((23, 23))
    lib().lvr_initialize(lo._p(lo._f32(a), C.c_float), lo._p(lo._f32(w), C.c_float), lo._p(lo._f32(q_xyzw), C.c_float), C.c_double(t),
                         lo._p(x, C.c_double), lo._p(P, C.c_double))
    return x, P


def propagate(state, P, last_time_integrated, imu_a, imu_w, imu_t, t):
    x, Pm = lo._f64(state).copy(), lo._f64(P).copy()
    a, w, ts = lo._f32(imu_a).reshape(-1, 3), lo._f32(imu_w).reshape(-1, 3), lo._f64(imu_t)
    lib().lvr_propagate(lo._p(x, C.c_double), lo._p(Pm, C.c_double), C.c_double(last_time_integrated), lo._p(a, C.c_float), lo._p(w, C.c_float),
                        lo._p(ts, C.c_double), C.c_size_t(len(ts)), C.c_double(t))
    return x, Pm.reshape(23, 23)


def state_integrate(state, a, w, t):
    s = state.copy()
    lib().lvr_state_integrate(s.ctypes.data_as(C.c_void_p), lo._p(lo._f32(a), C.c_float), lo._p(lo._f32(w), C.c_float), C.c_double(t))
    return s


def deskew(xyz, times, states, Xt2):
    p, t = lo._f32(xyz).reshape(-1, 3), lo._f64(times)
    st = np.ascontiguousarray(states)
    out = np.full_like(p, np.nan)
    k = lib().lvr_deskew(lo._p(p, C.c_float), lo._p(t, C.c_double), C.c_size_t(len(p)), st.ctypes.data_as(C.c_void_p), C.c_size_t(len(st)),
                         np.ascontiguousarray(Xt2).ctypes.data_as(C.c_void_p), lo._p(out, C.c_float))
    return out, int(k)


def path(states, imu_a, imu_w, imu_t, t1, t2, cap=4096):
    st = np.ascontiguousarray(states)
    a, w, ts = lo._f32(imu_a).reshape(-1, 3), lo._f32(imu_w).reshape(-1, 3), lo._f64(imu_t)
    out = np.zeros(cap, lo.MOTION_DTYPE)
    k = lib().lvr_path(st.ctypes.data_as(C.c_void_p), C.c_size_t(len(st)), lo._p(a, C.c_float), lo._p(w, C.c_float), lo._p(ts, C.c_double),
                       C.c_size_t(len(ts)), C.c_double(t1), C.c_double(t2), out.ctypes.data_as(C.c_void_p), C.c_size_t(cap))
    return out[:k].copy()


_DT = {"i1": 1, "u1": 2, "i2": 3, "u2": 4, "i4": 5, "u4": 6, "f4": 7, "f8": 8}


def cloud_ingest(raw: bytes, n: int, dtype: np.dtype, stamp_usec: int) -> np.ndarray:
    """PointCloudProcessor::msg2points -> downsample -> sort_points on a message whose fields are those of the numpy record
    dtype (names, offsets, types) — Config.LiDAR_type etc. as set by set_config."""
    names = list(dtype.names)
    arr = (C.c_char_p * len(names))(*[s.encode() for s in names])
    offs = np.array([dtype.fields[k][1] for k in names], np.uint32)
    dts = np.array([_DT[dtype.fields[k][0].str.lstrip("<|=")] for k in names], np.uint8)
    out = np.zeros(max(n, 1), lo.POINT_DTYPE)
    buf = (C.c_uint8 * len(raw)).from_buffer_copy(raw)
    k = lib().lvr_cloud_ingest(buf, C.c_size_t(n), C.c_uint32(dtype.itemsize), C.c_int(len(names)), arr, lo._p(offs, C.c_uint32), lo._p(dts, C.c_uint8),
                               C.c_uint64(stamp_usec), out.ctypes.data_as(C.c_void_p))
    return out[:k].copy()


def buffer_window(times, t1, t2, clear_t=None) -> np.ndarray:
    t = lo._f64(times)
    out = np.zeros(len(t))
    k = lib().lvr_buffer_window(lo._p(t, C.c_double), C.c_size_t(len(t)), C.c_double(t1), C.c_double(t2),
                                C.c_double(-1e301 if clear_t is None else clear_t), lo._p(out, C.c_double))
    return out[:k].copy()


# ---- record / replay of the library's answers (tests/golden/ref_calls.npz) --------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(_HERE), "tests", "golden", "ref_calls.npz")
_state = {"config": hashlib.sha256(bytes(default_config())).hexdigest(), "map": ""}
_live = None
_golden = None
_recorded = {}


def live() -> bool:
    """True when the library itself answers (built here, or prebuilt); False when calls are replayed from GOLDEN."""
    global _live
    if _live is None:
        _live = build() is not None
    return _live


def available() -> bool:
    return live() or os.path.exists(GOLDEN)


# floating-point (and record) answers of these functions are recorded as digests: every use the tests make of them is a bitwise
# comparison, a length / shape, or an argument to another call here (integer answers such as match's `src` stay whole)
DIGESTED = ("transform", "match", "calculate_H", "map_fetch", "cloud_ingest")


def digest(a) -> str:
    """SHA-256 of an array's dtype, shape and bytes (a Pinned is its own digest)."""
    if isinstance(a, Pinned):
        return a.digest
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.descr}{a.shape}".encode() + a.tobytes()).hexdigest()[:32]


class Pinned:
    """A replayed answer kept as its digest: it has a length, a shape, the fields of a record array, and its bits can be compared
    (same_bits) or handed back to this module as an argument."""

    def __init__(self, dig, shape, fields=None):
        self.digest, self.shape = dig, tuple(shape)
        self.fields = {k: Pinned(*v) for k, v in (fields or {}).items()}

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, name):
        return self.fields[name]


def same_bits(a, b) -> bool:
    """Bitwise equality (dtype, shape and every bit) of two arrays, either of which may be a Pinned."""
    return digest(a) == digest(b)


def _pin(a) -> list:
    names = [f for f in (a.dtype.names or ()) if f != "pad_"]
    return [digest(a), list(a.shape), {f: [digest(a[f]), list(a[f].shape)] for f in names} or None]


def _hash_arg(h, v):
    if isinstance(v, (np.ndarray, Pinned)):
        h.update(f"A{digest(v)}".encode())
    elif isinstance(v, (list, tuple)):
        h.update(f"L{len(v)}".encode())
        for x in v:
            _hash_arg(h, x)
    elif isinstance(v, bytes):
        h.update(b"B%d" % len(v) + v)
    elif isinstance(v, np.dtype):
        h.update(f"D{v.descr}{v.itemsize}".encode())
    elif isinstance(v, (bool, np.bool_)):
        h.update(f"b{bool(v)}".encode())
    elif isinstance(v, (int, np.integer)):
        h.update(f"i{int(v)}".encode())
    elif isinstance(v, (float, np.floating)):
        h.update(f"f{float(v).hex()}".encode())
    elif v is None:
        h.update(b"N")
    else:
        raise TypeError(f"lvref: cannot key an argument of type {type(v).__name__}")


def _key(name, args, kw) -> str:
    h = hashlib.sha256(f"{name}|{_state['config']}|{_state['map']}".encode())
    _hash_arg(h, list(args))
    for k in sorted(kw):
        h.update(k.encode())
        _hash_arg(h, kw[k])
    return h.hexdigest()[:16]


def _encode(v, leaves, pin=False):
    if isinstance(v, np.ndarray):
        if v.dtype.names and "pad_" in v.dtype.names:   # (whatever the library left in the padding is no answer of it)
            v = v.copy()
            v["pad_"] = 0
        if pin and (v.dtype.names or v.dtype.kind == "f"):
            return {"p": _pin(v)}
        leaves.append(np.ascontiguousarray(v))
        return {"a": len(leaves) - 1}
    if isinstance(v, dict):
        return {"d": {k: _encode(x, leaves, pin) for k, x in v.items()}}
    if isinstance(v, (list, tuple)):
        return {"l" if isinstance(v, list) else "t": [_encode(x, leaves, pin) for x in v]}
    if isinstance(v, (bool, np.bool_)):
        return {"b": bool(v)}
    if isinstance(v, (int, np.integer)):
        return {"i": int(v)}
    if isinstance(v, (float, np.floating)):
        return {"f": float(v).hex()}
    raise TypeError(f"lvref: cannot record an output of type {type(v).__name__}")


def _decode(spec, leaves):
    (tag, v), = spec.items()
    if tag == "a":
        return leaves[v].copy()
    if tag == "p":
        return Pinned(*v)
    if tag == "d":
        return {k: _decode(x, leaves) for k, x in v.items()}
    if tag in ("l", "t"):
        out = [_decode(x, leaves) for x in v]
        return out if tag == "l" else tuple(out)
    return {"b": bool, "i": int, "f": float.fromhex}[tag](v)


def _load(path) -> dict:
    """{key: (spec, [arrays])} from a record file."""
    with np.load(path, allow_pickle=False) as z:
        index, sizes = json.loads(lzma.decompress(z["index"].tobytes()))
        blob = lzma.decompress(z["blob"].tobytes())
    offsets = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
    arrays = [np.load(io.BytesIO(blob[offsets[i]:offsets[i + 1]]), allow_pickle=False) for i in range(len(sizes))]
    return {k: (spec, [arrays[i] for i in ids]) for k, (spec, ids) in index.items()}


def _save(path, records: dict):
    """Every array as a .npy image, all of them behind ONE LZMA stream (the calls repeat one another's data: its window finds it)."""
    index, chunks = {}, []
    for k in sorted(records):
        spec, arrays = records[k]
        ids = []
        for a in arrays:
            buf = io.BytesIO()
            np.save(buf, a, allow_pickle=False)
            chunks.append(buf.getvalue())
            ids.append(len(chunks) - 1)
        index[k] = (spec, ids)
    blob = lzma.compress(b"".join(chunks), preset=9)
    index = lzma.compress(json.dumps([index, [len(c) for c in chunks]], sort_keys=True).encode(), preset=9)
    np.savez(path, index=np.frombuffer(index, np.uint8), blob=np.frombuffer(blob, np.uint8))


def _same(a, b) -> bool:
    (sa, la), (sb, lb) = a, b
    return sa == sb and len(la) == len(lb) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
                                                   for x, y in zip(la, lb))


def _golden_records() -> dict:
    global _golden
    if _golden is None:
        _golden = _load(GOLDEN) if os.path.exists(GOLDEN) else {}
    return _golden


def _write_record():
    path = GOLDEN if os.environ["LV_REF_RECORD"] == "1" else os.environ["LV_REF_RECORD"]
    records = _load(path) if os.path.exists(path) else {}
    records.update(_recorded)
    _save(path, records)


def _pinned(fn):
    @functools.wraps(fn)
    def call(*args, **kw):
        key_args = args
        if fn.__name__ == "cloud_ingest":    # the message's fields, not the bytes between them (a permuted copy leaves those undefined)
            raw, n, dtype = args[:3]
            rec = np.frombuffer(raw, dtype, count=n)
            key_args = ([np.ascontiguousarray(rec[f]) for f in dtype.names],) + tuple(args[1:])
        key = _key(fn.__name__, key_args, kw)
        if not live():
            rec = _golden_records().get(key)
            if rec is None:
                raise KeyError(f"lvref.{fn.__name__}: no recorded answer of the reference library for this call (inputs or "
                               f"configuration differ from the recording); rerun the tests with the library and LV_REF_RECORD=1")
            return _decode(rec[0], rec[1])
        out = fn(*args, **kw)
        leaves = []
        rec = (_encode(out, leaves, fn.__name__ in DIGESTED), leaves)
        if os.environ.get("LV_REF_RECORD"):
            if not _recorded:
                atexit.register(_write_record)
            _recorded[key] = rec
        elif key in _golden_records():
            assert _same(_golden_records()[key], rec), f"lvref.{fn.__name__}: the library's answer differs from {GOLDEN}"
        return out
    return call


for _name in ("state_to_pose", "transform", "map_size", "map_fetch", "match", "plane", "estimate_plane", "calculate_H", "update",
              "initialize", "propagate", "state_integrate", "deskew", "path", "cloud_ingest", "buffer_window"):
    globals()[_name] = _pinned(globals()[_name])
