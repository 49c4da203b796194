"""The HIP path against the REFERENCE'S OWN CODE, without the oracle in between: oracle/_ref/liblvref.so (/root/reference/src
compiled in place, tests/test_oracle_ref.py) driven through its C glue on the same seeded inputs as the GPU context.  Where
the library is absent its answers recorded in tests/golden/ref_calls.npz stand in for it (oracle/lvref.py).

What equality here means: for every scan point, what Mapper::match / Plane / R3Math / Match / Localizator::calculate_H of the
reference compute (world point, chosen set, plane, residual, Jacobian row) are the bits lv_iterate's per-point outputs carry,
and a whole Localizator::correct lands on lv_update's posterior.  The reference-side kNN and filter algebra are stand-ins
(exact search; the oracle's esekf restatement) — see oracle/ref_build/slam/."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lr(oracle, lv):
    import lvref

    lvref.set_config()
    lvref.reset()
    return lvref


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("extrinsics,est", [("identity", False), ("xaloc", True)])
def test_per_point_outputs_equal_the_reference_code(capi, lr, extrinsics, est):
    from limo_velo_amd import synth

    sc = synth.make_scene(50_000, 2_000, extrinsics=extrinsics)
    lr.set_config(estimate_extrinsics=int(est))
    lr.reset()
    lr.map_add(sc["map_xyz"])
    with capi.Context(capi.default_params(estimate_extrinsics=int(est))) as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        for x in (sc["x_init"], sc["x_true"]):
            m = lr.match(x, sc["scan_xyz"])
            ctx.iterate(x)
            valid, pw, abcd, dist = ctx.fetch_matches()
            H, h = ctx.fetch_rows()
            v = valid.astype(bool)
            assert np.array_equal(np.nonzero(v)[0], m["src"])                      # the chosen set (Match::is_chosen)
            assert lr.same_bits(pw, lr.transform(x, sc["scan_xyz"]))               # Mapper.cpp:51 for EVERY point
            assert lr.same_bits(pw[v], m["p_world"])
            assert lr.same_bits(abcd[v], m["abcd"])                                 # R3Math::estimate_plane behind Plane's gates
            assert lr.same_bits(dist[v], m["dist"])                                 # Plane::dist_to_plane
            Hr, hr, _ = lr.calculate_H(x, m["p_world"], m["abcd"])                  # Localizator::calculate_H
            assert lr.same_bits(H[v], Hr) and lr.same_bits(h[v], hr)
            Hc, hc = ctx.calculate_H(x, pw[v], abcd[v], dist[v])                   # the drop-in entry point lv_calculate_H, on the
            assert lr.same_bits(Hc, Hr) and lr.same_bits(hc, hr)                    # reference's matches (the bits asserted above)
    lr.set_config()


@pytest.mark.parametrize("name,mdp,pth", [("kitti", 2.23, 0.1), ("ouster", 2.0, 0.1)])
def test_shipped_yaml_keys_on_ring_scans_equal_the_reference_code(capi, lr, name, mdp, pth):
    """config/kitti.yaml / ouster.yaml hot keys (MAX_DIST_PLANE, PLANES_THRESHOLD) on a spinning-LiDAR scan (16 rings x 1024 azimuth
    steps against a 300 k-point map: grazing incidence, sparse far rings — many points fail a gate): chosen set, planes, residuals
    and rows of the HIP path equal Mapper::match + Localizator::calculate_H of the reference's compiled sources."""
    from limo_velo_amd import synth

    sc = synth.make_ring_scene(300_000, 16, 1024)
    lr.set_config(max_dist_plane=mdp, planes_threshold=pth)
    lr.reset()
    lr.map_add(sc["map_xyz"])
    with capi.Context(capi.default_params(MAX_DIST_PLANE=mdp, PLANES_THRESHOLD=pth)) as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        m = lr.match(sc["x_init"], sc["scan_xyz"])
        ctx.iterate(sc["x_init"])
        valid, pw, abcd, dist = ctx.fetch_matches()
        H, h = ctx.fetch_rows()
        v = valid.astype(bool)
        assert 0.2 * len(v) < v.sum() < len(v)
        assert np.array_equal(np.nonzero(v)[0], m["src"])
        assert lr.same_bits(abcd[v], m["abcd"]) and lr.same_bits(dist[v], m["dist"])
        Hr, hr, _ = lr.calculate_H(sc["x_init"], m["p_world"], m["abcd"])
        assert lr.same_bits(H[v], Hr) and lr.same_bits(h[v], hr)
    lr.set_config()


def test_iterated_update_lands_on_the_reference_glue_posterior(capi, lr):
    from limo_velo_amd import synth

    sc = synth.make_scene(50_000, 2_000)
    lr.set_config()
    lr.reset()
    lr.map_add(sc["map_xyz"])
    xr, Pr, nr, trr, sr = lr.update(sc["x_init"], sc["P0"], sc["scan_xyz"])
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        x, P, n, tr, sums = ctx.update(sc["x_init"], sc["P0"])
    assert n == nr
    assert [s["n_valid"] for s in sums] == [s["n_valid"] for s in sr]
    assert np.abs(x - xr).max() < 1e-9 and np.abs(P - Pr).max() < 1e-9 * max(1.0, np.abs(Pr).max())
    lr.reset()


def test_deskew_window_against_the_reference_compensator(capi, lr, oracle):
    """Row f-2 on the device against Compensator::compensate compiled from the reference: the device evaluates sin / cos by the
    pinned polynomial, the reference by this platform's libm — so the bar is the rounding of one sin / cos per point (a few f32
    ulps of a coordinate up to 60 m), and exact equality wherever the angular rate is zero."""
    rng = np.random.default_rng(4)
    for w in ([0.0, 0.0, 0.0], [0.02, -0.05, 0.4]):
        states, cur = [], oracle.motion_state(R=np.linalg.qr(rng.normal(size=(3, 3)))[0].astype(np.float32), pos=[3, -2, 1.5], vel=[4, 0.5, 0.1],
                                              a=[0.3, 0.1, 9.8], w=w, time=50.0, tLI=[0.05, 0.0, -0.1])
        for i in range(12):
            states.append(cur.copy())
            cur = oracle.state_integrate(cur, rng.normal(0, 0.5, 3) + [0, 0, 9.8], np.asarray(w) * rng.uniform(0.5, 1.5), 50.0 + 0.01 * (i + 1))
        states = np.concatenate(states)
        times = np.sort(rng.uniform(50.0, 50.11, 3000))
        xyz = rng.uniform(-60, 60, (3000, 3)).astype(np.float32)
        Xt2 = oracle.state_integrate(states[-1:].copy(), states[-1]["a"], states[-1]["w"], 50.11)
        ref, k = lr.deskew(xyz, times, states, Xt2)
        assert k == 3000
        with capi.Context() as ctx:
            ctx.scan_deskew(xyz, times, states, Xt2, 0.0)      # no voxel grid: the scan keeps every point (Morton order)
            got = ctx.scan_fetch()
        key = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]
        if not any(w):
            assert np.array_equal(_bits(key(got[:, :3])), _bits(key(ref)))
        else:
            assert np.abs(key(got[:, :3]) - key(ref)).max() < 2e-4


def test_reference_main_loop_trajectory_beside_the_hip_pipeline(lr, lv, tmp_path):
    """The same recorded stream through (a) the reference's own main loop (oracle/_ref/ref_stream_demo: src/main.cpp and every
    in-tree source compiled in place, stand-ins for kNN / esekf algebra / voxel grid) and (b) the reference's loop over the shim
    and the HIP library (limo-velo_amd/host/stream_demo, both hand-over modes): the same localisation schedule (every t2), the
    same number of points in every update, scans handed to correct() that differ by f32 rounding only (first update 4.8e-7 m max —
    the reference's de-skew takes libm's sinf / cosf, the device a polynomial one ulp away in 2 % of the arguments — later ones
    1e-6 m in the mean as the states they are de-skewed with differ at that level), and trajectories that agree by block: position
    <= 2e-5 m, attitude <= 2e-6, velocity <= 5e-4 m/s (observed through consecutive positions: 1 / delta = 100 times the position
    noise) over the first twenty updates; later ones within what an update sitting on the LIMITS threshold may move the weakly
    observable states (the bound the two HIP hand-over modes are held to against each other)."""
    import os
    import subprocess
    import sys

    from limo_velo_amd import synth

    ref_exe = os.path.join(os.path.dirname(lr._LIB_PATH), "ref_stream_demo")
    if not os.path.exists(ref_exe):
        pytest.skip("oracle/_ref/ref_stream_demo did not travel with this snapshot")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "limo-velo_amd", "host")
    exe = os.path.join(host, "stream_demo")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", host])
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_gpu_shim as S

    n_revs, delta = 9, 0.01
    stream = synth.make_stream(1_048_576, n_revs, n_az=512, map_radius=62.0)
    # The synthetic firing times are multiples of 0.1 / 512 s, so every 50 ms one of them EQUALS a window end t2 exactly — and there
    # the reference's window is not the inclusive one: Accumulator::get starts its walk at before_t(t2) - 1 (Accumulator.hpp:73-87
    # over Utils.hpp:9-23) and so keeps exactly TWO of the points stamped t2 (which two is up to std::sort's order of equal
    # stamps, PointCloudProcessor.cpp:112-121), while every one of them is in the next window; limo-velo_amd takes t1 <= t <= t2.
    # A measure-zero case for a real sensor's stamps (test_window_boundary_quirk below pins it); the stamps are moved off the
    # lattice here so that the two pipelines see the same windows.
    for rev in stream["revs"]:
        rev["t"] = rev["t"] + 3.3e-7
    pos0, _, vel0, _, q0 = synth.stream_truth(0.30 - 0.1)
    x0 = synth.make_state(pos0 + [0.02, -0.015, 0.01], synth.quat_mul(q0, synth.quat_from_rotvec([0.002, -0.001, 0.003])), vel=vel0,
                          grav=(0, 0, synth.STREAM_G))
    inp = tmp_path / "in.bin"
    S._write_stream_input(inp, 0, delta, stream, n_revs, x0)
    out_ref = tmp_path / "out_ref.bin"
    r = subprocess.run([ref_exe, str(inp), str(out_ref)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, LV_DEMO_DUMP_PREFIX=str(tmp_path / "scan_ref"), LV_DEMO_PASSES_DUMP=str(tmp_path / "passes_ref.txt")))
    assert r.returncode == 0, r.stdout + r.stderr
    tr, xr, nr = S._read_stream_output(out_ref)
    worst = {}
    for on_device in (0, 1):
        inp_d, out_d = tmp_path / f"in{on_device}.bin", tmp_path / f"out{on_device}.bin"
        S._write_stream_input(inp_d, on_device, delta, stream, n_revs, x0)
        r = subprocess.run([exe, str(inp_d), str(out_d)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, LV_DEMO_DUMP_PREFIX=str(tmp_path / f"scan_hip{on_device}"),
                                    LV_DEMO_PASSES_DUMP=str(tmp_path / f"passes_hip{on_device}.txt")))
        assert r.returncode == 0, r.stdout + r.stderr
        t, x, n = S._read_stream_output(out_d)
        if on_device == 0:   # the scans the two loops hand to correct(), update by update (the voxel grid orders them alike)
            for j in range(6):
                a = np.fromfile(str(tmp_path / f"scan_ref_{j}.bin"), np.float32).reshape(-1, 3)
                b = np.fromfile(str(tmp_path / f"scan_hip0_{j}.bin"), np.float32).reshape(-1, 3)
                same = a.shape == b.shape
                dd = np.abs(a - b).max() if same else float("nan")
                print(f"scan of update {j}: {a.shape[0]} vs {b.shape[0]} points, max |d| {dd:.3e}, mean |d| {np.abs(a - b).mean() if same else float('nan'):.3e}")
        k = min(len(t), len(tr))
        assert k >= 50 and abs(len(t) - len(tr)) <= 1
        assert np.allclose(t[:k], tr[:k], atol=1e-12)                      # the same localisation schedule
        assert np.array_equal(n[:k], nr[:k])                               # the same scan sizes after window + voxel grid
        d = np.abs(x[:k] - xr[:k])
        worst[on_device] = (float(d[:20].max()), float(d[:, :3].max()), float(d.max()))
        names = ["pos"] * 3 + ["rot"] * 4 + ["offR"] * 4 + ["offT"] * 3 + ["vel"] * 3 + ["bg"] * 3 + ["ba"] * 3 + ["grav"] * 3
        by_comp = {}
        for j, nm in enumerate(names):
            by_comp[nm] = max(by_comp.get(nm, 0.0), float(d[:20, j].max()))
        print(f"on_device={on_device}: max |dx| over the first 20 updates by block {by_comp}; per update (max over state) {[float('%.2e' % v) for v in d[:24].max(axis=1)]}")
        # by block over the first 20 updates: positions / attitude to the f32 noise of the de-skewed points (1e-6 m per point, mean),
        # velocity 1 / delta = 100 times looser (it is observed through consecutive positions only), biases and gravity between
        tol = {"pos": 2e-5, "rot": 2e-6, "offR": 1e-12, "offT": 1e-12, "vel": 5e-4, "bg": 2e-5, "ba": 2e-5, "grav": 1e-5}
        assert all(by_comp[nm] <= tol[nm] for nm in tol), by_comp
        assert d[:, :3].max() < 1e-3 and d.max() < 3e-3, worst
        # WHICH update makes the tail of the replay looser than its head: the measurement passes every update
        # took, on both sides.  Up to the first update whose pass counts differ the trajectories stay at the head's level; the
        # looser bound above is only ever needed behind such an update (an update sitting on the LIMITS threshold converges one
        # pass earlier on one side, and the weakly observable states — biases, gravity — move by up to LIMITS until the filter
        # has pulled them back together).
        pr = np.loadtxt(str(tmp_path / "passes_ref.txt"), dtype=np.int64)[:k]
        ph = np.loadtxt(str(tmp_path / f"passes_hip{on_device}.txt"), dtype=np.int64)[:k]
        flips = np.nonzero(pr != ph)[0]
        first_flip = int(flips[0]) if len(flips) else k
        per_update = d.max(axis=1)
        print(f"on_device={on_device}: passes differ at updates {flips.tolist()} (reference / HIP passes there: {[(int(pr[i]), int(ph[i])) for i in flips[:6]]}); "
              f"max |dx| before the first one {per_update[:first_flip].max() if first_flip else 0.0:.2e}, from it on {per_update[first_flip:].max() if first_flip < k else 0.0:.2e}")
        assert first_flip >= 20, (first_flip, pr[:24].tolist(), ph[:24].tolist())
        print(f"      before the first differing pass count: positions {d[:first_flip, :3].max():.2e}, velocity {d[:first_flip, 14:17].max():.2e}, everything else "
              f"{np.delete(d[:first_flip], [14, 15, 16], axis=1).max():.2e}; behind it: positions {d[first_flip:, :3].max() if first_flip < k else 0.0:.2e}")
        assert per_update[:first_flip].max() < 5e-4, per_update[:first_flip].max()   # (velocity: 100 x the position noise)
        assert d[:first_flip, :3].max() < 1e-4
        if on_device == 0:
            by_value = (t, x, n)
    print("HIP pipeline vs the reference's main loop: max |dx| first 20 updates / positions overall / all states", worst)
    # (c) the THIRD program: the reference's own src/main.cpp compiled UNCHANGED against the shim (limo-velo_amd/host/Makefile
    # `refmain`: ref_main/Headers/*.hpp put the shim's classes where the reference's headers were, ref_main/ros/ros.h stands where
    # the ROS master stood) on the same stream.  stream_demo runs host/main_loop.hpp, a hand restatement of main.cpp:52-128 — so
    # the two must agree BIT FOR BIT, update by update: the loop a maintainer keeps is the reference's file itself.
    main_exe = os.path.join(os.path.dirname(lr._LIB_PATH), "ref_main_over_shim")
    if not os.path.exists(main_exe):
        pytest.skip("oracle/_ref/ref_main_over_shim did not travel with this snapshot")
    out_m = tmp_path / "out_main.bin"
    r = subprocess.run([main_exe, str(tmp_path / "in0.bin"), str(out_m)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    tm, xm, nm_ = S._read_stream_output(out_m)
    t0_, x0_, n0_ = by_value
    assert len(tm) == len(t0_) and len(tm) >= 50, (len(tm), len(t0_))
    assert np.array_equal(tm, t0_) and np.array_equal(nm_, n0_)
    assert np.array_equal(xm.view(np.uint64), x0_.view(np.uint64)), f"max |dx| {np.abs(xm - x0_).max():.3e}"
    print(f"the reference's src/main.cpp over the shim == stream_demo (main_loop.hpp): {len(tm)} updates, states bit-equal")
