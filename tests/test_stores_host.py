"""The reserve paths of the map, scan and cloud stores (limo-velo_amd/csrc/lv_stores.hpp: MapStore, ScanStore, CloudStore) compiled
with g++ and -fsanitize=address,undefined through tests/emu/hip/hip_runtime.h: tests/emu/stores_emu.cpp runs one case per call and
prints what the stand-in's call log, its mallocs / frees counters and its fail hook saw.  Held here: the growth of every path at its
floor, one past it and at five times it; what a growth keeps; a failure at every HIP call of every path; a release without leaks.
The rules are those of DESIGN.md "Host-side buffers"."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
LV_OK = 0


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stores_host") / "stores_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "stores_emu.cpp"), "-o",
                           str(exe)])

    def run(case):
        out = subprocess.run([str(exe), case], stdout=subprocess.PIPE, check=True).stdout.decode().strip().split("\n")
        facts = {}
        for ln in out:
            name, *vals = ln.split()
            facts.setdefault(name, []).append(vals)
        return facts

    return run


def _ints(vals):
    return [int(v) for v in vals]


def _tmp64(n):   # the stand-in's scratch formulas (stores_emu.cpp)
    return 16 * n + 256


def _scan_tmp(n):
    return n // 8 + 64


def test_growth_at_the_floor_one_past_it_and_at_five_times_it(emu):
    f = emu("growth")
    caps = (4096, 8192, 32768)                                       # requests of 4096, 4097, 20480
    assert [_ints(v) for v in f["map_reserve"]] == [[LV_OK, c, c, c, c, _tmp64(c)] for c in caps]
    assert [_ints(v) for v in f["map_alive"]] == [[LV_OK, c, c, _scan_tmp(c)] for c in caps]   # exact: the id capacity
    assert [_ints(v) for v in f["map_boxes"]] == [[LV_OK, 4 * c, 4 * c, c] for c in caps]      # the box table: next_pow2(4 x capacity)
    for v, c in zip(f["map_batch"], caps):
        gtab, reloc = 4 * c, 27 * c
        broken, comp, cstage = max(16384, 2 * c), min(reloc, 1 << 18), max(1 << 20, 32 * c)
        assert _ints(v) == [LV_OK, c, gtab, reloc, broken, comp, cstage, 27 * c, 28 * gtab, reloc, broken, cstage, max(_tmp64(c), _scan_tmp(c))]
    assert [_ints(v) for v in f["scan_reserve"]] == [[LV_OK, c, c, 8 * c + 256] for c in caps]
    assert [_ints(v) for v in f["scan_raw"]] == [[LV_OK, c, c, _tmp64(c), _scan_tmp(c), s, 8] for c, s in zip(caps, (2, 70, 70))]
    tiles = [_ints(v) for v in f["scan_tiles"]]                      # 0, 1, 1024, 1025, 5000 tiles: doubling from 1024
    assert [t[1] for t in tiles] == [0, 1024, 1024, 2048, 8192] and all(t[0] == LV_OK for t in tiles)
    assert [t[2] - tiles[0][2] for t in tiles] == [0, 1, 1, 2, 3]    # no tiles: nothing allocated
    msg = (65536, 131072, 524288)                                    # 65536, 65537, 327680 points of 16 bytes
    raw = (1 << 20, 2 << 20, 8 << 20)                                # 1 MiB, 1 MiB + 16, 5 MiB
    assert [_ints(v) for v in f["cloud_msg"]] == [[LV_OK, m, r, m, max(m + 128, _tmp64(m)), r, r] for m, r in zip(msg, raw)]
    assert [_ints(v) for v in f["cloud_buffer"]] == [[LV_OK, 1 << 18], [LV_OK, 1 << 19], [LV_OK, 1 << 21]]
    # larger stagings: the device is waited for BEFORE a pinned block is freed
    rc, *log = f["cloud_msg_log"][0]
    assert int(rc) == LV_OK and log[0] == "hipDeviceSynchronize" and log.count("hipHostFree") == 2 and log.count("hipHostMalloc") == 2
    m, fr = _ints(f["released"][0])
    assert m == fr


def test_growth_keeps_what_is_by_id_and_the_living_range(emu):
    f = emu("contents")
    # the points alone: kept across 4096 -> 8192 in a new block; no chains or positions appear that were not there
    assert _ints(f["orig_alone"][0]) == [LV_OK, 8192, 1, 1, 1, 1]
    # 8192 -> 16384 with d_box_next, d_backpos[l], d_cellpos in place: the first n_ids elements of each are the old ones
    assert _ints(f["by_id"][0]) == [LV_OK, 16384, 1, 1, 1, 1, 16384, 16384, 16384 * 27]
    assert f["orig_log"][0] == ["hipMalloc", "hipDeviceSynchronize", "hipMemcpyAsync", "hipStreamSynchronize", "hipFree"]
    # the LiDAR buffer: [head, size) moves to the front in place when it fits there ...
    rc, cap0, cap1, kept, mallocs, *log = f["cloud_move"][0]
    assert _ints([rc, cap0, cap1, kept, mallocs]) == [LV_OK, 1 << 18, 1 << 18, 1, 0] and log == ["hipMemcpyAsync@1"]
    # ... and into a block of twice the size when it does not: allocate, copy, wait, free
    rc, cap0, cap1, kept, mallocs, *log = f["cloud_grow"][0]
    assert _ints([rc, cap0, cap1, kept, mallocs]) == [LV_OK, 1 << 18, 1 << 19, 1, 1]
    assert log == ["hipMalloc", "hipMemcpyAsync@1", "hipStreamSynchronize@1", "hipFree"]
    m, fr = _ints(f["released"][0])
    assert m == fr


PATHS = ("map_reserve_first", "map_reserve_grow", "map_reserve_batch_first", "map_reserve_batch_grow", "map_alive_scratch_first",
         "map_alive_scratch_grow", "map_counters", "map_boxes_first", "map_boxes_grow", "scan_reserve_first", "scan_reserve_grow",
         "scan_raw_first", "scan_raw_grow", "scan_tiles_first", "scan_tiles_grow", "cloud_init", "cloud_msg_first", "cloud_msg_grow",
         "cloud_buffer_first", "cloud_buffer_grow", "cloud_buffer_move")


def test_a_failure_at_every_call_of_every_path(emu):
    f = emu("failures")
    rows = {v[0]: v[1:] for v in f["path"]}
    assert tuple(rows) == PATHS
    for name, (calls, again, again_calls, ehip, sound, retried, same, first_bad) in rows.items():
        calls = int(calls)
        assert calls >= 1, name
        assert (int(again), int(again_calls)) == (LV_OK, 0), name    # the request again, now that it fits: no HIP call at all
        # call k failing, for every k: LV_EHIP; no group field over the cap of a member; the request again is LV_OK and leaves
        # every capacity as a clean run leaves it
        assert (int(ehip), int(sound), int(retried), int(same), first_bad) == (calls, calls, calls, calls, "-"), name
    # the calls of a first reserve: one allocation per buffer (+ the waits and copies of grow_keep for d_orig)
    assert int(rows["map_reserve_first"][0]) == 3 + 8 and int(rows["scan_reserve_first"][0]) == 7
    assert int(rows["map_reserve_grow"][0]) == 5 + 2 * 8 + 4 * 5     # d_orig kept; 8 reallocated; chains, 2 x back-positions, list positions kept
    mallocs, frees, as_new, ev_made, ev_gone = _ints(f["released"][0])
    assert mallocs == frees and as_new == 1 and ev_made == ev_gone > 0


def test_design_cites_the_rules_for_these_stores():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### Host-side buffers (`lv_buffers.hpp`)"):]
    sec = sec[:sec.index("\n### ", 10)]
    for store in ("MapStore", "ScanStore", "CloudStore"):
        assert store in sec
    assert re.search(r"^4\. \*\*", sec, re.M) and "grow_keep" in sec
    cite = sec[sec.index("`MapStore`, `ScanStore` and `CloudStore`"):]
    assert all(f"rule {r}" in cite or f"rules {r}" in cite or f", {r}" in cite for r in (1, 2, 4))
