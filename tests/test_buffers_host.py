"""The host-side buffers of the map tools (limo-velo_amd/csrc/lv_buffers.hpp: DevBuf / PinBuf, PointStage, Counters4, blocks_of)
compiled with g++ and -fsanitize=address,undefined through tests/emu/hip/hip_runtime.h: tests/emu/buffers_emu.cpp runs one case
per call and prints what the stand-in's call log, its mallocs / frees counters and its fail hook saw.  The rules held here are
those of DESIGN.md "Host-side buffers"."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
LV_OK = 0


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("buffers_host") / "buffers_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "buffers_emu.cpp"), "-o",
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


def test_exact_growth(emu):
    f = emu("exact")
    assert _ints(f["first"][0]) == [LV_OK, 1, 100, 100 * 8]          # rc, hipMallocs, cap, bytes asked for
    assert _ints(f["same"][0]) == [LV_OK, 1, 0]                      # the same n again: no call at all
    assert _ints(f["smaller"][0]) == [LV_OK, 1, 0, 100]              # a smaller n: none, the capacity stands
    assert f["larger"][0] == ["hipFree", "hipMalloc"]                # a larger n: one free, then one allocation ...
    assert _ints(f["larger_bytes"][0]) == [LV_OK, 101, 101 * 8]      # ... of exactly n * sizeof(T)
    assert _ints(f["released"][0]) == [1, 0, 2, 2]                   # {nullptr, 0}, mallocs == frees
    assert _ints(f["bytes"][0]) == [LV_OK, 37, 37]                   # the byte form counts bytes
    assert _ints(f["zero"][0]) == [LV_OK, 1, 3, 3]                   # room for nothing allocates nothing


def test_doubling_growth(emu):
    f = emu("doubling")
    caps = [_ints(v) for v in f["cap"]]
    assert [c[1] for c in caps] == [1024, 1024, 2048, 8192]          # n = 1, 1024, 1025, 5000 from a floor of 1024
    assert [c[2] for c in caps] == [4096, 4096, 8192, 32768]
    assert [c[3] for c in caps] == [1, 1, 2, 3] and all(c[0] == LV_OK for c in caps)
    assert _ints(f["bytes"][0]) == [LV_OK, 8192, 8192]               # 4097 bytes from a floor of 4096
    m, fr = _ints(f["released"][0])
    assert m == fr == 4


def test_failure_and_release(emu):
    f = emu("failure")
    assert _ints(f["before"][0]) == [LV_OK, 8, 8]
    assert _ints(f["dev_failed"][0]) == [1, 1, 0, 1]                 # LV_EHIP, {nullptr, 0}, the error names the HIP failure
    assert _ints(f["pin_failed"][0]) == [1, 1, 0]
    assert _ints(f["dev_again"][0]) == [LV_OK, 1, 4, 1]              # the next call allocates, whatever its size
    assert _ints(f["pin_again"][0]) == [LV_OK, 1, 4, 1]
    m, fr = _ints(f["released"][0])
    assert m == fr == 4


def test_growth_that_keeps_contents(emu):
    f = emu("keep")
    assert f["empty"][0] == ["hipMalloc", "hipStreamSynchronize@1"]  # growth from empty: no copy, no free
    assert _ints(f["from_empty"][0]) == [LV_OK, 8, 1]
    # allocate, copy on the stream, wait, and only then free the old block
    assert f["stream"][0] == ["hipMalloc", "hipMemcpyAsync@1", "hipStreamSynchronize@1", "hipFree"]
    assert _ints(f["kept"][0]) == [LV_OK, 16, 16 * 4, 102, 103, 104, 105, 106]   # elements [2, 7) of the old block lead the new one
    assert f["device"][0] == ["hipMalloc", "hipDeviceSynchronize", "hipMemcpyAsync", "hipStreamSynchronize", "hipFree"]
    assert _ints(f["kept_device"][0]) == [LV_OK, 32, 102, 106]
    assert f["none"][0] == ["hipMalloc", "hipStreamSynchronize@1", "hipFree"]    # keep == 0: a new block and the wait, no copy
    assert _ints(f["kept_none"][0]) == [LV_OK, 64, 1]
    # the allocation, the copy or the wait failing: LV_EHIP, the old block and capacity untouched and readable, the new block freed
    assert [v[0] for v in f["failed"]] == ["hipMalloc", "hipMemcpyAsync", "hipStreamSynchronize"]
    assert all(_ints(v[1:]) == [1, 1, 64, 21, 0] for v in f["failed"])
    assert _ints(f["after"][0]) == [LV_OK, 128, 21]                  # ... and the same call again succeeds
    assert f["bytes"][0] == [str(LV_OK), "32", "abcdef"]             # the byte form counts bytes
    m, fr = _ints(f["released"][0])
    assert m == fr == 9


def test_point_stage(emu):
    f = emu("stage")
    assert _ints(f["empty"][0]) == [LV_OK, 0, 1, 1]                  # 0 points: nothing allocated, nothing uploaded
    # the wait comes first; then the allocations, then one upload on the same stream
    assert f["first"][0] == ["hipStreamSynchronize@1", "hipHostMalloc", "hipMalloc", "hipMemcpyAsync@1"]
    rc, n, *xyz = f["packed"][0]
    assert (int(rc), int(n)) == (LV_OK, 5)
    assert [float(v) for v in xyz] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 100, 101, 102, 103, 104, 105]   # packed, in order
    assert _ints(f["caps"][0]) == [15, 15]
    # a larger staging: the stream is waited for BEFORE the pinned buffer is freed
    log = f["second"][0]
    assert log == ["hipStreamSynchronize@1", "hipHostFree", "hipHostMalloc", "hipFree", "hipMalloc", "hipMemcpyAsync@1"]
    assert log.index("hipStreamSynchronize@1") < log.index("hipHostFree")
    assert [float(v) for v in f["second_packed"][0]] == [LV_OK, 6, 1, 9]
    # one that fits: the wait before the overwrite stays
    assert f["third"][0] == ["hipStreamSynchronize@1", "hipMemcpyAsync@1"]
    assert [float(v) for v in f["third_packed"][0]] == [LV_OK, 2, 100, 105]
    assert _ints(f["floor"][0]) == [LV_OK, 1024, 1024]               # 6 floats from a floor of 1024
    assert _ints(f["doubled"][0]) == [LV_OK, 2048, 2048]             # 1200 floats
    m, fr = _ints(f["released"][0])
    assert m == fr == 8


def test_counter_record(emu):
    f = emu("counters")
    assert _ints(f["lazy"][0]) == [0]                                # nothing before the first zero()
    assert f["zero"][0] == ["hipMalloc", "hipHostMalloc", "hipMemcpyAsync@1"]   # zeros from the pinned words
    assert _ints(f["zeroed"][0]) == [LV_OK, 0, 0, 0, 0]
    assert f["read"][0] == ["hipMemcpyAsync@1", "hipStreamSynchronize@1"]
    assert _ints(f["values"][0]) == [LV_OK, 1, 2 ** 64 - 1, 2 ** 40, 12345]   # what sat in the device words, as uint64_t
    assert _ints(f["again"][0]) == [LV_OK, 0, 0]                     # a second zero() allocates nothing
    assert _ints(f["rezeroed"][0]) == [LV_OK, 0, 0, 0, 0]            # ... and clears what the device words held
    m, fr = _ints(f["released"][0])
    assert m == fr == 2
    assert _ints(f["blocks"][0]) == [0, 1, 1, 2, 3]
