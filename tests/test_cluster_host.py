"""The host part of lv_cluster.hpp (the lock-free union-find by minimum id, the ordering key and the size rules: what the kernels
of lv_cluster.hip run) compiled with g++ through tests/emu/hip/hip_runtime.h, whose atomics are sequential, and held to
tests/cluster_ref.py (scipy's connected components put into the canonical order): tests/emu/cluster_emu.cpp links a given edge
list in a given order and prints the canonical labels.  Equality, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import cluster_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cluster_host") / "cluster_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "cluster_emu.cpp"), "-o", str(exe)])

    def run(n, edges, mask=None, min_size=1, max_size=0):
        edges = np.asarray(edges, np.int64).reshape(-1, 2)
        mask = np.ones(n, np.uint8) if mask is None else np.asarray(mask, np.uint8)
        text = f"{n} {min_size} {max_size} {len(edges)}\n" + " ".join(str(int(v)) for v in mask) + "\n" + \
            "\n".join(f"{a} {b}" for a, b in edges) + "\n"
        out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.split()
        C = int(out[0])
        labels = np.array(out[1:1 + n], np.int32)
        sizes = np.array(out[1 + n:1 + n + C], np.uint32)
        rules = np.array(out[1 + n + C:], np.int64).reshape(-1, 3)
        return labels, sizes, C, rules

    return run


def _ref(n, edges, mask=None, min_size=1, max_size=0):
    inc = np.ones(n, bool) if mask is None else np.asarray(mask) != 0
    return cr.canonical(cr.components_of_edges(n, edges, inc), inc, min_size, max_size)[:2]


def _hold(emu, n, edges, **kw):
    labels, sizes, C, _ = emu(n, edges, **kw)
    rl, rs = _ref(n, edges, **kw)
    assert C == len(rs)
    assert np.array_equal(labels, rl)
    assert np.array_equal(sizes, rs)
    return labels, sizes


def test_random_graphs(emu):
    rng = np.random.default_rng(11)
    for n, ne in ((1, 0), (2, 1), (50, 20), (300, 150), (300, 600), (2000, 1500), (2000, 40)):
        for rep in range(3):
            e = rng.integers(0, n, (ne, 2))   # (self loops and repeated edges included)
            mask = (rng.uniform(size=n) < 0.8).astype(np.uint8) if rep == 2 else None
            _hold(emu, n, e, mask=mask)
            _hold(emu, n, e, mask=mask, min_size=3, max_size=40)
            _hold(emu, n, e, mask=mask, min_size=2)


def test_a_path_in_every_edge_order(emu):
    n = 3000
    e = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    rng = np.random.default_rng(5)
    relabel = rng.permutation(n)   # (the path runs through the ids in a shuffled order: the deep-tree case)
    for edges in (e, e[::-1], e[rng.permutation(n - 1)], e[::-1, ::-1], relabel[e], relabel[e][rng.permutation(n - 1)]):
        labels, sizes = _hold(emu, n, edges)
        assert list(sizes) == [n] and np.all(labels == 0)
    # cut in three by excluded nodes
    mask = np.ones(n, np.uint8)
    mask[[1000, 2500]] = 0
    labels, sizes = _hold(emu, n, e[rng.permutation(n - 1)], mask=mask)
    assert list(sizes) == [1499, 1000, 499] and labels[1000] == -1 and labels[0] == 1 and labels[2999] == 2


def test_size_ties_go_to_the_first_member(emu):
    # components {7, 2}, {5, 0}, {1, 3}, {4}, {6}, {8, 9, 10}: by size, ties by the smallest member
    e = [(7, 2), (5, 0), (3, 1), (9, 8), (10, 9)]
    labels, sizes = _hold(emu, 11, e)
    assert list(sizes) == [3, 2, 2, 2, 1, 1]
    assert list(labels) == [1, 2, 3, 2, 4, 1, 5, 3, 0, 0, 0]
    labels, sizes = _hold(emu, 11, e, min_size=2, max_size=2)
    assert list(labels) == [0, 1, 2, 1, -1, 0, -1, 2, -1, -1, -1] and list(sizes) == [2, 2, 2]
    rng = np.random.default_rng(2)
    for _ in range(5):   # many equal sizes, every edge order
        pairs = rng.permutation(400).reshape(-1, 2)
        _hold(emu, 400, pairs[rng.permutation(len(pairs))])


def test_the_removal_rule(emu):
    rules = emu(1, [])[3]
    sizes = [1, 4, 5, 9, 10, 11]
    # debris (min 5): below 5 leaves, max ignored; seeded (5..10): inside the limits and seeded; never without a seed
    assert list(rules[:, 0]) == [int(s < 5) for s in sizes]
    assert list(rules[:, 1]) == [int(5 <= s <= 10) for s in sizes]
    assert list(rules[:, 2]) == [0] * len(sizes)
