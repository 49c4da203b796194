"""One context crosses every floor at which the map, scan and cloud stores grow (limo-velo_amd/csrc/lv_stores.hpp), at the smallest
sizes that cross them; the steps are those of tests/golden/make_golden_growth.py.  After every step the map equals a model kept
beside it — the oracle's sequential box rule for the adds, as in tests/test_gpu_map_add.py, and a numpy mask for the evicted box —
and map_knn of 256 queries equals brute force over the fetched points: the growths keep the points, the box chains and the
back-positions that the later down-sampling adds and evictions walk.  At the end the statistics (`bytes` included) and the SHA-256
digests of map_fetch, scan_fetch and cloud_fetch (and of every scan and of the reallocated LiDAR buffer on the way) equal what the library gave BEFORE the stores' memory moved into DevBuf / PinBuf
(tests/golden/store_growth.npz, recorded on an MI355X from that commit)."""
import os
import sys

import numpy as np
import pytest

from test_gpu_map_query import _assert_knn_equal, np_knn

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_growth as mg  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_every_growth_keeps_the_map_and_ends_at_the_parents_record(lv, oracle):
    from limo_velo_amd import capi

    g = np.load(os.path.join(HERE, "golden", "store_growth.npz"))
    rng = np.random.default_rng(3)
    ref = np.zeros((0, 3), np.float32)
    marks = {}
    with capi.Context() as ctx:
        for name, ev in mg.steps(ctx, capi, marks):
            if ev is not None and ev[0] == "build":
                ref = ev[1]
            elif ev is not None and ev[0] == "add":
                ref = oracle.map_add(ref, ev[1], downsample=True) if ev[2] else np.concatenate([ref, ev[1]])
            elif ev is not None and ev[0] == "evict":
                gone = np.all((ref >= ev[1]) & (ref <= ev[2]), axis=1)
                assert gone.any(), name
                ref = ref[~gone]
            got = ctx.map_fetch()
            assert got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref)), name
            q = (got[rng.integers(0, len(got), 256)] + rng.normal(0, 0.2, (256, 3))).astype(np.float32)
            _assert_knn_equal(ctx.map_knn(q, 5), np_knn(got, q, 5))
        names, stats, digests, sizes = mg.record(ctx, marks)
    assert names == list(g["stat_names"])
    assert dict(zip(names, stats.tolist())) == dict(zip(names, g["stats"].tolist()))
    want = dict(zip(g["digest_names"].tolist(), zip(g["sizes"].tolist(), g["digests"].tolist())))
    assert {k: (sizes[k], digests[k]) for k in digests} == want
