"""The *_workspaceSize exports are arithmetic on their arguments and part of the ABI: a caller that sized a workspace with an earlier
library must not find it refused by a later one.  tests/golden/workspace_sizes.json records every one of them on a grid of arguments
(tests/golden/make_golden_workspace_sizes.py, from the library before the workspace layouts were described once); the library has to
return the same numbers.  Likewise FSEHIP_FSE_optimalTableLog, which also has to return -- whatever it returns -- outside its contract.
No GPU is needed."""
import ctypes
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_workspace_sizes as gen  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return ctypes.CDLL(path)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")) as f:
        return json.load(f)


def test_fixture_covers_every_workspace_size_export(recorded):
    header = open(os.path.join(ROOT, "include", "fsehip.h")).read()
    declared = set(re.findall(r"FSEHIP_API size_t FSEHIP_(\w+)_workspaceSize\s*\(", header))
    assert len(declared) >= 18 and declared == set(recorded["workspaceSize"])
    for name, rows in recorded["workspaceSize"].items():
        assert [tuple(a) for a, _ in rows] == list(gen.grid()[name]), name
        if name in gen.BY_BLOCKS or name in gen.BY_BLOCKS_AND_LOG:          # the grid the batch calls are pinned on
            assert sorted(set(a[0] for a, _ in rows)) == [0, 1, 2, 63, 64, 65, 131071, 131072, 131073, 1000000]
        if name in gen.BY_BLOCKS_AND_LOG:
            assert sorted(set(a[1] for a, _ in rows)) == [0, 5, 9, 11, 12, 13]


def test_workspace_sizes_are_the_recorded_ones(lib, recorded):
    for name, rows in recorded["workspaceSize"].items():
        for args, want in rows:
            assert gen.call(lib, name, tuple(args)) == want, (name, args)


def test_spot_values(lib):
    assert gen.call(lib, "FSE_compress_batch", (1, 0)) == 9268
    assert gen.call(lib, "FSE_compress_batch", (200000, 12)) == 1483212800
    assert gen.call(lib, "FSE_decompress_batch", (7, 0)) == 93132
    assert gen.call(lib, "HUF_compress_batch", (1,)) == 270364
    assert gen.call(lib, "HUF_decompress_batch", (3,)) == 26780
    assert gen.call(lib, "FSE_compressU16_batch", (2,)) == 39440


def test_optimal_table_log(lib, recorded):
    assert len(recorded["optimalTableLog"]) == len(gen.OTL_GRID)
    for (tl, n, msv), want in recorded["optimalTableLog"]:
        assert n > 1 and msv >= 1
        assert gen.optimal_table_log(lib, tl, n, msv) == want, (tl, n, msv)
    # outside the contract (the reference takes the highest bit of 0 there): the call returns, with a table log the library can build
    for tl in (0, 5, 12, 13):
        for n, msv in ((0, 255), (1, 255), (0, 0), (1, 0), (2, 0), (1000, 0)):
            assert 5 <= gen.optimal_table_log(lib, tl, n, msv) <= 12, (tl, n, msv)
