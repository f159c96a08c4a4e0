"""Tensor digests and the gate without a device (include/fsehip.h, "tensor digests and checked deltas"): the numpy model of
planes_digest_corpus.py -- its XXH32 against the oracle's, the vectorised tile digests against the definition lane by lane, a digest that does
not depend on where the bytes lie, constructed pairs that must differ, the gate on integers -- then the library's three exports, every argument
refusal decided before any device call with nothing written, and the Python surface (DeltaBase(check=...), base_digests, tensor_digests)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import planes_digest_corpus as dg
from planes_digest_corpus import CORRUPT, GENERIC, T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
SZ, VP, U64, UI = C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint
EXPORTS = ("FSEHIP_tensor_digest_workspaceBound", "FSEHIP_tensor_digest_dbatch", "FSEHIP_tensor_gate_dbatch")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return C.CDLL(path)


# ---------------------------------------------------------------------------------------------------------------- 1
def test_model_xxh32_is_the_oracles(restatement):
    rng = np.random.default_rng(5)
    for n in list(range(41)) + [255, 256, 257, 512]:
        data = rng.integers(0, 256, n, dtype=np.uint8)
        for seed in (dg.S0, dg.S1):
            assert dg.xxh32(data, seed) == restatement.xxh32(data, seed), (n, seed)
    rows = rng.integers(0, 256, (7, 37), dtype=np.uint8)
    assert [int(x) for x in dg.xxh32_rows(rows, dg.S1)] == [restatement.xxh32(r, dg.S1) for r in rows]


def test_vectorised_tiles_are_the_definition():
    rng = np.random.default_rng(6)
    data = rng.integers(0, 256, 2 * T + 1024 + 3, dtype=np.uint8)
    got = dg.tile_digests(data)
    assert [tuple(int(x) for x in r) for r in got] == [dg.tile_digest(data[k:k + T]) for k in range(0, len(data), T)]
    # a lane's stream: 512 bytes in a full tile; in a partial one the last piece alone may be short, and lanes behind it are empty
    assert {len(s) for s in dg.lane_streams(data[:T])} == {512}
    lens = [len(s) for s in dg.lane_streams(data[:1024 + 16 + 3])]
    assert lens == [32, 19] + [16] * 62 and [len(s) for s in dg.lane_streams(data[:20])] == [16, 4] + [0] * 62
    assert dg.tensor_digest(data[:0]) == dg.xxh32(np.zeros(8, np.uint8), dg.S0) | (dg.xxh32(np.zeros(8, np.uint8), dg.S1) << 32)


def test_digest_does_not_depend_on_the_offset():
    rng = np.random.default_rng(7)
    data = rng.integers(0, 256, T + 1024 + 5, dtype=np.uint8)
    seen = set()
    for shift in range(16):
        big = rng.integers(0, 256, len(data) + 64, dtype=np.uint8)
        big[shift:shift + len(data)] = data
        digs, res = dg.digest_batch(big, [0, shift, shift + len(data), len(big)])
        assert res == [shift, len(data), len(big) - shift - len(data)]
        seen.add(digs[1])
    assert len(seen) == 1


def test_constructed_pairs_differ():
    rng = np.random.default_rng(8)
    for n in (0, 1, 15, 16, 17, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        assert dg.tensor_digest(np.zeros(n, np.uint8)) != dg.tensor_digest(np.zeros(n + 1, np.uint8)), n
    data = rng.integers(0, 256, 2 * T + 1024 + 3, dtype=np.uint8)
    d0 = dg.tensor_digest(data)

    def changed(f):
        x = data.copy()
        f(x)
        return dg.tensor_digest(x)
    last_piece_of_lane_5 = 31 * 1024 + 5 * 16                                   # (in tile 0)
    flips = {"first byte": 0, "last byte": len(data) - 1, "a lane's last piece": last_piece_of_lane_5 + 15, "tile 1": T + 77}
    seen = {d0}
    for name, at in flips.items():
        for bit in (0, 7):
            d = changed(lambda x: x.__setitem__(at, x[at] ^ (1 << bit)))
            assert d not in seen, (name, bit)
            seen.add(d)

    def swap(x, a, b, n):
        t = x[a:a + n].copy()
        x[a:a + n] = x[b:b + n]
        x[b:b + n] = t
    assert changed(lambda x: swap(x, 16 * 3, 16 * 4, 16)) not in seen            # two pieces of neighbouring lanes
    assert changed(lambda x: swap(x, 16 * 3, 1024 + 16 * 9, 16)) not in seen     # ... of different lanes and rounds
    assert changed(lambda x: swap(x, 16 * 3, 1024 + 16 * 3, 16)) not in seen     # ... of one lane: the order inside a stream counts too
    assert changed(lambda x: swap(x, 0, T, T)) not in seen                       # two whole tiles


# ---------------------------------------------------------------------------------------------------------------- 2
def test_gate_model():
    cases = dg.gate_cases()
    assert {c[2] for c in cases} == {1, 2, 4} and any(c[6] is not None for c in cases)
    for name, F, E, got, res, want, first in cases:
        G, R = dg.gate(F, E, got, res, want, first)
        nT, nF = len(want), len(F) - 1
        assert len(G) == nF + 1 and G[nF] == F[nF] and all(a <= b for a, b in zip(G, G[1:])), name
        own = [min(f, nF) for f in first[::E]] if first is not None else [i * E for i in range(nT + 1)]
        for i in range(nT):
            ok = res[i] >= 0 and got[i] == want[i]
            frames = range(own[i], own[i + 1])
            if ok:
                assert R[i] == res[i] and all(G[q] == F[q] for q in frames), (name, i)
            else:
                assert R[i] == (res[i] if res[i] < 0 else CORRUPT), (name, i)
                assert all(G[q] == F[own[i + 1]] for q in frames), (name, i)
                assert all(G[q + 1] - G[q] == 0 for q in frames if q + 1 < own[i + 1]), "empty extents"
    name, F, E, got, res, want, first = next(c for c in cases if c[0] == "error and mismatch E=2")
    G, R = dg.gate(F, E, got, res, want, first)
    assert R[1] == GENERIC and R[2] == CORRUPT and R[0] == res[0] and G[2:4] == [F[4]] * 2 and G[4:6] == [F[6]] * 2 and G[:2] == F[:2]


# ---------------------------------------------------------------------------------------------------------------- 3
def test_exports_and_bad_arguments_without_a_device(lib):
    for name in EXPORTS:
        getattr(lib, name)
    bound = lib.FSEHIP_tensor_digest_workspaceBound
    bound.restype = SZ
    a = (C.c_uint64 * 8)()
    room = (C.c_uint8 * 1024)()
    p, null = C.cast(a, VP), VP(0)
    ws = VP((C.addressof(room) + 255) & ~255)
    big = SZ(1 << 40)

    b0, b1, b2 = (bound(U64(c), SZ(n)) for c, n in ((0, 0), (1 << 20, 4), (1 << 30, 4096)))
    assert 0 <= b0 <= b1 < b2 < (1 << 30) and b0 % 256 == b1 % 256 == b2 % 256 == 0
    assert b2 >= 8 * ((1 << 30) // T + 2 * 4096), "eight bytes per work item and per tensor"
    for c, n in ((1 << 46, 1), (T << 24, 1), (8, 1 << 31), (8, 1 << 24)):
        assert bound(U64(c), SZ(n)) > (1 << 62), (c, n)

    def digest(ptrs=None, n=1, cap=8, w=ws, wb=big):             # ptrs: digests, results, src, offsets
        q = list(ptrs or [p] * 4)
        return lib.FSEHIP_tensor_digest_dbatch(q[0], q[1], q[2], q[3], SZ(n), U64(cap), w, wb, null)

    def gate(ptrs=None, nf=2, first=null, E=2, n=1):              # ptrs: gated offsets, gate results, frame offsets, digests, digest results, expected
        q = list(ptrs or [p] * 6)
        return lib.FSEHIP_tensor_gate_dbatch(q[0], q[1], q[2], SZ(nf), first, UI(E), q[3], q[4], q[5], SZ(n), null)

    for k in range(4):
        q = [p] * 4
        q[k] = null
        assert digest(q) == HIP_INVALID_VALUE, k
    assert digest(n=1 << 31) == HIP_INVALID_VALUE and digest(cap=1 << 46) == HIP_INVALID_VALUE and digest(cap=T << 24) == HIP_INVALID_VALUE
    assert digest(w=null, wb=SZ(0)) == HIP_INVALID_VALUE and digest(w=null) == HIP_INVALID_VALUE
    assert digest(w=VP(ws.value + 8)) == HIP_INVALID_VALUE
    assert digest(wb=SZ(bound(U64(8), SZ(1)) - 1)) == HIP_INVALID_VALUE
    for k in range(6):
        q = [p] * 6
        q[k] = null
        assert gate(q) == HIP_INVALID_VALUE, k
    for E in (0, 3, 5, 16, 0xFFFFFFFF):
        assert gate(E=E) == HIP_INVALID_VALUE and gate(E=E, first=p) == HIP_INVALID_VALUE, E
    for E in (1, 2, 4, 8):
        assert gate(E=E, nf=E + 1) == HIP_INVALID_VALUE and gate(E=E, nf=E - 1) == HIP_INVALID_VALUE, "nFrames != nTensors * E without d_frameFirst"
        assert gate(E=E, nf=E, n=(1 << 31) // E) == HIP_INVALID_VALUE and gate(E=E, n=(1 << 31) // E, first=p) == HIP_INVALID_VALUE
    assert gate(n=1 << 31, nf=1 << 32) == HIP_INVALID_VALUE and gate(nf=1 << 31, first=p) == HIP_INVALID_VALUE
    assert all(x == 0 for x in a) and not any(room), "nothing is written"


# ---------------------------------------------------------------------------------------------------------------- 4
def test_python_surface():
    import finitestateentropy_amd
    from finitestateentropy_amd import api
    assert finitestateentropy_amd.DeltaBase is api.DeltaBase and finitestateentropy_amd.tensor_digests is api.tensor_digests
    assert {"DeltaBase", "SparsePlanes", "tensor_digests"} <= set(finitestateentropy_amd.__all__)
    plain, checked = api.DeltaBase([1, 2], "xor"), api.DeltaBase([1, 2, 3], check=True)
    assert plain.check is False and checked.check is True and (checked.op, len(checked)) == ("sub", 3)
    assert repr(plain) == "DeltaBase(2 tensors, op='xor')" and repr(api.DeltaBase([])) == "DeltaBase(0 tensors, op='sub')", "unchanged without check"
    assert repr(checked) == "DeltaBase(3 tensors, op='sub', check=True)"
    assert list(inspect.signature(api.DeltaBase.__init__).parameters) == ["self", "tensors", "op", "check"]
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError):
            api.DeltaBase([], "sub", bad)
    # the object: a class-level default, set on the instance only where used
    assert api.CompressedTensors.base_digests is None
    obj = api.CompressedTensors([], [], [], None, 0, 5)
    assert obj.base_digests is None and "base_digests" not in vars(obj)
    hip = api.FseHip.__new__(api.FseHip)                          # (no launch below: nothing here has a device)
    for seg in (False, True):
        call = hip.compress_tensors_segmented if seg else hip.compress_tensors
        unchecked = call([], base=api.DeltaBase([], "sub"))
        assert unchecked.base_digests is None and "base_digests" not in vars(unchecked) and unchecked.delta
        for codec in (0, api.SparsePlanes(1)):
            got = call([], codec=codec, base=api.DeltaBase([], "sub", check=True))
            assert got.base_digests == [] and vars(got)["base_digests"] == [] and got.delta and got.delta_op == "sub"
            assert hip.decompress_tensors(got, api.DeltaBase([], "sub")) == []
    # the pinned signatures
    assert list(inspect.signature(api.compress_tensors).parameters) == ["tensors", "codec", "block_size_id", "base"]
    assert list(inspect.signature(api.compress_tensors_segmented).parameters) == ["tensors", "segment_log", "codec", "block_size_id", "base"]
    assert list(inspect.signature(api.decompress_tensors).parameters) == ["obj", "base"]
    assert list(inspect.signature(api.decompress_tensor_windows).parameters) == ["obj", "windows", "base"]
    assert list(inspect.signature(api.patch_tensor_windows).parameters) == ["obj", "tensors", "windows", "base"]
    assert list(inspect.signature(api.tensor_digests).parameters) == ["tensors"]
    # the low-level methods mirror the three C calls
    for name in ("tensor_digest_workspace_bound", "tensor_digest_dbatch", "tensor_gate_dbatch", "tensor_digests"):
        assert callable(getattr(api.FseHip, name)), name
    par = inspect.signature(api.FseHip.tensor_digest_dbatch).parameters
    assert all(par[k].default is None for k in ("capacity", "digests", "results", "workspace"))
    par = inspect.signature(api.FseHip.tensor_gate_dbatch).parameters
    assert all(par[k].default is None for k in ("frame_first", "n_frames", "gated_offsets", "results"))
    assert "not check" in api.FseHip.decompress_tensor_windows.__doc__.replace("NOT", "not")
    assert hip.tensor_digests([]) == []
    with pytest.raises(TypeError):
        hip.tensor_digests([np.zeros(4)])
