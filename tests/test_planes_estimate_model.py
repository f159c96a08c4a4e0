"""Plane estimates without a device (include/fsehip.h, "plane estimates"): the properties of the integer cost model of
planes_estimate_corpus.py -- L against log2, the cost of constant and flat planes, bits256 against the float entropy, the choice rule on
hand-made estimates -- the four rows of the header's table reproduced on their corpora, then the library's two exports, the workspace
bound answered by host arithmetic, every argument refusal decided before any device call with nothing written, and the Python surface."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

import planes_estimate_corpus as pe
from planes_estimate_corpus import PLAIN, PRED, SUB, XOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
SZ, VP, U64, UI = C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint
EXPORTS = ("FSEHIP_planes_estimate_workspaceBound", "FSEHIP_planes_estimate_dbatch")


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    return C.CDLL(path)


# ---------------------------------------------------------------------------------------------------------------- the model
def test_the_table_and_L():
    assert len(pe.T) == 256 and pe.T[0] == 0 and pe.T[255] == 255 and all(a <= b for a, b in zip(pe.T, pe.T[1:]))
    prev = 0
    for x in range(1, (1 << 16) + 1):
        v = pe.L(x)
        assert v >= prev, x
        prev = v
    for k in range(41):
        assert pe.L(1 << k) == 256 * k, k
    worst = max(abs(pe.L(x) / 256 - math.log2(x)) for x in list(range(1, 70000)) + [(1 << 32) - 1, (1 << 33) + 12345, (1 << 31) + 7, (1 << 40) - 1, (1 << 40) + 1])
    print("max |L(x) / 256 - log2 x| = %.3f / 256" % (worst * 256))
    assert worst < 1.95 / 256


def test_constant_and_flat_planes():
    for v, n in ((0, 1), (0, 5000), (255, 77), (9, 1 << 20)):
        plane = np.full(n, v, np.uint8)
        assert pe.plane_bits(plane) == 0 and pe.est_bytes([plane]) == 0
    assert pe.plane_bits(np.zeros(0, np.uint8)) == 0 and pe.est_bytes([np.zeros(0, np.uint8)]) == 0
    flat = np.tile(np.arange(256, dtype=np.uint8), 64)
    assert pe.plane_bits(flat) == 8 * 256 * len(flat) and pe.est_bytes([flat]) == len(flat), "eight bits a byte, exactly"
    assert pe.est_bytes([flat, np.full(10, 3, np.uint8), flat]) == 2 * len(flat), "the sum over the planes"


def test_bits256_against_the_float_entropy():
    rng = np.random.default_rng(8)
    n = 50000
    planes = {"random": rng.integers(0, 256, n, dtype=np.uint8),
              "skewed": np.minimum(rng.geometric(0.3, n) - 1, 255).astype(np.uint8),
              "two symbols": np.where(rng.random(n) < 0.03, 200, 7).astype(np.uint8)}
    for name, plane in planes.items():
        got, want = pe.plane_bits(plane) / 256, pe.float_entropy_bits(plane)
        print("%-12s bits256 / 256 = %.1f, float entropy %.1f bits, difference %.1f (allowed %.1f)" % (name, got, want, got - want, 2.5 * n / 256))
        assert abs(got - want) <= 2.5 * n / 256, name
    assert 0.99 * n < pe.est_bytes([planes["random"]]) <= n, "a finite sample of random bytes: just below eight bits a byte, never above the raw block"


def test_the_choice_rule():
    ALL, NOPLAIN = 15, 14
    assert pe.choose([100, 100, 100, 100], ALL, 0) == PLAIN, "ties stay with the lowest id"
    assert pe.choose([100, 99, 99, 98], ALL, 0) == SUB and pe.choose([100, 99, 99, 99], ALL, 0) == PRED, "margin 0: strictly smaller wins, ties do not"
    assert pe.choose([1000, 951, 0, 0], 3, 50) == PLAIN and pe.choose([1000, 950, 0, 0], 3, 50) == PLAIN and pe.choose([1000, 949, 0, 0], 3, 50) == PRED
    assert pe.choose([1000, 949, 903, 902], ALL, 50) == PRED, "the margin is taken against the current best: 903 and 902 are not 5 % below 949"
    assert pe.choose([1000, 949, 901, 855], ALL, 50) == SUB and pe.choose([1000, 949, 901, 856], ALL, 50) == XOR
    assert pe.choose([1000, 0, 0, 0], ALL, 1000) == PLAIN and pe.choose([0, 0, 0, 0], ALL, 1000) == PLAIN, "margin 1000: nothing is below zero"
    assert pe.choose([1, 500, 400, 300], NOPLAIN, 50) == SUB and pe.choose([1, 500, 490, 480], NOPLAIN, 50) == PRED, "without PLAIN the lowest requested id starts"
    assert pe.choose([5, 5, 5, 1], 1 << XOR, 0) == XOR and pe.choose([0, 0, 0, 0], 1 << SUB, 50) == SUB
    assert pe.choose([pe.ONES, 10, pe.ONES, 9], (1 << PRED) | (1 << SUB), 0) == SUB, "slots outside the mask are not looked at"


def _row(t, b, E, cands):
    return [pe.est_bytes(pe.candidate_planes(t, b, E, c)) for c in cands]


def test_the_table_of_the_header_reproduces():
    g = pe.bf16_gaussian()
    assert len(g) == 256 << 10 and _row(g, None, 2, (PLAIN, PRED)) == [174431, 183556]
    s = pe.sorted_int64()
    assert len(s) == 256 << 10 and _row(s, None, 8, (PLAIN, PRED)) == [163731, 108410]
    p = pe.position_ids()
    assert len(p) == 128 << 10 and _row(p, None, 4, (PLAIN, PRED)) == [49152, 108]
    t, b = pe.update_pair()
    assert len(t) == len(b) == 256 << 10 and _row(t, b, 2, (PLAIN, PRED, XOR, SUB)) == [174431, 183556, 33297, 28881]
    # ... and what the model of the whole call makes of them
    bits, est, choice, res = pe.estimate_model([t, g], 2, 15, [b, g], 50)
    assert est == [174431, 183556, 33297, 28881, 174431, 183556, 0, 0] and choice == [SUB, XOR] and res == [len(t), len(g)]
    assert bits[4 * 2:] == [pe.plane_bits(g[0::2]), pe.plane_bits(g[1::2])] + bits[10:12] + [0] * 4
    _, est, choice, _ = pe.estimate_model([g, np.zeros(0, np.uint8), g[:1]], 2, 3, None, 50)
    assert est == [174431, 183556, pe.ONES, pe.ONES, 0, 0, pe.ONES, pe.ONES, 0, 0, pe.ONES, pe.ONES] and choice == [PLAIN, PLAIN, PLAIN]
    _, est, choice, res = pe.estimate_model([g[:10], g[:10], g[:10]], 2, 2, None, 0, capacity=25, offsets=[0, 10, 5, 30])
    assert res == [10, pe.GENERIC, pe.GENERIC] and choice == [PRED, pe.NO_CHOICE, pe.NO_CHOICE] and est[4:] == [pe.ONES] * 8


# ---------------------------------------------------------------------------------------------------------------- the library
def test_exports_bound_and_bad_arguments_without_a_device(lib):
    for name in EXPORTS:
        getattr(lib, name)
    bound = lib.FSEHIP_planes_estimate_workspaceBound
    bound.restype = SZ
    for E in (1, 2, 4, 8):
        for mask in range(1, 16):
            got = [bound(SZ(n), UI(E), UI(mask)) for n in (0, 1, 2, 3, 100, 4096, (1 << 24) - 1)]
            assert all(b % 256 == 0 and b < (1 << 62) for b in got) and all(a <= b for a, b in zip(got, got[1:])), (E, mask)
            assert got[0] == 0 and got[2] > got[1] >= bin(mask).count("1") * E * 1024, "a histogram of 256 words per requested candidate and plane"
        assert bound(SZ(5), UI(E), UI(3)) < bound(SZ(5), UI(E), UI(15)), "candidates that are not requested take no room"
    for n, E, mask in ((1, 2, 0), (1, 2, 16), (1, 2, 0x80000001), (1, 3, 1), (1, 0, 1), (1, 16, 1), (1 << 24, 2, 1), (1 << 40, 1, 1)):
        assert bound(SZ(n), UI(E), UI(mask)) > (1 << 62), (n, E, mask)

    a = (C.c_uint64 * 16)()
    room = (C.c_uint8 * (40 << 10))()
    p, null = C.cast(a, VP), VP(0)
    ws = VP((C.addressof(room) + 255) & ~255)
    big = SZ(33 << 10)

    def est(ptrs=None, base=p, n=1, E=2, cap=8, mask=15, margin=50, w=ws, wb=big):     # ptrs: plane bits, estimates, choice, results, src, offsets
        q = list(ptrs or [p] * 6)
        return lib.FSEHIP_planes_estimate_dbatch(q[0], q[1], q[2], q[3], q[4], base, q[5], SZ(n), UI(E), U64(cap), UI(mask), UI(margin), w, wb, null)

    for k in range(6):
        q = [p] * 6
        q[k] = null
        assert est(q) == HIP_INVALID_VALUE, k
    for mask in (0, 16, 31, 0x100, 0xFFFFFFFF):
        assert est(mask=mask) == HIP_INVALID_VALUE, mask
    for mask in (4, 8, 12, 5, 15):
        assert est(mask=mask, base=null) == HIP_INVALID_VALUE, "XOR or SUB without a base"
    for E in (0, 3, 5, 16, 0xFFFFFFFF):
        assert est(E=E) == HIP_INVALID_VALUE, E
    assert est(margin=1001) == HIP_INVALID_VALUE and est(margin=0xFFFFFFFF) == HIP_INVALID_VALUE
    assert est(n=1 << 24) == HIP_INVALID_VALUE and est(cap=1 << 46) == HIP_INVALID_VALUE and est(cap=32768 << 24) == HIP_INVALID_VALUE
    assert est(w=null) == HIP_INVALID_VALUE and est(w=null, wb=SZ(0)) == HIP_INVALID_VALUE and est(w=VP(ws.value + 16)) == HIP_INVALID_VALUE
    for E in (1, 2, 4, 8):
        for mask in (1, 3, 15):
            assert est(E=E, mask=mask, wb=SZ(bound(SZ(1), UI(E), UI(mask)) - 1)) == HIP_INVALID_VALUE, (E, mask)
    assert est(n=0, mask=3, base=null, w=null, wb=SZ(0)) == 0, "no tensors: legal, nothing to launch and no workspace to have"
    assert all(x == 0 for x in a) and not any(room), "nothing is written"


def test_python_surface():
    import finitestateentropy_amd
    from finitestateentropy_amd import api
    for name in ("estimate_tensors", "compress_tensors_auto", "TensorBundle"):
        assert name in finitestateentropy_amd.__all__ and getattr(finitestateentropy_amd, name) is getattr(api, name), name
    assert list(inspect.signature(api.estimate_tensors).parameters) == ["tensors", "base", "candidates", "margin_permille"]
    assert list(inspect.signature(api.compress_tensors_auto).parameters) == ["tensors", "base", "codec", "block_size_id", "segment_log", "margin_permille"]
    assert list(inspect.signature(api.decompress_tensors).parameters) == ["obj", "base"], "unchanged"
    assert inspect.signature(api.estimate_tensors).parameters["margin_permille"].default == 50
    assert inspect.signature(api.compress_tensors_auto).parameters["margin_permille"].default == 50
    for name in ("planes_estimate_workspace_bound", "planes_estimate_dbatch", "estimate_tensors", "compress_tensors_auto"):
        assert callable(getattr(api.FseHip, name)), name
    par = inspect.signature(api.FseHip.planes_estimate_dbatch).parameters
    assert all(par[k].default is None for k in ("base", "capacity", "plane_bits", "est_bytes", "choice", "results", "workspace"))
    hip = api.FseHip.__new__(api.FseHip)                          # (no launch below: nothing here has a device)
    hip.lib = C.CDLL(os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so"))
    assert hip.planes_estimate_workspace_bound(3, 2, 3) == 3 * 2 * 2 * 1024
    with pytest.raises(ValueError):
        hip.planes_estimate_workspace_bound(3, 2, 0)
    assert hip.estimate_tensors([]) == []
    bundle = hip.compress_tensors_auto([])
    assert isinstance(bundle, api.TensorBundle) and bundle.parts == {} and bundle.index == {} and bundle.estimates == [] and bundle.nbytes == 0
    assert hip.decompress_tensors(bundle) == []
    # every refusal in front of the first launch (there is no device here to launch on)
    with pytest.raises(TypeError):
        hip.estimate_tensors([np.zeros(4)])
    with pytest.raises(TypeError):
        hip.compress_tensors_auto([np.zeros(4)])
    for bad in (("plain", "delta"), (), ("xor",), ("plain", "sub"), "plain"):
        with pytest.raises(ValueError):
            hip.estimate_tensors([], candidates=bad)                # an unknown name, none at all, a delta without a base, a bare string
    for bad in (-1, 1001, 2.5, True, None):
        with pytest.raises(ValueError):
            hip.estimate_tensors([], margin_permille=bad)
        with pytest.raises(ValueError):
            hip.compress_tensors_auto([], margin_permille=bad)
    with pytest.raises(ValueError):
        hip.estimate_tensors([], base=[1])
    delta = api.TensorBundle({"sub": api.CompressedTensors([], [], [], None, 0, 5, True)}, {"sub": [0]}, [dict(bytes=0, estimates={}, choice="sub")], 1)
    with pytest.raises(ValueError):
        hip.decompress_tensors(delta)
