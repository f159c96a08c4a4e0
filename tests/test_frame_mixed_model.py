"""The packed frame writer with a codec per frame, without a device (include/fsehip.h, FSEHIP_frame_compress_packed_mixed_dbatch): the exports
exist and refuse bad arguments before any device call; FSEHIP_frame_mixedWorkspaceBound keeps its stated bounds, is monotone and equals the
values recorded here; the reason for the feature, from the oracle's frames alone -- on a bf16 weight update the two planes of the delta want
different codecs; the corpus's expected choices hold both codecs; and the Python surface."""
import ctypes as C
import inspect
import os

import pytest

import frame_mixed_corpus as fmc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID_VALUE = 1
GIVEN, CHOOSE = 0, 1
SZ, VP, U64 = C.c_size_t, C.c_void_p, C.c_uint64
EXPORTS = ("FSEHIP_frame_mixedWorkspaceBound", "FSEHIP_frame_compress_packed_mixed_dbatch", "FSEHIP_tensor_compress_mixed_dbatch")
# FSEHIP_frame_mixedWorkspaceBound(nFrames, maxTotalBlocks, blockSizeId, policy): this function's pin (it is no *_workspaceSize: the fixture of
# test_workspace_sizes.py does not hold it)
PINNED = {
    (0, 0, 0, GIVEN): 271872, (0, 0, 0, CHOOSE): 272128,
    (1, 1, 0, GIVEN): 275200, (1, 1, 0, CHOOSE): 276736,
    (13, 40, 0, GIVEN): 578304, (13, 40, 0, CHOOSE): 640512,
    (2048, 2048, 5, GIVEN): 83651840, (2048, 2048, 5, CHOOSE): 152350208,
    (1000, 200000, 6, GIVEN): 14271964672, (1000, 200000, 6, CHOOSE): 27585564928,
}


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    if not os.path.exists(path):
        import finitestateentropy_amd
        finitestateentropy_amd.build_library()
    L = C.CDLL(path)
    for name in ("FSEHIP_frame_mixedWorkspaceBound", "FSEHIP_frame_compress_packed_dbatch_workspaceSize"):
        getattr(L, name).restype = SZ
    return L


def _up256(x):
    return (x + 255) & ~255


# ---------------------------------------------------------------------------------------------------------------- 1
def test_exports_and_bad_arguments_without_a_device(lib):
    for name in EXPORTS:
        getattr(lib, name)
    a = (C.c_uint64 * 8)()
    p = C.cast(a, VP)
    null = VP(0)
    room = (C.c_uint8 * 512)()
    ws = VP((C.addressof(room) + 255) & ~255)                # a workspace on its 256-byte alignment, "large enough": only what is named refuses the call
    big = 1 << 40
    fm, tm = lib.FSEHIP_frame_compress_packed_mixed_dbatch, lib.FSEHIP_tensor_compress_mixed_dbatch

    def frame(policy=GIVEN, tol=0, bsid=0, align=0, codecs=p, ws=ws, ws_bytes=big, n=1, nblk=4):
        return fm(p, U64(64), p, p, p, p, SZ(n), SZ(nblk), C.c_uint(bsid), codecs, C.c_int(policy), C.c_uint(tol), C.c_uint(align), ws, SZ(ws_bytes), null)

    def tensor(E=2, policy=GIVEN, tol=0, bsid=0, align=0, codecs=p, src=p, base=p, planes=p, ws=ws, ws_bytes=big, n=1, nblk=4):
        return tm(p, U64(64), p, p, p, src, base, p, SZ(n), C.c_uint(E), U64(8), SZ(nblk), C.c_uint(bsid), codecs, C.c_int(policy), C.c_uint(tol), C.c_uint(align),
                  planes, p, ws, SZ(ws_bytes), null)

    for call in (frame, tensor):
        for bad in (dict(policy=2), dict(policy=-1), dict(policy=CHOOSE, tol=1001), dict(policy=CHOOSE, tol=0xFFFFFFFF), dict(bsid=7), dict(bsid=255), dict(align=13),
                    dict(align=0xFFFFFFFF), dict(codecs=null), dict(policy=CHOOSE, codecs=null), dict(ws=VP(ws.value + 8)), dict(ws_bytes=0), dict(policy=CHOOSE, ws_bytes=0),
                    dict(nblk=1 << 31)):
            assert call(**bad) == HIP_INVALID_VALUE, (call.__name__, bad)
        for policy in (GIVEN, CHOOSE):                       # one byte short of the bound
            need = int(lib.FSEHIP_frame_mixedWorkspaceBound(SZ(2 if call is tensor else 1), SZ(4), C.c_uint(0), C.c_int(policy)))
            assert call(policy=policy, ws_bytes=need - 1) == HIP_INVALID_VALUE, (call.__name__, policy)
    assert frame(n=1 << 31) == HIP_INVALID_VALUE
    for E in (1, 2, 8):
        assert tensor(E=E, n=(1 << 31) // E) == HIP_INVALID_VALUE
    # the composite's own: element sizes, a null source, a null planes buffer (plain form: E > 1 only; delta form: E == 1 too)
    for E in (0, 3, 5, 16, 0xFFFFFFFF):
        assert tensor(E=E) == HIP_INVALID_VALUE, E
    for E in (1, 2, 4, 8):
        assert tensor(E=E, src=null) == HIP_INVALID_VALUE, E
        assert tensor(E=E, planes=null) == HIP_INVALID_VALUE, E
        if E > 1:
            assert tensor(E=E, base=null, planes=null) == HIP_INVALID_VALUE, E
    assert all(x == 0 for x in a) and not any(room)


# ---------------------------------------------------------------------------------------------------------------- 2
def test_workspace_bound(lib):
    W, P = lib.FSEHIP_frame_mixedWorkspaceBound, lib.FSEHIP_frame_compress_packed_dbatch_workspaceSize

    def w(nf, nb, bsid, policy):
        return int(W(SZ(nf), SZ(nb), C.c_uint(bsid), C.c_int(policy)))
    err = (1 << 64) - 1                                      # GENERIC
    for bad in ((1, 1, 7, GIVEN), (1, 1, 255, CHOOSE), (1, 1, 0, 2), (1, 1, 0, -1)):
        assert w(*bad) == err, bad
    for bsid in range(7):
        slot = (512 + (1024 << bsid) + ((1024 << bsid) >> 7) + 4 + 8 + 15) & ~15         # FSE_compressBound(block size), rounded up to 16
        prev = None
        for nf, nb in ((0, 0), (1, 0), (1, 1), (13, 40), (2048, 2048), (2049, 5000), (1000, 200000), (200000, 400000)):
            p0, p1 = (int(P(SZ(nf), SZ(nb), C.c_uint(bsid), C.c_int(c))) for c in (0, 1))
            g, c = w(nf, nb, bsid, GIVEN), w(nf, nb, bsid, CHOOSE)
            # the closed forms the header states
            assert g == max(p0, p1) + 3 * _up256(8 * nb), (bsid, nf, nb)
            assert c == max(p0, p1) + _up256(8 * nb) + _up256(8 * (nb + 1)) + _up256(nb * slot), (bsid, nf, nb)
            assert c <= p0 + p1 + 3 * _up256(8 * (nb + 1)), (bsid, nf, nb)
            if prev is not None:
                assert g >= prev[0] and c >= prev[1]        # monotone along a chain that grows in both counts
            prev = (g, c)
    for nf in (0, 1, 5, 1024, 1025, 70000):                  # monotone in each count alone
        for nb in (0, 1, 31, 32, 1000, 131072, 131073):
            for policy in (GIVEN, CHOOSE):
                assert w(nf + 1, nb, 0, policy) >= w(nf, nb, 0, policy) and w(nf, nb + 1, 0, policy) >= w(nf, nb, 0, policy), (nf, nb, policy)
    got = {k: w(*k) for k in PINNED}
    print("FSEHIP_frame_mixedWorkspaceBound:", got)
    assert got == PINNED


# ---------------------------------------------------------------------------------------------------------------- 3
def test_the_planes_of_a_weight_update_want_different_codecs(checker):
    sizes = {}
    for name, data in fmc.update_planes():
        sizes[name] = tuple(int(checker.frame_compress(data, 5, codec)[0]) for codec in (0, 1))
        F, H = sizes[name]
        print("%-13s %7d bytes: FSE frame %7d, Huff0 frame %7d (Huff0 over FSE %+.2f %%)" % (name, data.size, F, H, 100.0 * (H - F) / F))
    choice = lambda name, tol: fmc.expected_choice(*sizes[name], tol)[0]
    # at 5 %: the delta's low plane (nearly all of its bytes) goes to the fast Huff0 decoder, its high plane stays FSE (Huff0 cannot go below a bit per symbol)
    assert choice("delta_plane0", 50) == 1 and choice("delta_plane1", 50) == 0
    assert choice("plain_plane1", 20) == 1
    for name, (F, H) in sizes.items():
        assert choice(name, 0) == (0 if F < H else 1), name
        assert choice(name, 1000) == (1 if H <= 2 * F else 0), name
    assert sizes["delta_plane1"][1] > 2 * sizes["delta_plane1"][0]


@pytest.mark.parametrize("bsid", fmc.BSIDS)
def test_expected_choices_over_the_corpus_hold_both_codecs(checker, bsid):
    for tol in (0, 50):
        ch = fmc.choices(checker, bsid, tol)
        print("block-size id %d, tolerance %d: %s" % (bsid, tol, ch))
        assert set(ch) == {0, 1}, (bsid, tol)
    # the rule itself, on the errors too
    assert fmc.expected_choice(100, 100, 0) == (1, 100) and fmc.expected_choice(100, 101, 0) == (0, 100) and fmc.expected_choice(100, 105, 50) == (1, 105)
    assert fmc.expected_choice(1000, 1051, 50) == (0, 1000) and fmc.expected_choice(8, 16, 1000) == (1, 16) and fmc.expected_choice(8, 17, 1000) == (0, 8)
    assert fmc.expected_choice(-1, 9, 0) == (1, 9) and fmc.expected_choice(9, -1, 1000) == (0, 9) and fmc.expected_choice(-1, -3, 0) == (0, -1)


# ---------------------------------------------------------------------------------------------------------------- 4
def test_python_surface():
    from finitestateentropy_amd import api
    assert api.AutoCodec().tolerance_permille == 0 and api.AutoCodec(50).tolerance_permille == 50 and api.AutoCodec(50) == api.AutoCodec(50) != api.AutoCodec(20)
    for bad in (-1, 1001, 0.5, None):
        with pytest.raises(ValueError):
            api.AutoCodec(bad)
    par = list(inspect.signature(api.FseHip.frame_compress_packed_mixed_dbatch).parameters)
    assert par == ["self", "src", "src_offsets", "codecs", "tolerance_permille", "block_size_id", "dst", "capacity", "max_total_blocks", "align_log", "dst_offsets",
                   "workspace", "results"]
    par = inspect.signature(api.FseHip.tensor_compress_mixed_dbatch).parameters
    assert list(par)[:7] == ["self", "src", "src_offsets", "elem_bytes", "base", "codecs", "tolerance_permille"]
    assert par["base"].default is None and par["codecs"].default is None and par["tolerance_permille"].default == 0
    assert hasattr(api.FseHip, "frame_mixed_workspace_bound")
    # the pair keeps its parameter lists: `codec` only accepts more kinds of value
    assert list(inspect.signature(api.compress_tensors).parameters) == ["tensors", "codec", "block_size_id", "base"]
    assert list(inspect.signature(api.FseHip.compress_tensors).parameters) == ["self", "tensors", "codec", "block_size_id", "base"]
    assert list(inspect.signature(api.decompress_tensors).parameters) == ["obj", "base"]
    assert list(inspect.signature(api.CompressedTensors.__init__).parameters) == ["self", "groups", "dtypes", "shapes", "device", "codec", "block_size_id", "delta"]
    obj = api.CompressedTensors([], [], [], None, api.AutoCodec(50), 5)
    assert obj.codec == api.AutoCodec(50) and obj.delta is False


def test_workspace_bound_through_the_binding(lib):
    from finitestateentropy_amd import api
    hip = api.FseHip()
    for (nf, nb, bsid, policy), want in PINNED.items():
        assert hip.frame_mixed_workspace_bound(nf, nb, bsid, choose=policy == CHOOSE) == want
    with pytest.raises(ValueError):
        hip.frame_mixed_workspace_bound(1, 1, 7)
