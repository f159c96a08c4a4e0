"""The X2 table rule on the CPU: the per-cell restatement of tests/huf_x2_corpus.py against the compiled reference's HUF_readDTableX2[_wksp]
(lib/huf_decompress.c:551-656) on every corpus entry -- the same result code, and on success the same 1 + (1 << maxTableLog) words.  The device
side is tests/test_gpu_huf_x2.py."""
import ctypes as C

import numpy as np
import pytest

import huf_x2_corpus as xc
from oracle.oracle import is_error


@pytest.fixture(scope="module")
def corpus(ref, restatement):
    return xc.build(ref, restatement)


def ref_read(ref, hdr, dt0, wksp=None):
    """the reference's HUF_readDTableX2 (wksp None) / HUF_readDTableX2_wksp into a DTable whose descriptor is dt0: (result, 4097 words)"""
    hdr = np.ascontiguousarray(hdr, dtype=np.uint8)
    dt = np.zeros(1 + (1 << 12), dtype=np.uint32)
    dt[0] = dt0
    vp = C.c_void_p
    if wksp is None:
        r = ref._call("HUF_readDTableX2", C.c_size_t, dt.ctypes.data_as(vp), hdr.ctypes.data_as(vp), C.c_size_t(hdr.size))
    else:
        ws = np.zeros(max(wksp, 4) // 4 + 1, dtype=np.uint32)
        r = ref._call("HUF_readDTableX2_wksp", C.c_size_t, dt.ctypes.data_as(vp), hdr.ctypes.data_as(vp), C.c_size_t(hdr.size), ws.ctypes.data_as(vp), C.c_size_t(wksp))
    return int(r), dt


def test_corpus_holds_its_shapes(corpus, restatement):
    xc.check_shapes(restatement, corpus)


def test_restatement_equals_reference_on_every_entry(corpus, ref, restatement):
    good = bad = 0
    for name, hdr, L in corpus:
        r, dt = ref.huf_read_dtable_x2(hdr, L)
        rm, words, _ = xc.model(restatement, hdr, L)
        assert rm == r, (name, rm, r)
        if is_error(r):
            bad += 1
            assert words is None and (dt[1:] == 0).all() and int(dt[0]) == L * 0x01000001, name      # the reference writes nothing either
        else:
            good += 1
            assert words.size == 1 + (1 << L) and (words == dt[:words.size]).all(), (name, np.nonzero(words != dt[:words.size])[0][:8])
            assert (dt[words.size:] == 0).all(), name
    print("\n  %d entries: %d tables equal word for word, %d refused with the reference's code" % (len(corpus), good, bad))
    assert good >= 150 and bad >= 150


def test_workspace_and_descriptor_as_found(corpus, ref, restatement):
    """the workspace check comes first and at 1500 bytes (:570-581), then maxTableLog > 12 (:587), then the header; the reserved byte stays"""
    assert xc.WKSP_THRESHOLD == 1500
    picks = [e for e in corpus if e[0] in ("p14_n32768_l11a@12", "p14_n32768_l11a@13", "two@1")] + [e for e in corpus if "_cut" in e[0]][:2]
    assert len(picks) == 5
    for name, hdr, L in picks:
        for wksp in (0, 1496, 1499, 1500, 2048):
            dt0 = L | (L << 16) | (0x5A << 24)
            r, dt = ref_read(ref, hdr, dt0, wksp)
            rm, words, _ = xc.model(restatement, hdr, L, reserved=0x5A, wksp=wksp)
            assert rm == r, (name, wksp, rm, r)
            if wksp < 1500:
                assert r == xc.ferr("tableLog_tooLarge")
            if not is_error(r):
                assert (words == dt[:words.size]).all(), (name, wksp)
