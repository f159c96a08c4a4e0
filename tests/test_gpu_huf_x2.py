"""The double-symbol (X2) Huff0 family on the device against the compiled reference: HUF_readDTableX2[_wksp] (batch and single calls) word for
word on the corpus of tests/huf_x2_corpus.py, HUF_decompress4X2 / 1X2 and their DCtx forms on valid and damaged blocks, device-built tables fed
straight to the decoders, the strict _usingDTable forms, and the batch builder replayed from a HIP graph."""
import ctypes as C

import numpy as np
import pytest
import torch

import huf_x2_corpus as xc
from oracle.oracle import huf_compress_bound, is_error
from test_gpu_fse import s64
from test_huf_x2_model import ref_read

pytestmark = pytest.mark.gpu

W12 = 1 + (1 << 12)
PATTERN = 0x5A5A5A5A
GUARD_WORDS = 17                                                       # odd row stride: the tables start at all four offsets inside 16 bytes


@pytest.fixture(scope="module")
def corpus(ref, restatement):
    """[(name, header, maxTableLog, the reference's result, the reference's DTable)] -- computed once, never changed"""
    entries = xc.build(ref, restatement)
    xc.check_shapes(restatement, entries)
    out = []
    for name, hdr, L in entries:
        r, dt = ref.huf_read_dtable_x2(hdr, L)
        dt.setflags(write=False)
        out.append((name, hdr, L, r, dt))
    return out


def _headers_on_device(items):
    """(n, widest + 32) uint8 with 0xA5 behind every header, sizes"""
    n = len(items)
    width = max(len(e[1]) for e in items) + 32
    buf = np.full((n, width), 0xA5, np.uint8)
    sz = np.zeros(n, np.int64)
    for i, e in enumerate(items):
        buf[i, :len(e[1])] = e[1]
        sz[i] = len(e[1])
    return buf, torch.from_numpy(buf).cuda(), torch.from_numpy(sz).cuda()


def _check_tables(items, L, tables, res, what):
    words = 1 + (1 << min(L, 12))
    for i, (name, hdr, _, r, dt) in enumerate(items):
        assert res[i] == s64(r), (what, name, res[i], s64(r))
        if is_error(r):
            assert (tables[i, :words] == PATTERN).all(), (what, name, "a failing block wrote to its table")
        else:
            assert (tables[i, :words] == dt[:words]).all(), (what, name, np.nonzero(tables[i, :words] != dt[:words])[0][:8])
    assert (tables[:, words:] == PATTERN).all(), (what, "guard words behind the tables")


def test_builder_batch_whole_corpus_per_limit(hip, corpus):
    """every entry through FSEHIP_HUF_readDTableX2_batch, one call per limit: results, tables word for word, failed slots and guards untouched"""
    limits = sorted({e[2] for e in corpus})
    assert limits[0] == 0 and limits[-1] == 13 and {11, 12} <= set(limits)
    for L in limits:
        items = [e for e in corpus if e[2] == L]
        host, d_src, d_sz = _headers_on_device(items)
        words = 1 + (1 << min(L, 12))
        full = torch.full((len(items), words + GUARD_WORDS), PATTERN, dtype=torch.int32, device="cuda")
        dt, res = hip.huf_read_dtable_x2_batch(d_src, d_sz, L, dtables=full[:, :words])
        assert dt.data_ptr() == full.data_ptr()
        _check_tables(items, L, full.cpu().numpy().view(np.uint32), res.cpu().numpy(), "limit %d" % L)
        assert (d_src.cpu().numpy() == host).all(), "the headers are input"
    # the binding's own allocation (guarded like its neighbours' destinations): limit 12, uniform-size form on one header repeated
    items = [e for e in corpus if e[0] == "p14_n32768_l11a@12"] * 5
    _, d_src, _ = _headers_on_device(items)
    dt, res = hip.huf_read_dtable_x2_batch(d_src, len(items[0][1]), 12)
    assert tuple(dt.shape) == (5, W12) and (res.cpu().numpy() == s64(items[0][3])).all()
    assert (dt.cpu().numpy().view(np.uint32) == items[0][4][None, :]).all()


def test_builder_single_calls(hip, corpus, ref):
    """a shuffled sample through FSEHIP_HUF_readDTableX2 (host pointers): result, every word of the caller's DTable, the reserved byte as found"""
    rng = np.random.default_rng(5)
    pick = rng.permutation(len(corpus))[:48]
    for k, j in enumerate(pick):
        name, hdr, L, r, dt = corpus[int(j)]
        rg, dg = hip.huf_read_dtable_x2(hdr, L)
        assert rg == r and (dg == dt).all(), (name, rg, r)
        if k % 6 == 0:
            dt0 = L | (0x5A << 24) | (3 << 16)
            r2, d2 = ref_read(ref, hdr, dt0)
            mine = np.zeros(W12, np.uint32)
            mine[0] = dt0
            rg2, _ = hip.huf_read_dtable_x2(hdr, L, dtable=mine)
            assert rg2 == r2 and (mine == d2).all(), (name, hex(int(mine[0])), hex(int(d2[0])))


def test_builder_workspace_sizes(hip, corpus, ref):
    """HUF_readDTableX2_wksp at wkspSize 0, threshold - 4, threshold - 1, threshold, 2048 (threshold = 1500 bytes, :570-581)"""
    T = xc.WKSP_THRESHOLD
    picks = [e for e in corpus if e[0] in ("p14_n32768_l11a@12", "p14_n32768_l11a@13", "p14_n32768_l11a@10", "two@1")] + [e for e in corpus if "_cut" in e[0]][1:3]
    assert len(picks) == 6
    for name, hdr, L, _, _ in picks:
        for wksp in (0, T - 4, T - 1, T, 2048):
            r, dt = ref_read(ref, hdr, L * 0x01000001, wksp)
            rg, dg = hip.huf_read_dtable_x2(hdr, L, wksp_bytes=wksp)
            assert rg == r and (dg == dt).all(), (name, wksp, rg, r)


def _ref_x2(ref, base, csrc, dst_size, dctx=None, wksp=None):
    """the reference's HUF_decompress{4,1}X2 / _DCtx / _DCtx_wksp"""
    csrc = np.ascontiguousarray(csrc, dtype=np.uint8)
    out = np.zeros(max(dst_size, 1) + 16, np.uint8)
    out[dst_size:] = 0xA5
    vp, sz = C.c_void_p, C.c_size_t
    args = [out.ctypes.data_as(vp), sz(dst_size), csrc.ctypes.data_as(vp), sz(csrc.size)]
    if dctx is None:
        r = ref._call(base, sz, *args)
    elif wksp is None:
        r = ref._call(base + "_DCtx", sz, dctx.ctypes.data_as(vp), *args)
    else:
        ws = np.zeros(max(wksp, 4) // 4 + 1, np.uint32)
        r = ref._call(base + "_DCtx_wksp", sz, dctx.ctypes.data_as(vp), *args, ws.ctypes.data_as(vp), sz(wksp))
    assert (out[dst_size:] == 0xA5).all()
    return int(r), out[:dst_size]


def _ref_compress1x(ref, blk):
    cap = huf_compress_bound(len(blk))
    out = np.zeros(cap + 16, np.uint8)
    r = ref._call("HUF_compress1X", C.c_size_t, out.ctypes.data_as(C.c_void_p), C.c_size_t(cap), blk.ctypes.data_as(C.c_void_p), C.c_size_t(blk.size),
                  C.c_uint(255), C.c_uint(11))
    return int(r), out[:cap]


def _fresh_dctx(L=12):
    d = np.zeros(W12, np.uint32)
    d[0] = L * 0x01000001
    return d


@pytest.fixture(scope="module")
def blocks(ref, restatement):
    """[(P, size, block, HUF_compress2 output, HUF_compress1X output)] for P 2 / 14 / 80 at 257 / 5000 / 32768 bytes, where the block compresses"""
    out = []
    for P in (2, 14, 80):
        for size in (257, 5000, 32768):
            blk = np.ascontiguousarray(restatement.probagen_batch(P, 1, size, 300 + P + size)[0])
            c4, d4 = ref.huf_compress2(blk)
            c1, d1 = _ref_compress1x(ref, blk)
            out.append((P, size, blk, d4[:c4].copy() if c4 > 1 and not is_error(c4) else None, d1[:c1].copy() if c1 > 1 and not is_error(c1) else None))
    assert sum(b[3] is not None for b in out) >= 7 and sum(b[4] is not None for b in out) >= 7
    return out


def test_decompress_x2_forms(hip, ref, blocks):
    """HUF_decompress4X2 / _DCtx / _DCtx_wksp and the 1X2 family: result, bytes and the caller's dctx equal the reference's"""
    T = xc.WKSP_THRESHOLD
    for P, size, blk, c4, c1 in blocks:
        for base, fn, c in (("HUF_decompress4X2", hip.huf_decompress4x2, c4), ("HUF_decompress1X2", hip.huf_decompress1x2, c1)):
            if c is None:
                continue
            for dst_size in (size, size - 1):
                r, exp = _ref_x2(ref, base, c, dst_size)
                rg, og = fn(c, dst_size)
                assert rg == r, (base, P, size, dst_size, rg, r)
                if not is_error(r):
                    assert (og[:r] == exp[:r]).all()
                    assert dst_size != size or (og == blk).all()
            for L, wksp in ((12, None), (11, None), (12, 2048), (12, T), (12, T - 1), (5, None), (13, 2048)):
                dr, dg = _fresh_dctx(L), _fresh_dctx(L)
                r, exp = _ref_x2(ref, base, c, size, dr, wksp)
                rg, og = fn(c, size, dctx=dg, wksp_bytes=wksp)
                assert rg == r, (base, P, size, L, wksp, rg, r)
                assert (dg == dr).all(), (base, P, size, L, wksp, "dctx")
                if not is_error(r):
                    assert (og[:r] == exp[:r]).all() and (og == blk).all()
            # the error order of :883-889: a header that fills the block
            h = xc.header_size(int(c[0]))
            for cut in (h, h - 1, 0):
                dr, dg = _fresh_dctx(), _fresh_dctx()
                r, _ = _ref_x2(ref, base, c[:cut], size, dr)
                rg, _ = fn(c[:cut], size, dctx=dg)
                assert rg == r and (dg == dr).all(), (base, P, size, cut, rg, r)


def test_decompress_x2_damaged_streams(hip, ref, blocks):
    """twelve seeded truncated / flipped / jump-table-damaged blocks: the verdict of the reference's X2 decoder, and its bytes when it accepts"""
    rng = np.random.default_rng(12)
    usable = [b for b in blocks if b[3] is not None and b[1] >= 5000]
    for trial in range(12):
        P, size, blk, c4, c1 = usable[trial % len(usable)]
        four = trial % 4 != 3
        base, fn, c = ("HUF_decompress4X2", hip.huf_decompress4x2, c4) if four else ("HUF_decompress1X2", hip.huf_decompress1x2, c1)
        h = xc.header_size(int(c[0]))
        bad = c.copy()
        if trial % 3 == 0:
            bad = bad[:max(h + 10, len(bad) - int(rng.integers(1, 40)))]
        elif trial % 3 == 1:
            pos = rng.integers(h, len(bad), 4)
            bad[pos] ^= rng.integers(1, 256, 4).astype(np.uint8)
        else:
            bad[h:h + 6] = rng.integers(0, 256, 6, dtype=np.uint8)          # (4X: the jump table)
        r, exp = _ref_x2(ref, base, bad, size)
        rg, og = fn(bad, size)
        assert rg == r, (trial, base, P, size, rg, r)
        if not is_error(r):
            assert (og[:r] == exp[:r]).all(), (trial, base)


def test_device_built_tables_feed_the_decoders(hip, ref, blocks):
    """tables from the batch builder go straight to HUF_decompress4X_usingDTable_batch beside reference-built ones; the strict 4X2 / 1X2 forms
    refuse a table of type 0 with GENERIC, in the batch and in the single calls"""
    for streams in (4, 1):
        use = [(b[2], b[3] if streams == 4 else b[4], b[1]) for b in blocks if (b[3] if streams == 4 else b[4]) is not None]
        n = len(use)
        size = max(u[2] for u in use)
        cbuf = np.zeros((n, max(len(u[1]) for u in use) + 8), np.uint8)
        csz = np.array([len(u[1]) for u in use], np.int64)
        for i, u in enumerate(use):
            cbuf[i, :len(u[1])] = u[1]
        d_blocks = torch.from_numpy(cbuf).cuda()
        dt, hres = hip.huf_read_dtable_x2_batch(d_blocks, torch.from_numpy(csz).cuda(), 12)        # on the whole blocks: the header in front
        hres = hres.cpu().numpy()
        ref_tables = []
        for i, u in enumerate(use):
            r, t = ref.huf_read_dtable_x2(u[1], 12)
            assert hres[i] == s64(r) and not is_error(r)
            ref_tables.append(t)
        assert (dt.cpu().numpy().view(np.uint32) == np.stack(ref_tables)).all()
        sbuf = np.zeros_like(cbuf)
        ssz = csz - hres
        for i, u in enumerate(use):
            sbuf[i, :ssz[i]] = u[1][hres[i]:]
        d_s, d_ssz = torch.from_numpy(sbuf).cuda(), torch.from_numpy(ssz).cuda()
        d_dsz = torch.tensor([u[2] for u in use], dtype=torch.int64, device="cuda")
        d_ref = torch.from_numpy(np.stack(ref_tables).view(np.int32)).cuda()
        dispatch = hip.huf_decompress4x_using_dtable_batch if streams == 4 else hip.huf_decompress1x_using_dtable_batch
        strict = hip.huf_decompress4x2_using_dtable_batch if streams == 4 else hip.huf_decompress1x2_using_dtable_batch
        o1, r1 = dispatch(d_s, d_ssz, dt, d_dsz)
        o2, r2 = dispatch(d_s, d_ssz, d_ref, d_dsz)
        o3, r3 = strict(d_s, d_ssz, dt, d_dsz)
        assert torch.equal(r1, r2) and torch.equal(r1, d_dsz) and torch.equal(r3, d_dsz)
        o1, o2, o3 = o1.cpu().numpy(), o2.cpu().numpy(), o3.cpu().numpy()
        for i, u in enumerate(use):
            assert (o1[i, :u[2]] == u[0]).all() and (o2[i, :u[2]] == u[0]).all() and (o3[i, :u[2]] == u[0]).all(), (streams, i)
        # single-symbol tables in every other slot: the strict forms refuse exactly those
        mixed = np.stack(ref_tables).copy()
        for i in range(0, n, 2):
            r, t = ref.huf_read_dtable_x1(use[i][1], 11)
            assert not is_error(r)
            mixed[i] = 0
            mixed[i, :len(t)] = t[:W12]
        d_mixed = torch.from_numpy(mixed.view(np.int32)).cuda()
        _, r4 = strict(d_s, d_ssz, d_mixed, d_dsz)
        _, r5 = dispatch(d_s, d_ssz, d_mixed, d_dsz)
        r4, r5 = r4.cpu().numpy(), r5.cpu().numpy()
        for i, u in enumerate(use):
            assert r5[i] == u[2], (streams, i)
            assert r4[i] == (s64(xc.ferr("GENERIC")) if i % 2 == 0 else u[2]), (streams, i, r4[i])
        name = "HUF_decompress4X2_usingDTable" if streams == 4 else "HUF_decompress1X2_usingDTable"
        one = hip.huf_decompress4x2_using_dtable if streams == 4 else hip.huf_decompress1x2_using_dtable
        for i in (0, 1):
            strm = use[i][1][hres[i]:]
            out = np.zeros(use[i][2] + 16, np.uint8)
            r = int(ref._call(name, C.c_size_t, out.ctypes.data_as(C.c_void_p), C.c_size_t(use[i][2]), np.ascontiguousarray(strm).ctypes.data_as(C.c_void_p),
                              C.c_size_t(len(strm)), np.ascontiguousarray(mixed[i]).ctypes.data_as(C.c_void_p)))
            rg, og = one(strm, mixed[i], use[i][2])
            assert rg == r, (name, i, rg, r)
            assert (r == xc.ferr("GENERIC")) == (i == 0)
            if not is_error(r):
                assert (og == use[i][0]).all()


def test_builder_replays_from_a_hip_graph(hip, corpus):
    """one ordinary call, then the batch builder captured (one stream, linear) and replayed on new headers in the same buffers"""
    from finitestateentropy_amd.api import FseHip
    sets = [[e for e in corpus if e[2] == 12][k::3][:64] for k in range(3)]
    n = min(len(s) for s in sets)
    assert n >= 32
    sets = [s[:n] for s in sets]
    width = max(len(e[1]) for s in sets for e in s) + 32
    old = FseHip.guard
    FseHip.guard = 0                                      # (the guard's check synchronises: not inside a capture)
    try:
        d_src = torch.zeros((n, width), dtype=torch.uint8, device="cuda")
        d_sz = torch.zeros(n, dtype=torch.int64, device="cuda")
        full = torch.full((n, W12 + GUARD_WORDS), PATTERN, dtype=torch.int32, device="cuda")
        res = torch.zeros(n, dtype=torch.int64, device="cuda")
        ws = torch.empty(int(hip.lib.FSEHIP_HUF_readDTableX2_batch_workspaceSize(C.c_size_t(n))), dtype=torch.uint8, device="cuda")

        def load(items):
            host, _, _ = _headers_on_device(items)
            buf = np.full((n, width), 0xA5, np.uint8)
            buf[:, :host.shape[1]] = host
            d_src.copy_(torch.from_numpy(buf).cuda())
            d_sz.copy_(torch.tensor([len(e[1]) for e in items], dtype=torch.int64).cuda())
            full.fill_(PATTERN)

        def work():
            hip.huf_read_dtable_x2_batch(d_src, d_sz, 12, dtables=full[:, :W12], results=res, workspace=ws)
        load(sets[0]); work(); torch.cuda.synchronize()
        _check_tables(sets[0], 12, full.cpu().numpy().view(np.uint32), res.cpu().numpy(), "direct call")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            work()
        for k in (1, 2, 0):
            load(sets[k])
            g.replay()
            torch.cuda.synchronize()
            _check_tables(sets[k], 12, full.cpu().numpy().view(np.uint32), res.cpu().numpy(), "replay on set %d" % k)
    finally:
        FseHip.guard = old
