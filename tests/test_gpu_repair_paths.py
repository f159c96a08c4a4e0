"""The repair corpus (tests/repair_corpus.py) through the device: every branch of k_fse_encode_wave's and k_huf_decode_par's
speculate / verify / repair loops against the compiled reference, byte for byte, alone and in company; and the lane-exact models
(scripts/sim/) against the device's own records of the instrumented builds (FSE_ENC_TIMING, HPAR_STATS)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import repair_corpus as rc
from oracle.oracle import fse_compress_bound, is_error

pytestmark = pytest.mark.gpu

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "finitestateentropy_amd", "csrc")
VARIANTS = {"enctiming": "-DFSE_ENC_TIMING", "hparstats": "-DHPAR_STATS"}


def s64(v):
    v = int(v)
    return v - (1 << 64) if v >= (1 << 63) else v


@pytest.fixture(scope="module")
def corpus(checker):
    groups = rc.enc_groups(checker)
    entries = rc.huf_entries(checker)
    rc.prepare_oneshot(checker, entries)
    return groups, entries


def _check_enc(checker, g, res, dst, idx, cap=None):
    for k, i in enumerate(idx):
        r, out = checker.fse_compress_using_ctable(g.blocks[i], g.cts[i], fse_compress_bound(len(g.blocks[i])) if cap is None else cap)
        assert res[k] == s64(r), (g.name, i, cap, res[k], r)
        if r:
            assert (dst[k][:r] == out[:r]).all(), (g.name, i, cap)


def _min_cap(checker, blk, ct):
    """the smallest capacity the reference accepts the block with (its result is monotone in the capacity)"""
    lo, hi = 1, fse_compress_bound(len(blk))
    while lo < hi:
        mid = (lo + hi) // 2
        if checker.fse_compress_using_ctable(blk, ct, mid)[0]:
            hi = mid
        else:
            lo = mid + 1
    return lo


def test_encoder_corpus_against_reference(hip, checker, corpus):
    """caller tables (TT4 / TT8 by the group's table log) in batch order, each block alone at its smallest capacity and one byte short,
    and the one-shot FSE_compress over the same blocks; the device decodes the reference's streams and the reference the device's"""
    groups, _ = corpus
    for g in groups:
        src, sizes, ct, _ = rc.enc_device_batch(g, torch)
        dst, res = hip.fse_compress_using_ctable_batch(src, ct, max_table_log=g.tl, sizes=sizes)
        _check_enc(checker, g, res.cpu().numpy(), dst.cpu().numpy(), range(len(g.blocks)))
        if g.name == "delta":
            continue                                        # (64 copies of one block: the batch above is what it is for)
        for i, blk in enumerate(g.blocks):
            cmin = _min_cap(checker, blk, g.cts[i])
            one = torch.from_numpy(blk[None]).cuda()
            for cap in (cmin, cmin - 1):
                d1, r1 = hip.fse_compress_using_ctable_batch(one, ct[i:i + 1], max_table_log=g.tl, dst_capacity=cap)
                _check_enc(checker, g, r1.cpu().numpy(), d1.cpu().numpy(), [i], cap)
            r, out = checker.fse_compress2(blk, 255, g.tl)
            d2, r2 = hip.fse_compress_batch(one, table_log=g.tl)
            assert r2[0].item() == s64(r), (g.name, i, r2[0].item(), r)
            if not is_error(r) and r > 1:
                dev = d2[0].cpu().numpy()[:r]
                assert (dev == out[:r]).all(), (g.name, i)
                o, dres = hip.fse_decompress_batch(torch.from_numpy(out[None, :r].copy()).cuda(), r, len(blk), max_log=12)
                assert dres[0].item() == len(blk) and (o[0].cpu().numpy()[:len(blk)] == blk).all(), (g.name, i)
                rr, back = checker.fse_decompress(dev, len(blk))
                assert rr == len(blk) and (back == blk).all(), (g.name, i)


def test_encoder_batch_independence(hip, checker, corpus):
    """every block (the delta sweep aside) gives the reference's result alone and at a random place beside random partners"""
    groups, _ = corpus
    rng = np.random.RandomState(3)
    for tl in (11, 12):
        pool = [(g, i) for g in groups if g.tl == tl and g.name != "delta" for i in range(len(g.blocks))]
        for trial in range(2):
            order = rng.permutation(len(pool))
            gs = [pool[k] for k in order]
            mix = rc.EncGroup("mix", tl, [g.specs[i] for g, i in gs], [g.blocks[i] for g, i in gs], [g.cts[i] for g, i in gs], None,
                              int(rng.randint(0, 64)))
            src, sizes, ct, _ = rc.enc_device_batch(mix, torch)
            dst, res = hip.fse_compress_using_ctable_batch(src, ct, max_table_log=tl, sizes=sizes)
            _check_enc(checker, mix, res.cpu().numpy(), dst.cpu().numpy(), range(len(gs)))
        for g, i in pool:
            one = rc.EncGroup("one", tl, [g.specs[i]], [g.blocks[i]], [g.cts[i]], None)
            src, sizes, ct, _ = rc.enc_device_batch(one, torch)
            dst, res = hip.fse_compress_using_ctable_batch(src, ct, max_table_log=tl)
            _check_enc(checker, one, res.cpu().numpy(), dst.cpu().numpy(), [0])


def _ref_huf(checker, e, payload=None):
    payload = e.payload if payload is None else payload
    f = checker.huf_decompress1x1_using_dtable if e.form == 1 else checker.huf_decompress4x1_using_dtable
    return f(payload, e.dt, e.dst_size)


def _check_huf(checker, es, res, out, payloads=None):
    for i, e in enumerate(es):
        r, ref = _ref_huf(checker, e, None if payloads is None else payloads[i])
        assert res[i] == s64(r), (e.name, res[i], r)
        if not is_error(r):
            assert (out[i][:r] == ref[:r]).all(), e.name


def _damaged(e):
    """a flipped bit inside the first lane that needed a repair, one in the middle of the payload, and the payload one byte short"""
    rec = e.simulate(decode=False)
    out = []
    st = rec["streams"][0] if rec["streams"] else None
    if st and st["pieces"] and any(st["pieces"][0]["reruns"]):
        j = next(k for k, v in enumerate(st["pieces"][0]["reruns"]) if v)
        L = len(e.payload) if e.form == 1 else int(e.payload[0]) | int(e.payload[1]) << 8
        Sd = (L + 3) // 4
        C = 32 * Sd - st["T0"] + (j * st["T0"]) // 64
        byte = (32 * Sd - 1 - C) // 8 + 6 * (e.form == 4)
        p = e.payload.copy(); p[min(max(byte, 0), len(p) - 1)] ^= 0x10; out.append(p)
    p = e.payload.copy(); p[len(p) // 2] ^= 0x04; out.append(p)
    out.append(e.payload[:-1].copy())
    return out


@pytest.mark.parametrize("form", [1, 4])
def test_huf_corpus_against_reference(hip, checker, corpus, form):
    """the corpus through the caller-table decoders (1X1 / 1X or 4X1 / 4X), the one-shot HUF_decompress, and damaged copies of the
    repair-heavy streams: the reference's result codes and bytes"""
    _, entries = corpus
    es = [e for e in entries if e.form == form]
    c, cs, dt, ds = rc.huf_device_batch(es, torch)
    fns = (hip.huf_decompress1x1_using_dtable_batch, hip.huf_decompress1x_using_dtable_batch) if form == 1 else \
          (hip.huf_decompress4x1_using_dtable_batch, hip.huf_decompress4x_using_dtable_batch)
    for fn in fns:
        out, res = fn(c, cs, dt, ds)
        _check_huf(checker, es, res.cpu().numpy(), out.cpu().numpy())
    one = [e for e in es if e.oneshot is not None]
    if one:
        cb = np.zeros((len(one), max(len(e.oneshot) for e in one) + 8), np.uint8)
        for i, e in enumerate(one):
            cb[i, :len(e.oneshot)] = e.oneshot
        out, res = hip.huf_decompress_batch(torch.from_numpy(cb).cuda(), torch.tensor([len(e.oneshot) for e in one], device="cuda"),
                                            torch.tensor([e.dst_size for e in one], device="cuda"))
        res, out = res.cpu().numpy(), out.cpu().numpy()
        for i, e in enumerate(one):
            r, ref = checker.huf_decompress(e.oneshot, e.dst_size)
            assert res[i] == s64(r) and (is_error(r) or (out[i][:r] == ref[:r]).all()), e.name
    heavy = [e for e in es if e.simulate(decode=False)["rounds"] >= 2]
    assert len(heavy) >= 8
    dmg, pls = [], []
    for e in heavy:
        for p in _damaged(e):
            dmg.append(e); pls.append(p)
    c, cs, dt, ds = rc.huf_device_batch(dmg, torch, pls)
    for fn in fns:
        out, res = fn(c, cs, dt, ds)
        _check_huf(checker, dmg, res.cpu().numpy(), out.cpu().numpy(), pls)


def test_huf_batch_independence(hip, checker, corpus):
    """every Huff0 corpus block alone and shuffled among partners of the other decoders (serial-only, multi-piece, raw tables)"""
    _, entries = corpus
    rng = np.random.RandomState(5)
    for form in (1, 4):
        es = [e for e in entries if e.form == form]
        fn = hip.huf_decompress1x1_using_dtable_batch if form == 1 else hip.huf_decompress4x1_using_dtable_batch
        extra = [rc.huf_entry(checker, "p2_big", ("proba", 2, 65536, 9), form), rc.huf_entry(checker, "p14_small", ("proba", 14, 900, 9), form)]
        pool = es + extra
        mix = [pool[k] for k in rng.permutation(len(pool))]
        c, cs, dt, ds = rc.huf_device_batch(mix, torch)
        out, res = fn(c, cs, dt, ds)
        _check_huf(checker, mix, res.cpu().numpy(), out.cpu().numpy())
        for e in es:
            c, cs, dt, ds = rc.huf_device_batch([e], torch)
            out, res = fn(c, cs, dt, ds)
            _check_huf(checker, [e], res.cpu().numpy(), out.cpu().numpy())


def _variant(name):
    lib = os.path.join(CSRC, "variants", name, "libfsehip.so")
    subprocess.check_call(["make", "-C", CSRC, "B=variants/" + name, "EXTRA=" + VARIANTS[name], "-j16"], stdout=subprocess.DEVNULL)
    assert os.path.exists(lib), lib
    return lib


def _child(variant, what, tmp_path):
    out = str(tmp_path / ("%s.npz" % what))
    env = dict(os.environ, FSEHIP_LIB=_variant(variant))
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "tests", "repair_corpus.py"), "device", what, out]
    subprocess.run(cmd, env=env, cwd=ROOT, check=True)
    return np.load(out)


def test_encoder_model_matches_device(checker, corpus, tmp_path):
    """FSE_ENC_TIMING build, caller-table batches (waves = consecutive blocks): rounds, nBad0 and firstBad of every wave equal the
    model's with the device's source addresses; the instrumented build's results and bytes are the reference's"""
    groups, _ = corpus
    d = _child("enctiming", "enc", tmp_path)
    waves_cmp, top = 0, 0
    for gi, g in enumerate(groups):
        rec, addrs = d["g%d_rec" % gi], [int(a) for a in d["g%d_addr" % gi]]
        waves, _ = g.simulate(addrs=addrs)
        for w, sim in enumerate(waves):
            dev = tuple(int(v) for v in rec[2 * w])
            assert dev == (sim["rounds"], sim["nBad0"], sim["firstBad"]), (g.name, w, dev, sim["rounds"], sim["nBad0"], sim["firstBad"])
            waves_cmp += 1
            top = max(top, dev[0])
        _check_enc(checker, g, d["g%d_res" % gi], d["g%d_dst" % gi], range(len(g.blocks)))
    print("\n  encoder: model == device on %d waves; most repair rounds on the device: %d" % (waves_cmp, top))


@pytest.mark.parametrize("form", [1, 4])
def test_huf_model_matches_device(checker, corpus, tmp_path, form):
    """HPAR_STATS build, caller-table batch: repair rounds and bad links of every block the model sends down the parallel path equal the
    device's; a block the model declines before staging leaves no record; results and bytes are the reference's"""
    _, entries = corpus
    es = [e for e in entries if e.form == form]
    d = _child("hparstats", "huf%d" % form, tmp_path)
    rec = d["rec"]
    n_cmp, top = 0, 0
    for i, e in enumerate(es):
        sim = e.simulate(decode=False)
        if sim["entered"]:
            assert (int(rec[i, 0]), int(rec[i, 1])) == (sim["rounds"], sim["bad"]), (e.name, rec[i, :2], sim["rounds"], sim["bad"])
            n_cmp += 1
            top = max(top, max((p["rounds"] for st in sim["streams"] for p in st["pieces"]), default=0))
        else:
            assert rec[i, 2] == 0, e.name                       # (never staged a stream)
    _check_huf(checker, es, d["res"], d["out"])
    # (the record sums a block's rounds over its streams and pieces; the most in one piece is the model's figure, checked through that sum)
    print("\n  Huff0 %dX: model == device on %d blocks; most repair rounds of a block on the device (summed over its streams): %d; "
          "most in one piece (model): %d" % (form, n_cmp, int(rec[:len(es), 0].max()), top))
