"""FSEHIP_HUF_buildCTable_fromCount_batch / FSEHIP_HUF_writeCTable_batch with MANY tables per launch (k_huf_cprep<2, HPM_BUILD / HPM_WRITE> puts two
tables in a wave): the corpus of tests/huf_glue_corpus.py in corpus order, shuffled and in a pairing order that puts every ordered pair of distinct
classes -- refused tables included -- into one wave, every table against ref.huf_build_ctable / ref.huf_write_ctable case by case.  Strides, batch
sizes, garbage above maxSymbolValue, header capacities, refusals, argument checks, the chain against the one-shot call, and the headers read back."""
import itertools

import numpy as np
import pytest
import torch

import huf_glue_corpus as C
from oracle.oracle import is_error
from test_gpu_fse import s64
from test_gpu_glue_vectors import takes_m2

pytestmark = pytest.mark.gpu

MARK = 0x5A5A5A5A
UNSET = -77                                # fill of the result rows: a call that launches nothing leaves it


# ------------------------------------------------------------------------------------------------------------------------------
#  the corpus and the reference's answers, computed once
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hists():
    """the builder's rows: the corpus and, behind it, the refusal list (device expectations only)"""
    rows = [dict(c, refused_at=()) for c in C.builder_corpus()]
    rows += [dict(r, refused_at=r["limits"], id="refused:%s:%d" % (r["cls"], r["msv"])) for r in C.refused_hists()]
    for r in rows:
        r["count"].setflags(write=False)
    return rows


@pytest.fixture(scope="module")
def ref_built(ref, hists):
    """{(row, limit): (result, HUF_CElt[256])} of the reference for every row the model does not decline"""
    out = {}
    for i, h in enumerate(hists):
        for limit in C.LIMITS:
            if C.model_build(h["count"], h["msv"], limit) is not None:
                r, celt = ref.huf_build_ctable(h["count"], h["msv"], limit)
                assert not is_error(r)
                celt.setflags(write=False)
                out[(i, limit)] = (r, celt)
    return out


def _builder_expect(hists, ref_built, i, limit):
    """(signed result, HUF_CElt row or None for a refusal)"""
    if (i, limit) in ref_built:
        return ref_built[(i, limit)]
    h = hists[i]
    return (C.MSV_TOO_LARGE if h["msv"] > 255 else C.GENERIC), None


def _pairing_order(classes):
    """indexes such that every ordered pair of distinct classes sits at least once in slots (2k, 2k+1); classes: class per row"""
    members = {}
    for i, c in enumerate(classes):
        members.setdefault(c, []).append(i)
    turn = {c: 0 for c in members}
    order = []
    for a, b in itertools.permutations(sorted(members), 2):
        for c in (a, b):
            order.append(members[c][turn[c] % len(members[c])])
            turn[c] += 1
    return order


def _launch_builder(hip, hists, order, limit, stride=256, garbage=False):
    n = len(order)
    counts = np.stack([hists[i]["count"] for i in order]).astype(np.uint32)
    msv = np.array([hists[i]["msv"] for i in order], np.int32)
    if garbage:
        for k in range(n):
            counts[k, msv[k] + 1:] = 0xFFFFFFFF
    ct = torch.full((n, stride), MARK, dtype=torch.int32, device="cuda")
    res = torch.full((n,), UNSET, dtype=torch.int64, device="cuda")
    d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    hip.huf_build_ctable_from_count_batch(d_counts, torch.from_numpy(msv).cuda(), limit, ctables=ct, results=res)
    assert (d_counts.cpu().numpy().view(np.uint32) == counts).all(), "the counters are input"
    return ct.cpu().numpy().view(np.uint32), res.cpu().numpy()


def _check_builder(hists, ref_built, order, limit, tables, res, what):
    for k, i in enumerate(order):
        er, celt = _builder_expect(hists, ref_built, i, limit)
        msv = hists[i]["msv"]
        assert res[k] == s64(er), (what, k, hists[i]["id"], res[k], s64(er))
        if celt is None:
            assert (tables[k] == MARK).all(), (what, k, hists[i]["id"], "a refused table was written")
        else:
            assert (tables[k, :msv + 1] == celt[:msv + 1]).all(), (what, k, hists[i]["id"], np.nonzero(tables[k, :msv + 1] != celt[:msv + 1])[0][:8])
            assert not tables[k, msv + 1:256].any(), (what, k, hists[i]["id"], "entries above maxSymbolValue")
            assert (tables[k, 256:] == MARK).all(), (what, k, hists[i]["id"], "the gap behind the table")


def _orders(classes, seed):
    n = len(classes)
    return (("corpus", list(range(n))), ("shuffled", [int(x) for x in np.random.default_rng(seed).permutation(n)]), ("pairing", _pairing_order(classes)))


@pytest.mark.parametrize("limit", C.LIMITS)
def test_builder_whole_corpus_in_one_launch(hip, hists, ref_built, limit):
    """one launch per order: corpus order, shuffled, and every ordered pair of distinct classes (refusals are a class) side by side in a wave;
    table stride 256 and 260 (the gap keeps its mark); then every row again with 0xFFFFFFFF above its maxSymbolValue: nothing may change"""
    classes = ["refused" if (i, limit) not in ref_built else C.builder_class(h, limit) for i, h in enumerate(hists)]
    assert "refused" in classes and len(set(classes)) >= 8, sorted(set(classes))
    for (name, order), stride in zip(_orders(classes, 11 + limit), (256, 260, 260)):
        tables, res = _launch_builder(hip, hists, order, limit, stride)
        _check_builder(hists, ref_built, order, limit, tables, res, (limit, name))
        if name == "pairing":
            seen = {(classes[order[k]], classes[order[k + 1]]) for k in range(0, len(order), 2)}
            assert seen >= set(itertools.permutations(set(classes), 2))
        g_tables, g_res = _launch_builder(hip, hists, order, limit, stride, garbage=True)
        assert (g_res == res).all() and (g_tables == tables).all(), (limit, name, "garbage above maxSymbolValue changed the answer")


@pytest.mark.parametrize("n_blocks", (1, 2, 3))
def test_builder_small_batches(hip, hists, ref_built, n_blocks):
    """1, 2 and 3 tables (the last wave half empty), neighbours of different classes, maxSymbolValues differing per block"""
    classes = ["refused" if (i, 11) not in ref_built else C.builder_class(h, 11) for i, h in enumerate(hists)]
    pairing = _pairing_order(classes)
    for start in (0, 2, 40, 101):
        for limit in (11, 5):
            order = pairing[start:start + n_blocks]
            tables, res = _launch_builder(hip, hists, order, limit, 260)
            _check_builder(hists, ref_built, order, limit, tables, res, (limit, start, n_blocks))


def test_builder_refusals_beside_valid_tables(hip, hists, ref_built):
    """no symbol in use, more symbols than codes, maxSV 256, a count of 2^23: GENERIC / maxSymbolValue_tooLarge for that table alone, on either side
    of a valid neighbour, whose table is the reference's"""
    refused = [i for i, h in enumerate(hists) if h["refused_at"]]
    assert {hists[i]["cls"] for i in refused} == {"no_symbol", "more_symbols_than_codes", "msv_256", "count_2_23"}
    for limit in C.LIMITS:
        valid = [i for i in range(len(hists)) if (i, limit) in ref_built]
        order = []
        for k, r in enumerate(i for i in refused if limit in hists[i]["refused_at"]):
            order += [valid[(3 * k) % len(valid)], r, r, valid[(3 * k + 1) % len(valid)]]
        tables, res = _launch_builder(hip, hists, order, limit)
        _check_builder(hists, ref_built, order, limit, tables, res, ("refusals", limit))
        for k, i in enumerate(order):
            if limit in hists[i]["refused_at"]:
                assert res[k] == hists[i]["result"], (limit, hists[i]["cls"], res[k])


# ------------------------------------------------------------------------------------------------------------------------------
#  the writer
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def length_tables():
    rows = [dict(c, refused_at=()) for c in C.writer_corpus()]
    rows += [dict(r, refused_at=r["logs"], top=int(r["nb"].max()), id="refused:%s" % r["cls"]) for r in C.refused_tables()]
    return rows


def _writer_fits(t, log):
    return not t["refused_at"] and t["top"] <= log


def _writer_expect(ref, cache, length_tables, i, log, cap=256):
    """(result, header bytes or None for a refusal) -- the reference is asked only what the model says is defined"""
    key = (i, log, cap)
    if key not in cache:
        t = length_tables[i]
        if _writer_fits(t, log) and log <= 12:
            cache[key] = ref.huf_write_ctable(cap, C.celt_rows(t["nb"]), t["msv"], log)
        else:
            cache[key] = (C.MSV_TOO_LARGE if t["msv"] > 255 else C.GENERIC, None)
    return cache[key]


@pytest.fixture(scope="module")
def wcache():
    return {}


def _launch_writer(hip, length_tables, order, log, cap=256, stride=256, garbage=False):
    n = len(order)
    ct = np.full((n, stride), MARK, np.uint32)
    msv = np.array([length_tables[i]["msv"] for i in order], np.int32)
    for k, i in enumerate(order):
        ct[k, :256] = C.celt_rows(length_tables[i]["nb"])
        if garbage:
            ct[k, msv[k] + 1:256] = 0xFFFFFFFF
    d_ct = torch.from_numpy(ct.view(np.int32)).cuda()
    res = torch.full((n,), UNSET, dtype=torch.int64, device="cuda")
    width = max(cap, 256) + 7 + (hip.guard & 1)                                      # (the binding's guard bytes follow every row)
    hdr, _ = hip.huf_write_ctable_batch(d_ct, torch.from_numpy(msv).cuda(), log, header_capacity=cap, header_stride=width, results=res)
    assert hdr.stride(0) % 2 == 1 and hdr.stride(0) > cap, hdr.stride(0)            # odd, so the rows start at every byte alignment
    assert (d_ct.cpu().numpy().view(np.uint32) == ct).all(), "the tables (and the gap behind them) are input"
    return hdr.cpu().numpy(), res.cpu().numpy()


def _check_writer(ref, wcache, length_tables, order, log, cap, hdr, res, what):
    for k, i in enumerate(order):
        er, eh = _writer_expect(ref, wcache, length_tables, i, log, cap)
        assert res[k] == s64(er), (what, k, length_tables[i]["id"], res[k], s64(er))
        done = 0 if s64(er) < 0 else er
        if done:
            assert (hdr[k, :done] == eh[:done]).all(), (what, k, length_tables[i]["id"], np.nonzero(hdr[k, :done] != eh[:done])[0][:8])
        assert (hdr[k, done:] == 0xA5).all(), (what, k, length_tables[i]["id"], "bytes behind the header")


@pytest.mark.parametrize("log", C.HUFF_LOGS)
def test_writer_whole_corpus_in_one_launch(hip, ref, length_tables, wcache, log):
    """every length table that fits the huffLog, plus the refusal list, in corpus order, shuffled and with every ordered pair of distinct classes in
    one wave; header rows on an odd stride above the capacity; then again with 0xFFFFFFFF in the HUF_CElt entries above maxSymbolValue"""
    rows = [i for i, t in enumerate(length_tables) if _writer_fits(t, log) or log in t["refused_at"]]
    classes = ["refused" if length_tables[i]["refused_at"] else C.writer_class(ref, takes_m2, length_tables[i], log) for i in rows]
    assert {"refused"} | set(C.WRITER_CLASSES) == set(classes), sorted(set(classes))
    for (name, order), stride in zip(_orders(classes, 23 + log), (256, 260, 260)):
        if name == "pairing":
            seen = {(classes[order[k]], classes[order[k + 1]]) for k in range(0, len(order), 2)}
            assert seen >= set(itertools.permutations(set(classes), 2))
        order = [rows[j] for j in order]
        hdr, res = _launch_writer(hip, length_tables, order, log, 256, stride)
        _check_writer(ref, wcache, length_tables, order, log, 256, hdr, res, (log, name))
        g_hdr, g_res = _launch_writer(hip, length_tables, order, log, 256, stride, garbage=True)
        assert (g_res == res).all() and (g_hdr == hdr).all(), (log, name, "garbage above maxSymbolValue changed the answer")
        for n_blocks in (1, 2, 3):
            hdr, res = _launch_writer(hip, length_tables, order[:n_blocks], log, 256, stride)
            _check_writer(ref, wcache, length_tables, order[:n_blocks], log, 256, hdr, res, (log, name, n_blocks))


def test_writer_refusals(hip, ref, length_tables, wcache):
    """a length above huffLog beside valid neighbours (both ways round), and huffLog 13, which refuses every table of the call"""
    bad = next(i for i, t in enumerate(length_tables) if t["cls"] == "length_above_log")
    valid = [i for i, t in enumerate(length_tables) if _writer_fits(t, 8)]
    order = [valid[0], bad, bad, valid[1], valid[2]]
    hdr, res = _launch_writer(hip, length_tables, order, 8)
    _check_writer(ref, wcache, length_tables, order, 8, 256, hdr, res, "length above huffLog")
    assert res[1] == C.GENERIC and res[2] == C.GENERIC
    order = list(range(len(length_tables)))
    hdr, res = _launch_writer(hip, length_tables, order, 13)
    assert [int(r) for r in res] == [C.MSV_TOO_LARGE if length_tables[i]["msv"] > 255 else C.GENERIC for i in order]
    assert (hdr == 0xA5).all()


def test_writer_header_capacities(hip, ref, length_tables, wcache):
    """one table of each class at capacities full, full-1, full-2, 5, 1, full+1 (capacity is per call: the same batch at every capacity, so each
    table also sits beside neighbours for which that capacity is plenty or far too small): results and bytes of the reference"""
    order, caps = [], set()
    for cls in C.WRITER_CLASSES:
        order.append(next(i for i, t in enumerate(length_tables) if t["cls"] == cls and not t["refused_at"] and t["at_log"] == 12))
    for i in order:
        t = length_tables[i]
        full, _ = _writer_expect(ref, wcache, length_tables, i, 12)
        if is_error(full):
            full = (t["msv"] + 1) // 2 + 1
        caps |= {c for c in (full, full - 1, full - 2, 5, 1, full + 1) if c >= 1}
    assert len(order) == len(C.WRITER_CLASSES) and len(caps) >= 12
    errors = 0
    for cap in sorted(caps):
        hdr, res = _launch_writer(hip, length_tables, order, 12, cap)
        _check_writer(ref, wcache, length_tables, order, 12, cap, hdr, res, ("capacity", cap))
        errors += int((res < 0).sum())
    assert errors >= 20, errors


# ------------------------------------------------------------------------------------------------------------------------------
#  argument checks, the chain against the one-shot call, the headers read back
# ------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_launch_nothing(hip):
    """a table stride that is no multiple of 4 or below 256, a counter stride other than 256: hipErrorInvalidValue from both calls before any
    launch (results and outputs keep their fill); no blocks: success"""
    n = 4
    msv = torch.full((n,), 255, dtype=torch.int32, device="cuda")
    for stride in (258, 255):
        counts = torch.ones((n, 256), dtype=torch.int32, device="cuda")
        ct = torch.full((n, stride), 0x1234567, dtype=torch.int32, device="cuda")
        res = torch.full((n,), UNSET, dtype=torch.int64, device="cuda")
        with pytest.raises(RuntimeError, match="hipError 1$"):
            hip.huf_build_ctable_from_count_batch(counts, msv, 11, ctables=ct, results=res)
        assert bool((res == UNSET).all()) and bool((ct == 0x1234567).all()), stride
        ct.fill_(5 << 16)
        with pytest.raises(RuntimeError, match="hipError 1$"):
            hip.huf_write_ctable_batch(ct, msv, 11, results=res)
        assert bool((res == UNSET).all()), stride
    wide = torch.ones((n, 260), dtype=torch.int32, device="cuda")
    ct = torch.full((n, 256), 0x1234567, dtype=torch.int32, device="cuda")
    res = torch.full((n,), UNSET, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="hipError 1$"):
        hip.huf_build_ctable_from_count_batch(wide, msv, 11, ctables=ct, results=res)
    assert bool((res == UNSET).all()) and bool((ct == 0x1234567).all())
    torch.cuda.synchronize()
    empty = torch.zeros((0, 256), dtype=torch.int32, device="cuda")
    none = torch.zeros((0,), dtype=torch.int32, device="cuda")
    ct0, res0 = hip.huf_build_ctable_from_count_batch(empty, none, 11)
    hdr0, hres0 = hip.huf_write_ctable_batch(empty, none, 11)
    assert res0.numel() == 0 and hres0.numel() == 0


def test_chain_gives_the_one_shot_tables_and_headers(hip, ref):
    """hist_count_batch -> buildCTable_fromCount_batch at the one-shot's table log -> writeCTable_batch = huf_build_ctable_batch, on 32 probagen
    blocks of 4096 bytes"""
    src = hip.probagen_mixed((2, 14, 50, 80), 32, block_size=4096)
    ct1, hdr1, res1 = hip.huf_build_ctable_batch(src, table_log=11)
    counts, msv, _ = hip.hist_count_batch(src)
    msv_h, res1_h = msv.cpu().numpy(), res1.cpu().numpy()
    logs = np.array([ref.fse_optimal_tablelog(11, 4096, int(m), 1) for m in msv_h])
    coded = res1_h > 1
    assert coded.sum() >= 24, res1_h
    ct1_h, hdr1_h = ct1.cpu().numpy(), hdr1.cpu().numpy()
    for log in sorted(set(logs[coded])):
        sel = np.nonzero(coded & (logs == log))[0]
        idx = torch.from_numpy(sel).cuda()
        ct2, res2 = hip.huf_build_ctable_from_count_batch(counts[idx].contiguous(), msv[idx].contiguous(), int(log))
        res2_h = res2.cpu().numpy()
        assert (res2_h > 0).all() and (res2_h <= log).all()
        assert (ct2.cpu().numpy() == ct1_h[sel]).all(), log
        for tl in sorted(set(res2_h)):
            sub = np.nonzero(res2_h == tl)[0]
            j = torch.from_numpy(sub).cuda()
            hdr2, hres2 = hip.huf_write_ctable_batch(ct2[j].contiguous(), msv[idx][j].contiguous(), int(tl))
            hres2_h, hdr2_h = hres2.cpu().numpy(), hdr2.cpu().numpy()
            for k, b in enumerate(sel[sub]):
                assert hres2_h[k] == res1_h[b] and (hdr2_h[k, :hres2_h[k]] == hdr1_h[b, :res1_h[b]]).all(), (log, tl, b)


def test_headers_of_the_corpus_read_back(hip, ref, hists, ref_built):
    """closure: the device's tables of the corpus through the device's writer, and every header the reference's HUF_readDTableX1 accepts through
    huf_read_dtable_x1_batch / huf_read_dtable_x2_batch: results and tables of the reference"""
    headers = []
    for limit in (11, 12, 8):
        order = [i for i in range(len(hists)) if (i, limit) in ref_built and hists[i]["msv"] >= 1]
        tables, res = _launch_builder(hip, hists, order, limit)
        for tl in sorted(set(int(r) for r in res)):
            sub = [k for k in range(len(order)) if res[k] == tl]
            ct = torch.from_numpy(np.ascontiguousarray(tables[sub]).view(np.int32)).cuda()
            msv = torch.tensor([hists[order[k]]["msv"] for k in sub], dtype=torch.int32, device="cuda")
            hdr, hres = hip.huf_write_ctable_batch(ct, msv, tl)
            hdr, hres = hdr.cpu().numpy(), hres.cpu().numpy()
            for j, k in enumerate(sub):
                er, eh = ref.huf_write_ctable(256, ref_built[(order[k], limit)][1], hists[order[k]]["msv"], tl)
                assert hres[j] == s64(er), (limit, hists[order[k]]["id"])
                if not is_error(er):
                    assert (hdr[j, :er] == eh[:er]).all(), (limit, hists[order[k]]["id"])
                    if not is_error(ref.huf_read_dtable_x1(eh[:er], 12)[0]):
                        headers.append(eh[:er].copy())
    uniq = {h.tobytes(): h for h in headers}
    headers = list(uniq.values())
    assert len(headers) >= 20, len(headers)
    buf = np.full((len(headers), 160), 0xA5, np.uint8)
    for i, h in enumerate(headers):
        buf[i, :len(h)] = h
    d_src = torch.from_numpy(buf).cuda()
    d_sz = torch.tensor([len(h) for h in headers], dtype=torch.int64, device="cuda")
    dt1, r1 = hip.huf_read_dtable_x1_batch(d_src, d_sz, max_table_log=12)
    dt2, r2 = hip.huf_read_dtable_x2_batch(d_src, d_sz, max_table_log=12)
    dt1, r1, dt2, r2 = dt1.cpu().numpy().view(np.uint32), r1.cpu().numpy(), dt2.cpu().numpy().view(np.uint32), r2.cpu().numpy()
    for i, h in enumerate(headers):
        e1, t1 = ref.huf_read_dtable_x1(h, 12)
        e2, t2 = ref.huf_read_dtable_x2(h, 12)
        assert r1[i] == s64(e1) == len(h) and r2[i] == s64(e2), (i, r1[i], e1, r2[i], e2)
        tl = (int(t1[0]) >> 16) & 0xFF
        assert (dt1[i][:1 + (1 << (tl - 1))] == t1[:1 + (1 << (tl - 1))]).all(), i
        if not is_error(e2):
            assert (dt2[i] == t2[:dt2.shape[1]]).all(), i
