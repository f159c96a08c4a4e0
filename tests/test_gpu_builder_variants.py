"""The table builders come in two instantiations -- 32 cells per lane for launches whose tables have at most 2048 cells, 64 for tableLog 12
(csrc/fse_wave_build.h, the launchers of csrc/fse_tables.hip) -- and k_fse_dbuild runs both in one FSE_decompress call with maxLog 12.  One
batch of blocks whose FSE_optimalTableLog comes out at 9, 10, 11 and 12 (3,000 / 6,000 / 12,000 / 17,000 bytes: highbit(size - 1) - 2),
over alphabets of 2, 64, 65 and 256 symbols (one rank window, the first two-window alphabet, four windows) plus a histogram of one dominant
symbol beside symbols that occur once (counters -1 only), through every entry point that builds a table, against the COMPILED REFERENCE:
compressed bytes and round trips with workspaces for tableLog 11 and 12, decodes with maxLog 12 and (blocks of tableLog <= 11) maxLog 11,
and the tables of FSE_buildCTable_batch / FSE_buildDTable_batch word for word."""
import numpy as np
import pytest
import torch

from oracle.oracle import fse_compress_bound, fse_ctable_u32, fse_dtable_u32, is_error

pytestmark = pytest.mark.gpu


def s64(v):
    v = int(v)
    return v - (1 << 64) if v >= (1 << 63) else v

SIZES = {9: 3000, 10: 6000, 11: 12000, 12: 17000}               # tableLog FSE_optimalTableLog(12, size, .) picks -> block bytes
STRIDE = 17000


def make_rows():
    rng = np.random.default_rng(4242)
    rows = []
    for tl, size in SIZES.items():
        for nsym in (2, 64, 65, 256):
            w = rng.dirichlet(np.full(nsym, 0.2)) * 0.95 + 0.05 / nsym
            blk = rng.choice(nsym, size, p=w).astype(np.uint8)
            blk[:nsym] = np.arange(nsym, dtype=np.uint8)
            rows.append((tl, blk))
        blk = np.full(size, 7, np.uint8)                         # one dominant symbol, 120 symbols once each: counters -1 beside it
        blk[rng.choice(size, 120, replace=False)] = np.arange(100, 220, dtype=np.uint8)
        rows.append((tl, blk))
    return rows


@pytest.fixture(scope="module")
def batch(ref):
    rows = make_rows()
    buf = np.zeros((len(rows), STRIDE), np.uint8)
    for i, (_, blk) in enumerate(rows):
        buf[i, :len(blk)] = blk
    exp = {}
    for req in (11, 12):                                         # the reference once per requested table log
        per = []
        for want, blk in rows:
            n = len(blk)
            mx, msv, cnt = ref.hist_count(blk, 255)
            tl = ref.fse_optimal_tablelog(req, n, msv, 2)
            assert tl == min(want, req), (want, req, tl)
            r, norm = ref.fse_normalize_count(tl, cnt, n, msv)
            assert r == tl
            h, hdr = ref.fse_write_ncount(512, norm, msv, tl)
            _, ct = ref.fse_build_ctable(norm, msv, tl)
            _, dt = ref.fse_build_dtable(norm, msv, tl)
            c, comp = ref.fse_compress2(blk, 255, req)
            assert not is_error(c) and c > h
            rd = ref.fse_read_ncount(hdr[:h])[0]                     # (the header alone, nothing behind it)
            per.append({"tl": tl, "msv": msv, "norm": norm, "hdr": hdr[:h], "ct": ct, "dt": dt, "comp": comp[:c], "read": rd})
        exp[req] = per
    lows = sum(int((e["norm"] == -1).sum() >= 100 and (e["norm"] > 0).sum() == 1) for e in exp[12])
    assert lows == len(SIZES), lows                              # the histogram of -1 counters beside one symbol is what it says
    return {"rows": rows, "src": torch.from_numpy(buf).cuda(),
            "sizes": torch.tensor([len(b) for _, b in rows], dtype=torch.int64, device="cuda"), "exp": exp}


@pytest.mark.parametrize("req", [11, 12])
def test_compress_and_decode_with_both_instantiations(hip, batch, req):
    """workspace for tableLog 11: k_fse_cprep<32>; for 12: k_fse_cprep<64>.  Decode with maxLog 12: k_fse_dbuild<32> for the blocks of
    tableLog <= 11 and k_fse_dbuild<64> for those of 12 in one call; with maxLog 11 the 32-cell launch alone"""
    rows, exp = batch["rows"], batch["exp"][req]
    n = len(rows)
    dst, res = hip.fse_compress_batch(batch["src"], table_log=req, sizes=batch["sizes"], dst_capacity=fse_compress_bound(STRIDE))
    dst_h, res_h = dst.cpu().numpy(), res.cpu().numpy()
    for b in range(n):
        assert res_h[b] == len(exp[b]["comp"]), (req, b, res_h[b], len(exp[b]["comp"]))
        assert (dst_h[b][:res_h[b]] == exp[b]["comp"]).all(), (req, b)
    assert {e["tl"] for e in exp} == ({9, 10, 11, 12} if req == 12 else {9, 10, 11})
    out, dres = hip.fse_decompress_batch(dst, res, STRIDE, max_log=12)
    out_h, dres_h = out.cpu().numpy(), dres.cpu().numpy()
    for b in range(n):
        assert dres_h[b] == len(rows[b][1]) and (out_h[b][:dres_h[b]] == rows[b][1]).all(), (req, b, dres_h[b])
    small = [b for b in range(n) if exp[b]["tl"] <= 11]
    idx = torch.tensor(small, device="cuda")
    out, dres = hip.fse_decompress_batch(dst[idx].contiguous(), res[idx].contiguous(), STRIDE, max_log=11)
    out_h, dres_h = out.cpu().numpy(), dres.cpu().numpy()
    for k, b in enumerate(small):
        assert dres_h[k] == len(rows[b][1]) and (out_h[k][:dres_h[k]] == rows[b][1]).all(), (req, b, dres_h[k])
    if req == 12:                                                # maxLog 11 refuses the tableLog-12 blocks, as FSE_decompress_wksp does
        _, dres = hip.fse_decompress_batch(dst, res, STRIDE, max_log=11)
        for b in range(n):
            assert (dres[b].item() == -5) == (exp[b]["tl"] == 12), (b, dres[b].item())


@pytest.mark.parametrize("req", [11, 12])
def test_tables_word_for_word(hip, batch, req):
    rows, exp = batch["rows"], batch["exp"][req]
    n = len(rows)
    ct, hdr, res = hip.fse_build_ctable_batch(batch["src"], table_log=req, sizes=batch["sizes"])
    ct_h, hdr_h, res_h = ct.cpu().numpy().view(np.uint32), hdr.cpu().numpy(), res.cpu().numpy()
    for b in range(n):
        e = exp[b]
        assert res_h[b] == len(e["hdr"]) and (hdr_h[b][:res_h[b]] == e["hdr"]).all(), (req, b, "header")
        w = fse_ctable_u32(e["tl"], e["msv"])
        assert (ct_h[b][:w] == e["ct"][:w]).all(), (req, b, "ctable", np.nonzero(ct_h[b][:w] != e["ct"][:w])[0][:8])
    for max_log in (12, 11):
        pick = [b for b in range(n) if exp[b]["tl"] <= max_log]
        idx = torch.tensor(pick, device="cuda")
        dt, dres = hip.fse_build_dtable_batch(hdr[idx].contiguous(), res[idx].contiguous(), max_log=max_log)
        dt_h, dres_h = dt.cpu().numpy().view(np.uint32), dres.cpu().numpy()
        for k, b in enumerate(pick):
            e = exp[b]
            assert dres_h[k] == s64(e["read"]), (req, max_log, b, dres_h[k], e["read"])
            if is_error(e["read"]):
                continue
            w = fse_dtable_u32(e["tl"])
            assert (dt_h[k][:w] == e["dt"][:w]).all(), (req, max_log, b, "dtable", np.nonzero(dt_h[k][:w] != e["dt"][:w])[0][:8])
