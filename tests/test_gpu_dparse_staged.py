"""k_fse_dparse parses the NCount header from a copy of its first 256 bytes in LDS (csrc/ncount_reader.h: ncount_stage / StagedBytes) and takes
whatever lies beyond from memory: headers on both sides of that length, every truncation of them, and trailing garbage, against the COMPILED
REFERENCE -- return values (sizes and error codes) and decoded bytes of FSE_decompress block for block, in batches of one lane, a partial wave,
a full wave and two waves; the same headers through the single-call FSE_readNCount and the batched glue reader, which keep reading from memory.

The blocks: 600-4,096 bytes over all 256 symbols, a few frequent symbols and many rare ones (counters -1, 1, 2), normalised at a table log
chosen per block and put together with the reference's own step-by-step calls (FSE_compress2 would pick tableLog 9 for every one of these
sizes, and a tableLog-9 header of 256 symbols is 213-239 bytes).  Header sizes, checked against the reference below:
  224 (well inside the staged bytes), 254 / 255 / 256 / 257 / 258 (the last windows lie across the end of the staged bytes, or just before or
  behind it), 286 and 333 (tableLog 11 / 12: the parse goes on in memory)."""
import numpy as np
import pytest
import torch

from oracle.oracle import is_error

pytestmark = pytest.mark.gpu

STAGED = 256                     # NCS_BYTES of csrc/ncount_reader.h
CAP = 4096                       # dstCapacity of every decode: the largest block
# (bytes, frequent symbols, tableLog, seed) -> header bytes
BLOCKS = [((1000, 4, 9, 0), 224), ((4096, 4, 10, 0), 254), ((1000, 4, 10, 0), 255), ((2048, 4, 10, 0), 256), ((600, 4, 10, 0), 257),
          ((4096, 4, 10, 5), 258), ((1000, 4, 11, 0), 286), ((1000, 4, 12, 4), 333)]


def s64(v):
    v = int(v)
    return v - (1 << 64) if v >= (1 << 63) else v


def make_block(ref, size, hot, tl, seed):
    """-> (source bytes, header || payload, header bytes)"""
    rng = np.random.default_rng(seed)
    w = np.full(256, 0.25 / (256 - hot))
    w[rng.choice(256, hot, replace=False)] = 0.75 / hot
    src = rng.choice(256, size, p=w).astype(np.uint8)
    src[:256] = np.arange(256, dtype=np.uint8)                   # every symbol at least once
    cnt = np.bincount(src, minlength=256).astype(np.uint32)
    r, norm = ref.fse_normalize_count(tl, cnt, size, 255)
    assert r == tl
    h, hdr = ref.fse_write_ncount(512, norm, 255, tl)
    _, ct = ref.fse_build_ctable(norm, 255, tl)
    p, pay = ref.fse_compress_using_ctable(src, ct)
    assert not is_error(h) and not is_error(p) and p > 0
    return src, np.concatenate([hdr[:h], pay[:p]]), h


@pytest.fixture(scope="module")
def pool(ref):
    """every input of this module with what the reference makes of it, computed once: rows = list of byte arrays, `full` = the rows that are
    whole blocks, exp = [(FSE_decompress result, bytes)], hdr = [(FSE_readNCount result, maxSV, tableLog, counters)]"""
    rng = np.random.default_rng(99)
    rows, full, sizes = [], [], []
    for (size, hot, tl, seed), _ in BLOCKS:
        src, blk, h = make_block(ref, size, hot, tl, seed)
        sizes.append(h)
        full.append(len(rows))
        rows.append(blk)
        for k in (1, 3, 8):                                      # garbage behind the block
            rows.append(np.concatenate([blk, rng.integers(0, 256, k, dtype=np.uint8)]))
        for n in range(0, h + 5):                                # every truncation up to a little behind the header
            rows.append(blk[:n])
    exp = [ref.fse_decompress(r, CAP) for r in rows]
    hdr = [ref.fse_read_ncount(r, 255) for r in rows]
    return {"rows": rows, "full": full, "sizes": sizes, "exp": exp, "hdr": hdr}


def to_device(rows):
    """rows of different lengths -> (n, stride) uint8 filled with 0xA5 behind every row, sizes"""
    stride = max(max(len(r) for r in rows), 1) + 8
    buf = np.full((len(rows), stride), 0xA5, np.uint8)
    for i, r in enumerate(rows):
        buf[i, :len(r)] = r
    return torch.from_numpy(buf).cuda(), torch.tensor([len(r) for r in rows], dtype=torch.int64, device="cuda")


def check_decode(hip, pool, idx, max_log=12):
    csrc, csizes = to_device([pool["rows"][i] for i in idx])
    out, res = hip.fse_decompress_batch(csrc, csizes, CAP, max_log=max_log)
    out_h, res_h = out.cpu().numpy(), res.cpu().numpy()
    for k, i in enumerate(idx):
        r, eo = pool["exp"][i]
        assert res_h[k] == s64(r), (k, i, len(pool["rows"][i]), res_h[k], s64(r))
        if not is_error(r):
            assert (out_h[k][:r] == eo[:r]).all(), (k, i, len(pool["rows"][i]))


def test_generator_yields_headers_on_both_sides_of_the_staged_length(pool, ref):
    assert pool["sizes"] == [h for _, h in BLOCKS], pool["sizes"]
    assert min(pool["sizes"]) < STAGED - 4 and STAGED in pool["sizes"] and max(pool["sizes"]) > STAGED + 4
    for i in pool["full"]:                                       # the blocks are good ones: the reference decodes them
        r, _ = pool["exp"][i]
        assert not is_error(r) and r >= 600, (i, r)
        assert pool["hdr"][i][1] == 255


def test_every_truncation_and_garbage_in_one_batch(hip, pool):
    check_decode(hip, pool, list(range(len(pool["rows"]))))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_batches_of_one_lane_to_two_waves(hip, pool, n):
    """whole blocks, blocks with garbage and truncations around the end of each header, mixed: the last wave of 65 / 130 holds 1 / 2 lanes"""
    rows, near = pool["rows"], []
    for f, h in zip(pool["full"], pool["sizes"]):
        first = f + 4                                            # row of the truncation to 0 bytes
        near += [f, f + 1, f + 3] + [first + k for k in (0, 1, 3, 4, 15, 16, 17, h - 5, h - 1, h, h + 1, h + 4) if k <= h + 4]
    idx = [near[(7 * k) % len(near)] for k in range(n)]         # (the first one is a whole block: a batch of one decodes something)
    assert len(rows[idx[0]]) > 600
    check_decode(hip, pool, idx)


def test_max_log_below_the_tables_log(hip, pool):
    """the tableLog check behind the parse (lib/fse_decompress.c:266) on the staged path"""
    csrc, csizes = to_device([pool["rows"][i] for i in pool["full"]])
    _, res = hip.fse_decompress_batch(csrc, csizes, CAP, max_log=10)
    for k, ((_, _, tl, _), _) in enumerate(BLOCKS):
        assert (res[k].item() == -5) == (tl > 10), (k, tl, res[k].item())         # tableLog_tooLarge


def test_glue_readers_did_not_change(hip, pool):
    """FSE_readNCount as a batch call over every row, and as the single call over the rows around each header's end"""
    rows = pool["rows"]
    headers, sizes = to_device(rows)
    msv = torch.full((len(rows),), 255, dtype=torch.int32, device="cuda")
    norms, msv_out, tls, res = hip.fse_read_ncount_batch(headers, sizes, msv)
    norms_h, msv_h, tls_h, res_h = norms.cpu().numpy(), msv_out.cpu().numpy(), tls.cpu().numpy(), res.cpu().numpy()
    for i in range(len(rows)):
        r, m, tl, norm = pool["hdr"][i]
        assert res_h[i] == s64(r), (i, len(rows[i]), res_h[i], s64(r))
        if not is_error(r):
            assert msv_h[i] == m and tls_h[i] == tl and (norms_h[i][:m + 1] == norm[:m + 1]).all(), (i, len(rows[i]))
    for f, h in zip(pool["full"], pool["sizes"]):
        for i in [f, f + 2] + [f + 4 + k for k in (0, 3, 4, h - 1, h, h + 4)]:
            r, m, tl, norm = pool["hdr"][i]
            gr, gm, gtl, gnorm = hip.fse_read_ncount(rows[i], 255)
            assert gr == r, (i, len(rows[i]), gr, r)
            if not is_error(r):
                assert gm == m and gtl == tl and (gnorm[:m + 1] == norm[:m + 1]).all(), (i, len(rows[i]))
