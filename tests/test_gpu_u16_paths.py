"""The labelled corpus of the 16-bit-symbol coder (tests/u16_corpus.py) on the device: FSE_compressU16 / FSE_decompressU16 through the host calls
and the batched calls against the COMPILED REFERENCE (oracle/_ref/libfse_ref.so, which travels with the snapshot) -- results, compressed
bytes, regenerated symbols, the symbols written in front of an error, all exact.  Every block runs alone at every capacity it lists and at
the addresses it lists (caller-made rows of odd stride on offset views: compressed rows at every address modulo 4, output rows at 0 2 4 6
modulo 8, source rows at every even address modulo 16, payloads at every address modulo 64), the whole corpus in one call, each table-log
class at batch sizes around the decoder's blocks per workgroup, workgroups of mixed fate, damaged streams between intact neighbours.

What the route assertions mean: the labels are the MODEL's (scripts/sim/u16_codec_sim.py, pinned on the CPU by tests/test_u16_corpus.py).
The tests assert that what ran here -- the same blocks, capacities and addresses -- carries every label, i.e. that the corpus on the device
is the corpus the CPU test vouched for.  They do not observe a route on the device: the kernels export no counters.

Where the reference is undefined the documented device behaviour is asserted instead (include/fsehip.h): a header with nothing behind it is
srcSize_wrong; 8 bytes or less behind a header that fits return the header writer's verdict (the header's size, or its error) and no
payload."""
import numpy as np
import pytest
import torch

import u16_corpus as uc

pytestmark = pytest.mark.gpu
sim = uc.sim
GUARD = 32                        # symbols / bytes of 0xA5 around every caller-made destination row


def s64(v):
    v = int(v)
    return v - (1 << 64) if v >= (1 << 63) else v


@pytest.fixture(scope="module")
def corpus(ref):
    D, C = uc.build(ref)
    return D, C


_RDEC, _RCOMP = {}, {}


def ref_decode(ref, b, cap):
    """(result, symbols written) the device must give: the reference's, or the documented refusal where the reference is undefined"""
    key = (b.name, cap)
    if key not in _RDEC:
        if not b.defined:
            _RDEC[key] = (uc.ferr("srcSize_wrong"), [])
        else:
            r, out = ref.fse_decompress_u16(b.comp, cap)
            k = r if not uc.is_err(r) else len(b.sim(cap)["out"])                  # in front of an error: the model's count, the reference's symbols
            _RDEC[key] = (r, out[:k].tolist())
    return _RDEC[key]


def ref_compress(ref, b, cap):
    key = (b.name, cap)
    if key not in _RCOMP:
        if b.ref_defined(cap):
            r, out = ref.fse_compress_u16(b.src, b.msv, b.tl, cap=cap)
            _RCOMP[key] = (r, out[:r].tobytes() if not uc.is_err(r) and r > 1 else b"")
        else:
            f = b.facts
            r, out = ref.fse_write_ncount(cap, f["norm"], f["msv"], f["tl"])     # the part of the call that is defined
            _RCOMP[key] = (r, out[:r].tobytes() if not uc.is_err(r) else b"")
    return _RCOMP[key]


def out_rows(n, cap, off, stride_pad=1):
    """caller-made output rows of 16-bit symbols with GUARD symbols of 0xA5A5 in front of and behind every row's capacity; the first row `off`
    bytes above a 256-byte boundary, an odd number of symbols from row to row -> (the view handed to the library, the whole rows)"""
    w = (2 * GUARD + max(cap, 1) + stride_pad) | 1
    buf = torch.full((n * w + 512,), 0xA5A5 - 0x10000, dtype=torch.int16, device="cuda")
    base = ((-buf.data_ptr()) % 256 + off) // 2
    rows = buf[base:base + n * w].view(n, w)
    return rows[:, GUARD:GUARD + max(cap, 1)], rows


def check_guard(rows, cap, what):
    h = rows.cpu().numpy().view(np.uint16)
    assert (h[:, :GUARD] == 0xA5A5).all() and (h[:, GUARD + cap:] == 0xA5A5).all(), "%s wrote outside its capacity" % what
    return h[:, GUARD:GUARD + cap]


def decode_batch(hip, ref, blocks, cap, off=0, out_off=0, caller_dst=True):
    """one FSE_decompressU16 batch over `blocks`, compared block by block"""
    csrc, _ = uc.device_bytes(torch, [b.comp for b in blocks], off)
    sizes = torch.tensor([len(b.comp) for b in blocks], dtype=torch.int64, device="cuda")
    if caller_dst:
        dst, rows = out_rows(len(blocks), cap, out_off)
        _, res = hip.fse_decompress_u16_batch(csrc, sizes, cap, dst=dst)
        torch.cuda.synchronize()
        out_h = check_guard(rows, cap, "FSE_decompressU16_batch")
    else:
        out, res = hip.fse_decompress_u16_batch(csrc, sizes, cap)                 # the binding's own rows: guard mode of the `hip` fixture
        torch.cuda.synchronize()
        out_h = out.cpu().numpy().view(np.uint16)
    res_h = res.cpu().numpy()
    for i, b in enumerate(blocks):
        rr, want = ref_decode(ref, b, cap)
        assert int(res_h[i]) == s64(rr), (i, b.name, cap, int(res_h[i]), s64(rr))
        assert out_h[i, :len(want)].tolist() == want, (i, b.name, cap)
    return csrc, dst if caller_dst else out


def test_geometry_of_the_decoder_launches():
    """blocks per workgroup, recomputed from u16d_launch's formula: 160 KiB of LDS, table slots of 4 / 8 KiB, 784 ring bytes and 48 control
    bytes per block, at most four blocks per service wave"""
    g = {}
    for log, srv in ((11, 9), (12, 5)):
        g[log] = min((160 * 1024 - 16) // ((2 << log) + (64 * 8 + 256 + 16) + 48), 4 * srv)
    assert g == {11: 33, 12: 18} and all(sim.launch_geometry(k) == v for k, v in g.items())


def test_decode_every_block_alone(hip, ref, corpus):
    D, _ = corpus
    n = 0
    for b in D:
        for cap in b.caps:
            rr, want = ref_decode(ref, b, cap)
            r, out = hip.fse_decompress_u16(b.comp, cap)                         # host pointers
            assert r == rr, (b.name, cap, r, rr)
            assert out[:len(want)].tolist() == want, (b.name, cap)
            if len(b.comp) == 0:
                continue
            csrc, dst = decode_batch(hip, ref, [b], cap, b.in_off, b.out_off)     # nBlocks == 1, the block's own addresses
            assert csrc.data_ptr() % 64 == b.in_off and dst.data_ptr() % 8 == b.out_off, b.name
            n += 1
    assert n >= 400


@pytest.mark.parametrize("cap", uc.BATCH_CAPS)
def test_decode_whole_corpus_in_one_call(hip, ref, corpus, cap):
    D, _ = corpus
    decode_batch(hip, ref, D, cap, off=3, caller_dst=False)
    order = np.random.RandomState(20 + cap).permutation(len(D))
    decode_batch(hip, ref, [D[i] for i in order], cap, off=30, out_off=6)


@pytest.mark.parametrize("cls", [11, 12])
def test_decode_batch_sizes_around_a_workgroup(hip, ref, corpus, cls):
    D, _ = corpus
    G = sim.launch_geometry(cls)
    assert G == (33 if cls == 11 else 18)
    pool = [b for b in D if b.n <= 2100 and b.sim(b.n)["cls"] == cls]
    assert len(pool) >= 20
    cap = 2100
    for k, nb in enumerate((1, G - 1, G, G + 1, 2 * G + 1)):
        blocks = [pool[(7 * k + i) % len(pool)] for i in range(nb)]
        decode_batch(hip, ref, blocks, cap, off=(k + 1) & 3, out_off=2 * (k & 3))


def test_decode_workgroups_of_mixed_fate(hip, ref, corpus):
    """one workgroup's range holds blocks of the other class, a header that fails, a header with nothing behind it, table log 13, blocks that
    never enter the bulk and one 20,000-symbol block among blocks of under 200 symbols; three orders, each its own workgroup of one call"""
    D, _ = corpus
    for name, (cls, grp) in uc.decode_company(D).items():
        G = sim.launch_geometry(cls)
        assert len(grp) == G
        batch = grp + grp[::-1] + grp[4:] + grp[:4]
        decode_batch(hip, ref, batch, uc.BATCH_CAPS[0], off=1, out_off=2)


def test_decode_damaged_streams_between_intact_neighbours(hip, ref, corpus):
    D, _ = corpus
    bad = [b for b in D if b.kind.startswith("damaged_")]
    good = [b for b in D if not b.kind.startswith("damaged_") and b.kind != "parse" and b.n <= 6000]
    assert len(bad) >= 100
    batch = []
    for i, b in enumerate(bad):
        batch += [good[(5 * i) % len(good)], b]
    batch.append(good[0])
    for cap in (6007, 6000):
        decode_batch(hip, ref, batch, cap, off=2, out_off=4)
    # the neighbours came out as they do alone: their rows are compared in full inside decode_batch (result and every symbol), and every
    # row's guard symbols are untouched


def compress_alone(hip, b, cap):
    src = uc.device_u16(torch, [b.src], b.src_off)
    dst, _ = uc.device_bytes(torch, [b""], (b.dst_off - GUARD) & 63, stride_pad=cap, guard=2 * GUARD, fill=0xA5)
    assert src.data_ptr() % 16 == b.src_off and (dst.data_ptr() + GUARD) % 64 == b.dst_off
    view = dst[:, GUARD:GUARD + max(cap, 1)]
    sizes = torch.tensor([b.n], dtype=torch.int64, device="cuda")
    _, res = hip.fse_compress_u16_batch(src, table_log=b.tl, max_symbol_value=b.msv, sizes=sizes, dst=view, dst_capacity=cap)
    torch.cuda.synchronize()
    h = dst.cpu().numpy()[0]
    assert (h[:GUARD] == 0xA5).all() and (h[GUARD + cap:] == 0xA5).all(), "FSE_compressU16_batch wrote outside its capacity (%s, %d)" % (b.name, cap)
    return int(res.cpu()[0]) & ((1 << 64) - 1), h[GUARD:GUARD + cap]


def test_compress_every_block_alone(hip, ref, corpus):
    _, C = corpus
    n = back = 0
    for b in C:
        for cap in b.caps:
            rr, want = ref_compress(ref, b, cap)
            r, out = hip.fse_compress_u16(b.src, b.msv, b.tl, cap=cap)           # host pointers
            assert r == rr, (b.name, cap, r, rr)
            assert out[:len(want)].tobytes() == want, (b.name, cap)
            r, out = compress_alone(hip, b, cap)                                  # nBlocks == 1: the block's own addresses, odd strides
            assert r == rr, (b.name, cap, r, rr)
            assert out[:len(want)].tobytes() == want, (b.name, cap)
            n += 1
            if not uc.is_err(rr) and b.sim(cap)["hdr"] is not None and rr > b.sim(cap)["hdr"]:   # a stream was written (result > 1, a payload behind the header): decode it on the device
                r2, sym = hip.fse_decompress_u16(out[:rr], b.n)
                assert r2 == b.n and (sym[:b.n] == b.src).all(), (b.name, cap)
                back += 1
    assert n >= 200 and back >= 100


def test_compress_shuffled_batches(hip, ref, corpus):
    """every compress-side block in batches of one (maxSymbolValue, tableLog) request each, shuffled, ragged sizes, caller-made rows of odd
    stride; what compressed is decoded again on the device in one call and compared with the source"""
    _, C = corpus
    groups = {}
    for b in C:
        if (b.msv or 286) <= 286 and (b.tl or 12) <= 13:                         # (an argument error is the whole call's: those blocks run alone)
            groups.setdefault((b.msv, b.tl), []).append(b)
    assert len(groups) >= 4
    total = 0
    for (msv, tl), blocks in sorted(groups.items()):
        order = np.random.RandomState(7 + tl).permutation(len(blocks))
        blocks = [blocks[i] for i in order]
        cap = max(b.bound for b in blocks)
        src = uc.device_u16(torch, [b.src for b in blocks], 2 * (tl & 7))
        dst, w = uc.device_bytes(torch, [b""] * len(blocks), 5 + tl, stride_pad=cap, guard=GUARD, fill=0xA5)
        sizes = torch.tensor([b.n for b in blocks], dtype=torch.int64, device="cuda")
        _, res = hip.fse_compress_u16_batch(src, table_log=tl, max_symbol_value=msv, sizes=sizes, dst=dst, dst_capacity=cap)
        torch.cuda.synchronize()
        h, res_h = dst.cpu().numpy(), res.cpu().numpy()
        assert (h[:, cap:] == 0xA5).all()
        keep = []
        for i, b in enumerate(blocks):
            rr, want = ref_compress(ref, b, cap)
            assert int(res_h[i]) == s64(rr), (b.name, int(res_h[i]), s64(rr))
            assert h[i, :len(want)].tobytes() == want, b.name
            if not uc.is_err(rr) and rr > 1:
                keep.append(i)
        total += len(blocks)
        if keep:
            idx = torch.tensor(keep, device="cuda")
            wide = max(blocks[i].n for i in keep)
            out, dres = hip.fse_decompress_u16_batch(dst[idx], res[idx], wide)
            torch.cuda.synchronize()
            out_h, dres_h = out.cpu().numpy().view(np.uint16), dres.cpu().numpy()
            for k, i in enumerate(keep):
                b = blocks[i]
                assert int(dres_h[k]) == b.n and (out_h[k, :b.n] == b.src).all(), b.name
    assert total >= 140


def test_the_corpus_that_ran_carries_every_label(corpus):
    """the blocks, capacities and addresses the tests above ran (each asserts its rows' addresses) are the ones tests/test_u16_corpus.py
    vouched for: the model gives every label for them.  Nothing here is observed on the device (see the module docstring)."""
    D, C = corpus
    lab = uc.corpus_labels(D, C)
    missing = [k for k in uc.LABELS if k not in lab]
    assert not missing, missing
