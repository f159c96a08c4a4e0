"""Weights headers for the double-symbol (X2) Huff0 table builder, and the rule of lib/huf_decompress.c:460-649 restated per cell in numpy.

The corpus (`build(ref, orc)`): entries (name, header bytes, maxTableLog), the headers made with the COMPILED REFERENCE --
  * real blocks: the headers HUF_compress2 writes for probagen blocks, P 2 / 14 / 20 / 50 / 80 at 257 / 5000 / 32768 bytes with huffLog 5, 8, 11, 12
    (P50 at huffLog 12 gives its one-bit symbol the weight 12, which HUF_readStats refuses, lib/entropy_common.c:189: kept, as a refused header);
  * hand-made histograms through HUF_buildCTable + HUF_writeCTable: two symbols (tableLog 1), equal counts (256 symbols -- the reference cannot write that
    header: equal weights do not compress and 255 of them do not fit the 4-bit form, HUF_writeCTable returns GENERIC; so also 128 and 64 of them),
    Fibonacci-like counts (depths 11 and 12), one heavy symbol beside many rare ones;
  * every header at maxTableLog = tableLog, tableLog + 1 and 12 (the three values of the rescale shift; minWeight clamped to 1 or not), tableLog - 1
    (the table cannot hold the code: tableLog_tooLarge) and 13 (refused before the header is read);
  * damaged headers: every truncation of four headers, 64 seeded byte flips.
`check_shapes()` asserts that the corpus holds what it is meant to hold, from the restatement's own account of every table.

The restatement (`model(orc, header, L)`): HUF_readStats in Python (its FSE-coded weights through the project's CPU restatement of FSE_decompress,
oracle/fse_oracle.c), then every cell of the table on its own, as the kernel computes it: L = maxTableLog, B = tableLog + 1;
  first level   classes ascend with the cell index, class starts rankVal0[w] = sum_{w' < w} rankStats[w'] << (w' + L - B); inside a class the symbols in
                symbol order; a symbol of weight w1 has n1 = B - w1 bits and owns 1 << (L - n1) cells
  single cells  minBits = B - maxW; L - n1 < minBits: {s1, n1, 1}
  second level  the offset v in the symbol's run indexes a sub-table of L - n1 bits; class starts rankVal0[w2] >> n1 (floors); minWeight =
                max(1, n1 + B - L); v below the start of class minWeight (minWeight > 1): the skip cell {s1, n1, 1}; else {s1 | s2 << 8, n1 + B - w2, 2},
                s2 by position among the classes w2 >= minWeight, 1 << (L - n1 - (B - w2)) cells each
  descriptor    {maxTableLog, tableType 1, tableLog = maxTableLog, reserved as found}
"""
import numpy as np

from oracle.oracle import is_error

ERR = {"GENERIC": 1, "dstSize_tooSmall": 2, "srcSize_wrong": 3, "corruption_detected": 4, "tableLog_tooLarge": 5}     # lib/error_public.h:45-56
PROBAS, SIZES, HUFFLOGS = (2, 14, 20, 50, 80), (257, 5000, 32768), (5, 8, 11, 12)
HUF_TABLELOG_MAX = 12
WKSP_THRESHOLD = 4 * ((HUF_TABLELOG_MAX + 1) * HUF_TABLELOG_MAX + (HUF_TABLELOG_MAX + 1) + (HUF_TABLELOG_MAX + 2) + 2 * 256 // 4 + 256 // 4)   # :570-581


def ferr(name):
    return (1 << 64) - ERR[name]


def header_size(first):
    """bytes of the weights header whose first byte is `first` (lib/entropy_common.c:164-181)"""
    return 1 + (first - 127 + 1) // 2 if first >= 128 else 1 + first


# ---------------------------------------------------------------------------------------------------------------- the restatement
def read_stats(orc, src):
    """HUF_readStats (lib/entropy_common.c:154-215): (header size or error, weights incl. the implied last one, tableLog)"""
    src = np.ascontiguousarray(src, dtype=np.uint8)
    if src.size == 0:
        return ferr("srcSize_wrong"), None, 0
    first = int(src[0])
    if first >= 128:
        n = first - 127
        isz = (n + 1) // 2
        if isz + 1 > src.size:
            return ferr("srcSize_wrong"), None, 0
        b = src[1:1 + isz].astype(np.int64)
        w = np.stack([b >> 4, b & 15], axis=1).reshape(-1)[:n]
    else:
        isz = first
        if isz + 1 > src.size:
            return ferr("srcSize_wrong"), None, 0
        body = src[1:1 + isz]
        # FSE_decompress_wksp(huffWeight, 255, ip + 1, iSize, .., 6), lib/fse_decompress.c:255-274: the NCount header, the limit, then the stream
        r, _, tl, _ = orc.fse_read_ncount(body if body.size else np.zeros(0, np.uint8), 255)
        if is_error(r):
            return r, None, 0
        if tl > 6:
            return ferr("tableLog_tooLarge"), None, 0
        r, out = orc.fse_decompress(body, 255)
        if is_error(r):
            return r, None, 0
        w = out[:r].astype(np.int64)
    if (w >= HUF_TABLELOG_MAX).any():
        return ferr("corruption_detected"), None, 0
    total = int(((1 << w) >> 1).sum())
    if total == 0:
        return ferr("corruption_detected"), None, 0
    tl = total.bit_length()
    if tl > HUF_TABLELOG_MAX:
        return ferr("corruption_detected"), None, 0
    rest = (1 << tl) - total
    if rest & (rest - 1):
        return ferr("corruption_detected"), None, 0
    w = np.concatenate([w, [rest.bit_length()]])
    n1 = int((w == 1).sum())
    if n1 < 2 or n1 & 1:
        return ferr("corruption_detected"), None, 0
    return isz + 1, w, tl


def model(orc, src, L, reserved=None, wksp=2048):
    """HUF_readDTableX2_wksp: (result, words -- 1 + (1 << L) uint32, or None on failure --, account of the table)"""
    if wksp < WKSP_THRESHOLD or L > HUF_TABLELOG_MAX:
        return ferr("tableLog_tooLarge"), None, None
    r, w, tl = read_stats(orc, src)
    if is_error(r):
        return r, None, None
    if tl > L:
        return ferr("tableLog_tooLarge"), None, None
    B = tl + 1
    order = np.argsort(w, kind="stable")
    order = order[w[order] > 0]                                  # symbols by (weight, symbol), weight >= 1
    stats = np.bincount(w, minlength=HUF_TABLELOG_MAX + 2)
    maxW = int(np.nonzero(stats[1:tl + 1])[0].max()) + 1
    base = np.zeros(HUF_TABLELOG_MAX + 2, np.int64)              # first list position of every class
    rv0 = np.zeros(HUF_TABLELOG_MAX + 2, np.int64)               # first cell of every class (first level)
    for k in range(1, HUF_TABLELOG_MAX + 2):
        base[k] = base[k - 1] + (stats[k - 1] if k > 1 else 0)
        rv0[k] = rv0[k - 1] + ((int(stats[k - 1]) << (k - 1 + L - B)) if k > 1 else 0)
    classes = np.arange(1, tl + 1)
    u = np.arange(1 << L, dtype=np.int64)
    w1 = classes[np.searchsorted(rv0[1:tl + 1], u, side="right") - 1]          # the last class that starts at or before the cell
    r1 = u - rv0[w1]
    lg1 = w1 + L - B
    n1 = B - w1
    s1 = order[base[w1] + (r1 >> lg1)]
    v = r1 & ((1 << lg1) - 1)
    minBits = B - maxW
    second = lg1 >= minBits
    st2 = rv0[None, 1:tl + 1] >> n1[:, None]                                    # second-level class starts, per cell
    k2 = (st2 <= v[:, None]).sum(axis=1) - 1                                    # (st2[:, 0] == 0: at least one)
    w2 = classes[k2]
    minWeight = np.maximum(1, n1 + B - L)
    two = second & (w2 >= minWeight)
    n2 = B - w2
    sh2 = np.where(two, lg1 - n2, 0)
    s2 = order[np.where(two, base[w2] + ((v - st2[u, k2]) >> sh2), 0)]
    cells = np.where(two, s1 | (s2 << 8) | ((n1 + n2) << 16) | (2 << 24), s1 | (n1 << 16) | (1 << 24)).astype(np.uint32)
    res = L if reserved is None else reserved
    words = np.concatenate([np.array([L | (1 << 8) | (L << 16) | (res << 24)], np.uint32), cells])
    account = {"tableLog": tl, "L": L, "two": int(two.sum()), "skip": int((second & ~two).sum()),
               "clamped": bool((second & (n1 + B - L < 1)).any()), "unclamped": bool((second & (n1 + B - L > 1)).any()),
               "kind": "raw" if int(src[0]) >= 128 else "fse"}
    return r, words, account


# ---------------------------------------------------------------------------------------------------------------- the corpus
def _written(ref, count, max_nb_bits):
    count = np.asarray(count, np.uint32)
    msv = len(count) - 1
    tl, celt = ref.huf_build_ctable(count, msv, max_nb_bits)
    assert not is_error(tl), tl
    h, out = ref.huf_write_ctable(256, celt, msv, tl)
    return None if is_error(h) else out[:h].copy()


def good_headers(ref, orc):
    """[(name, header)]: distinct headers the reference wrote"""
    out, seen = [], set()

    def add(name, hdr):
        key = hdr.tobytes()
        if key not in seen:
            seen.add(key)
            out.append((name, hdr))

    for P in PROBAS:
        for size in SIZES:
            for k, blk in enumerate(orc.probagen_batch(P, 2, size, 7 * P + size)):      # two seeds
                for hl in HUFFLOGS:
                    cs, c = ref.huf_compress2(blk, 255, hl)
                    if is_error(cs) or cs <= 1:
                        continue                                 # not compressible at this size: no header
                    add("p%d_n%d_l%d%s" % (P, size, hl, "ab"[k]), c[:header_size(int(c[0]))].copy())
    fib = [1, 1]
    while len(fib) < 14:
        fib.append(fib[-1] + fib[-2])
    hand = {"two": ([1, 1], 11), "flat256": ([1] * 256, 11), "flat128": ([1] * 128, 11), "flat64": ([3] * 64, 11),
            "fib11": (fib[:12], 11), "fib12": (fib[:13], 12), "fib14_cut11": (fib[:14] + [1, 1, 2], 11), "fib14_cut12": (fib[:14] + [5] * 40, 12),
            "heavy": ([100000] + [1] * 200, 11), "heavy12": ([1 << 20] + [1] * 60 + [30] * 20, 12)}
    for name, (count, nb) in hand.items():
        hdr = _written(ref, count, nb)
        if name == "flat256":
            assert hdr is None, "the reference wrote a header for 256 equal counts after all: use it"
            continue
        assert hdr is not None, name
        add(name, hdr)
    return out


def build(ref, orc):
    """[(name, header, maxTableLog)]"""
    rng = np.random.default_rng(20)
    heads = good_headers(ref, orc)
    entries = []
    for name, hdr in heads:
        _, _, tl = read_stats(orc, hdr)
        for L in sorted({tl, min(tl + 1, 12), 12, tl - 1, 13} if tl else {11, 12, 13}):      # (tl == 0: the header the reference cannot read)
            entries.append(("%s@%d" % (name, L), hdr, L))
    by_len = sorted(heads, key=lambda e: len(e[1]))
    fse = [e for e in by_len if e[1][0] < 128]
    raw = [e for e in by_len if e[1][0] >= 128]
    for name, hdr in (fse[0], fse[len(fse) // 2], raw[0], raw[-1]):
        for cut in range(len(hdr)):
            entries.append(("%s_cut%d" % (name, cut), hdr[:cut].copy(), 12))
    for i in range(64):
        name, hdr = heads[int(rng.integers(len(heads)))]
        bad = hdr.copy()
        pos = int(rng.integers(len(bad)))
        bad[pos] ^= np.uint8(rng.integers(1, 256))
        entries.append(("%s_flip%d" % (name, i), bad, 12 if i % 4 else 11))
    return entries


def check_shapes(orc, entries):
    """nothing passes by absence: the corpus holds every shape it is meant to hold"""
    acc = {}
    for name, hdr, L in entries:
        if "_cut" in name or "_flip" in name:
            continue
        r, _, a = model(orc, hdr, L)
        acc[name] = (r, a)
    ok = [a for r, a in acc.values() if a is not None]
    assert {a["kind"] for a in ok} == {"raw", "fse"}
    assert any(a["clamped"] for a in ok) and any(a["unclamped"] for a in ok)
    assert any(a["two"] == 0 for a in ok), "no table without a two-symbol cell"
    assert any(a["skip"] > 0 and a["two"] > 0 for a in ok), "no table with skip cells"
    triple = 0
    for name in {n.split("@")[0] for n in acc}:
        mine = {int(n.split("@")[1]): acc[n] for n in acc if n.split("@")[0] == name}
        if all(a is None for r, a in mine.values()):
            continue                                             # (a header the reference writes and cannot read: a weight of 12, lib/entropy_common.c:189)
        tl = max(a["tableLog"] for r, a in mine.values() if a is not None)
        assert mine[13][0] == ferr("tableLog_tooLarge") and mine[tl - 1][0] == ferr("tableLog_tooLarge"), name
        if tl <= 10:
            assert all(mine[L][1] is not None for L in (tl, tl + 1, 12)), name
            triple += 1
    assert triple >= 8, triple
    assert {a["tableLog"] for a in ok} >= {1, 5, 8, 11, 12}
    assert 200 <= len(entries) <= 900, len(entries)
