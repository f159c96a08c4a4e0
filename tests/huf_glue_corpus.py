"""Corpus for the Huff0 table glue on CALLER-made statistics (FSEHIP_HUF_buildCTable_fromCount_batch / FSEHIP_HUF_writeCTable_batch): histograms
for the builder and arbitrary length tables for the header writer, deterministic, every case with a class label, and the plain Python models that
assign the labels -- `limit_heights` restates the reference's height limit (lib/huf_compress.c:215-291: cut, debt, repair, overshoot) and logs the
branches it takes, `writer_class` restates the decisions of HUF_writeCTable / HUF_compressWeights (lib/huf_compress.c:63-147) on top of the compiled
reference's FSE calls.  tests/test_huf_glue_corpus.py pins both against the compiled reference on the CPU; tests/test_gpu_huf_glue_batch.py puts the
corpus through the device calls, neighbours of different classes in one wave.

Nothing compared with the reference here invokes what is undefined in it (tests/test_gpu_wksp.py): no symbol in use, more symbols than
2^limit, a limit above 12 on a deeper tree, a length above huffLog.  Those are refused_hists() and refused_tables(), which hold the device's answers only."""
import numpy as np

LIMITS = (0, 11, 12, 8, 5)               # maxNbBits of the builder launches (0 = HUF_TABLELOG_DEFAULT = 11)
HUFF_LOGS = (12, 11, 8)                  # huffLog of the writer launches
NONE = None
GENERIC, MSV_TOO_LARGE = -1, -6          # the device's refusals as signed results

# ---------------------------------------------------------------------------------------------------------------------------------
#  builder: the model
# ---------------------------------------------------------------------------------------------------------------------------------


def sorted_leaves(count, msv):
    """symbols in use in the reference's order (HUF_sort: count descending, ties in symbol order)"""
    return sorted((s for s in range(msv + 1) if count[s]), key=lambda s: (-int(count[s]), s))


def tree_depths(c):
    """depths of the leaves of the unlimited tree, c = counts descending (two or more): the two-queue merge of HUF_buildCTable_wksp (:357-384) -- the
    smaller head of the leaf queue and of the node queue is taken, the node queue on a tie"""
    L = len(c)
    nodes, par_leaf, par_node = [], [0] * L, []
    leaf, low_n = L - 1, 0
    for k in range(L - 1):
        total = 0
        for _ in range(2):
            lv = c[leaf] if leaf >= 0 else 1 << 31
            nv = nodes[low_n] if low_n < len(nodes) else 1 << 30
            if lv < nv:
                par_leaf[leaf] = k; total += lv; leaf -= 1
            else:
                par_node[low_n] = k; total += nv; low_n += 1
        nodes.append(total); par_node.append(-1)
    depth = [0] * (L - 1)
    for k in range(L - 3, -1, -1):
        depth[k] = depth[par_node[k]] + 1
    return [depth[par_leaf[r]] + 1 for r in range(L)]


def limit_heights(nb, c, M, log):
    """HUF_setMaxHeight on lengths `nb` by rank (ascending along the sorted leaves, changed in place), counts `c` by rank, limit M.  Returns the table
    log; `log` (a set) receives the branches taken: fits | cut, repair_hi_none / repair_lo_none / repair_count (how the search for a cheaper class went),
    overshoot_nonempty / overshoot_empty (class M-1 when an overpayment is given back)"""
    largest = nb[-1]
    if largest <= M:
        log.add("fits")
        return largest
    log.add("cut")
    debt, n = 0, len(nb) - 1
    while nb[n] > M:
        debt += (1 << (largest - M)) - (1 << (largest - nb[n]))
        nb[n] = M
        n -= 1
    while n >= 0 and nb[n] == M:
        n -= 1
    assert debt < 1 << 31, "the reference's int would overflow"
    debt >>= largest - M
    last = [NONE] * 14                                  # last[k]: last rank of length M - k
    cur = M
    for pos in range(n, -1, -1):
        if nb[pos] >= cur:
            continue
        cur = nb[pos]
        last[M - cur] = pos
    while debt > 0:
        k = debt.bit_length()
        while k > 1:
            hi, lo = last[k], last[k - 1]
            if hi is NONE:
                log.add("repair_hi_none"); k -= 1; continue
            if lo is NONE:
                log.add("repair_lo_none"); break
            if c[hi] <= 2 * c[lo]:
                log.add("repair_count"); break
            k -= 1
        while k <= 12 and last[k] is NONE:
            k += 1
        assert last[k] is not NONE, "no leaf left to lengthen: more symbols than codes"
        debt -= 1 << (k - 1)
        if last[k - 1] is NONE:
            last[k - 1] = last[k]
        r = last[k]
        nb[r] += 1
        last[k] = NONE if r == 0 else (r - 1 if nb[r - 1] == M - k else NONE)
    while debt < 0:
        if last[1] is NONE:
            log.add("overshoot_empty")
            while nb[n] == M:
                n -= 1
            nb[n + 1] -= 1
            last[1] = n + 1
        else:
            log.add("overshoot_nonempty")
            nb[last[1] + 1] -= 1
            last[1] += 1
        debt += 1
    return M


def model_build(count, msv, limit):
    """(table log, nbBits[256], branch log) of HUF_buildCTable(count, msv, limit) by the model; None where the device refuses"""
    M = limit or 11
    if msv > 255:
        return None
    order = sorted_leaves(count, msv)
    if not order or len(order) > 1 << M or max(int(count[s]) for s in order) >= 1 << 23:
        return None
    log = set()
    nb = np.zeros(256, np.uint8)
    if len(order) == 1:                                 # the reference's walk with one leaf gives it one bit (:357-384 with nonNullRank 0)
        nb[order[0]] = 1
        return 1, nb, {"fits"}
    c = [int(count[s]) for s in order]
    d = tree_depths(c)
    tl = limit_heights(d, c, M, log)
    for s, x in zip(order, d):
        nb[s] = x
    return tl, nb, log


BRANCH_CLASSES = ("overshoot_empty", "overshoot_nonempty", "repair_lo_none", "repair_hi_none", "repair_count", "cut_repaired")


def builder_class(case, limit):
    """the ONE class a histogram falls into at a limit (what the pairing order of the GPU test pairs): refused, else the rarest branch of the height
    limit it takes, else (the tree fits) the shape it was made as"""
    m = model_build(case["count"], case["msv"], limit)
    if m is None:
        return "refused"
    log = m[2]
    if "cut" not in log:
        return case["cls"]
    for b in BRANCH_CLASSES[:-1]:
        if b in log:
            return b
    return "cut_repaired"


# ---------------------------------------------------------------------------------------------------------------------------------
#  builder: the histograms
# ---------------------------------------------------------------------------------------------------------------------------------
def _place(values, msv, rng, keep_msv=True):
    """counts `values` on distinct symbols of 0..msv (symbol msv in use when keep_msv)"""
    c = np.zeros(256, np.uint32)
    k = len(values)
    pos = rng.choice(msv + 1, k, replace=False)
    if keep_msv and msv not in pos:
        pos[0] = msv
    c[pos] = np.asarray(values, np.uint32)
    return c


def make_hist(family, seed, k, msv):
    rng = np.random.default_rng(1000003 * seed + 7919 * k + msv)
    if family == "geo":                                 # geometric fall-off, the ratio from the seed
        r = 1.15 + 0.1 * (seed % 12)
        v = [max(1, int(3 * r ** i)) for i in range(k)]
        v = [min(x, (1 << 23) - 1) for x in v]
    elif family == "fib":                               # Fibonacci-like: the deepest tree a total allows
        v = [1, 1 + seed % 3]
        while len(v) < k:
            v.append(min(v[-1] + v[-2] + (seed >> 2) % 2, (1 << 23) - 1))
    elif family == "flat":
        v = [1 + seed] * k
    elif family == "runs":                              # long runs of equal counts: tie order decides who gets the shorter code
        levels = [1 + seed % 3, 2 + seed % 5, 5 + seed % 7, 40, 41, 500]
        v = [levels[(i * len(levels)) // k] for i in range(k)]
    elif family == "big":                               # counts at 2^23 - 1
        v = [(1 << 23) - 1] * (1 + seed % 4) + [int(x) for x in rng.integers(1, 1 << (4 + seed % 18), k - 1 - seed % 4)]
    elif family == "head":                              # a steep head over a flat tail
        h = 2 + seed % 5
        v = [int(x) for x in rng.integers(1000, 200000, h)] + [1 + seed % 4] * (k - h)
    else:                                               # "rand": counts of every magnitude
        v = [int(x) for x in (2.0 ** rng.uniform(0, 4 + seed % 16, k))]
    return _place(v[:k], msv, rng)


def _h(cls, family, seed, k, msv, at_limit=None):
    """at_limit: the limit at which a case found for a branch of the height limit takes it (None: a shape, whatever the limit does to it)"""
    return {"cls": cls, "count": make_hist(family, seed, k, msv), "msv": msv, "at_limit": at_limit, "id": "%s:%s:%d:%d:%d" % (cls, family, seed, k, msv)}


def builder_corpus():
    cases = []
    for seed in range(3):
        cases.append(_h("one_symbol", "flat", seed, 1, (0, 17, 255)[seed]))
        cases.append(_h("two_symbols", "geo", seed, 2, (1, 63, 200)[seed]))
        for k in (63, 64, 65):
            cases.append(_h("in_use_%d" % k, ("rand", "geo", "head")[seed], seed, k, (255, 130, 64 + seed)[seed] if k > 63 else (255, 62 + seed, 80)[seed]))
        for msv in (62, 63, 64):
            cases.append(_h("msv_%d" % msv, ("rand", "head", "flat")[seed], seed + 3, (40, msv + 1, 20)[seed], msv))
        cases.append(_h("flat_256", "flat", 7 * seed, 256, 255))
        cases.append(_h("tie_runs", "runs", seed, (200, 96, 30)[seed], (255, 100, 29)[seed]))
        cases.append(_h("big_counts", "big", seed + 1, (6, 20, 150)[seed], (20, 63, 255)[seed]))
        cases.append(_h("fibonacci", "fib", seed, (30, 20, 24)[seed], (255, 19, 63)[seed]))
    # found by a seeded search over the families above with the model's branch log (tests/test_huf_glue_corpus.py checks the labels against the
    # reference's lengths): the rare branches of the height limit
    for row in SEARCHED:
        cases.append(_h(*row))
    return cases


SEARCHED = (                                           # (class, family, seed, symbols in use, maxSV, the limit at which the class is taken)
    ('overshoot_empty', 'head', 0, 12, 20, 5), ('overshoot_empty', 'head', 0, 20, 40, 5), ('overshoot_empty', 'big', 0, 20, 40, 5),
    ('overshoot_empty', 'big', 0, 28, 63, 5),
    ('overshoot_nonempty', 'runs', 0, 20, 40, 5), ('overshoot_nonempty', 'runs', 0, 140, 200, 8), ('overshoot_nonempty', 'head', 1, 12, 20, 5),
    ('overshoot_nonempty', 'head', 1, 16, 15, 5),
    ('repair_lo_none', 'head', 0, 28, 63, 5), ('repair_lo_none', 'head', 0, 32, 31, 5), ('repair_lo_none', 'rand', 0, 12, 20, 5),
    ('repair_lo_none', 'big', 0, 32, 31, 5),
    ('repair_hi_none', 'geo', 0, 20, 40, 5), ('repair_hi_none', 'geo', 0, 28, 63, 5), ('repair_hi_none', 'fib', 0, 28, 63, 5),
    ('repair_hi_none', 'fib', 0, 24, 255, 5),
    ('repair_count', 'geo', 0, 32, 31, 8), ('repair_count', 'geo', 0, 33, 64, 8), ('repair_count', 'fib', 0, 12, 20, 8),
    ('repair_count', 'fib', 0, 20, 40, 0),
    ('cut_repaired', 'geo', 0, 16, 15, 5), ('cut_repaired', 'rand', 0, 20, 40, 5), ('cut_repaired', 'big', 0, 12, 20, 5),
    ('cut_repaired', 'big', 0, 33, 64, 8),
)


def refused_hists():
    """(count, msv, the device's result) -- undefined in the reference or outside the device's key width: never compared with the reference"""
    none = np.zeros(256, np.uint32)
    over = np.zeros(256, np.uint32); over[:40] = 3; over[7] = 1 << 23
    many = np.ones(256, np.uint32)
    return [{"cls": "no_symbol", "count": none, "msv": 255, "limits": LIMITS, "result": GENERIC},
            {"cls": "no_symbol", "count": none, "msv": 0, "limits": LIMITS, "result": GENERIC},
            {"cls": "more_symbols_than_codes", "count": many, "msv": 255, "limits": (5,), "result": GENERIC},
            {"cls": "more_symbols_than_codes", "count": many, "msv": 32, "limits": (5,), "result": GENERIC},
            {"cls": "msv_256", "count": many, "msv": 256, "limits": LIMITS, "result": MSV_TOO_LARGE},
            {"cls": "count_2_23", "count": over, "msv": 60, "limits": LIMITS, "result": GENERIC}]


# ---------------------------------------------------------------------------------------------------------------------------------
#  writer: the model and the length tables
# ---------------------------------------------------------------------------------------------------------------------------------
WRITER_CLASSES = ("fse", "one_weight", "no_weight_twice", "m2", "just_below_half", "at_half", "raw", "generic", "msv_0", "msv_1")


def weights_of(nb, msv, huff_log):
    """huffWeight[0 .. msv-1] of HUF_writeCTable (:126-130)"""
    return np.array([huff_log + 1 - int(x) if x else 0 for x in nb[:msv]], np.uint8)


def compress_weights(ref, takes_m2, w, cap=255):
    """HUF_compressWeights (:63-103) over the compiled reference's FSE calls: (size, notes)"""
    from oracle.oracle import is_error
    n = len(w)
    if n <= 1:
        return 0, {"tiny"}
    cnt = np.bincount(w, minlength=256).astype(np.uint32)
    top, max_w = int(cnt.max()), int(np.nonzero(cnt)[0].max())
    if top == n:
        return 1, {"one_weight"}
    if top == 1:
        return 0, {"no_weight_twice"}
    tl = ref.fse_optimal_tablelog(6, n, max_w, 2)
    notes = {"m2"} if takes_m2(tl, cnt, n, max_w) else set()
    r, norm = ref.fse_normalize_count(tl, cnt, n, max_w)
    assert not is_error(r)
    h, hdr = ref.fse_write_ncount(cap, norm, max_w, tl)
    if is_error(h):
        return h, notes
    _, ct = ref.fse_build_ctable(norm, max_w, tl)
    c, _ = ref.fse_compress_using_ctable(w, ct, cap - h)
    return (0 if c == 0 else h + c), notes


def writer_class(ref, takes_m2, case, huff_log):
    """the ONE class of a length table at a huffLog, by the model"""
    nb, msv = case["nb"], case["msv"]
    if msv < 2:
        return "msv_%d" % msv
    size, notes = compress_weights(ref, takes_m2, weights_of(nb, msv, huff_log))
    coded = 1 < size < msv // 2
    if "m2" in notes:                                   # FSE_normalizeCount left its main loop for FSE_normalizeM2, whatever becomes of the header
        return "m2"
    if not coded and msv > 128:
        return "generic"
    if "one_weight" in notes or "no_weight_twice" in notes:
        return next(iter(notes))
    if size == msv // 2:
        return "at_half"
    if not coded:
        return "raw"
    return "just_below_half" if size == msv // 2 - 1 else "fse"


def make_lengths(family, seed, msv, top):
    """nbBits[256] with every length <= top (entries above msv zero)"""
    rng = np.random.default_rng(7 * seed + 131 * msv + top)
    nb = np.zeros(256, np.uint8)
    k = msv + 1
    if family == "uniform":                             # every length as likely: the weights hardly compress
        nb[:k] = rng.integers(0, top + 1, k)
    elif family == "same":                              # one weight only
        nb[:k] = 1 + seed % top
    elif family == "distinct":                          # no weight twice (at most top + 1 symbols below msv)
        nb[:k] = rng.permutation(top + 1)[:k] if k <= top + 1 else 0
    elif family == "canon":                             # the lengths of a real code: few long-lived classes
        p = rng.dirichlet(np.full(k, 0.3 + 0.2 * (seed % 5)))
        nb[:k] = np.clip(np.ceil(-np.log2(np.maximum(p, 2.0 ** -top))), 1, top)
    elif family == "skew":                              # mostly one length, a few others
        nb[:k] = 1 + seed % top
        j = rng.choice(k, max(1, k // (3 + seed % 9)), replace=False)
        nb[j] = rng.integers(0, top + 1, len(j))
    else:                                               # "hist": lengths drawn to a given weight histogram (the M2 example of the issue and its kin)
        hist = [3, 2, 1, 3, 1, 2, 0, 2, 1, 1, 1, 4, 0][:top + 1]
        pool = np.repeat(np.arange(len(hist)), hist)
        w = np.concatenate([rng.permutation(pool), rng.integers(0, top + 1, max(0, k - len(pool)))])[:k]
        nb[:k] = np.where(w == 0, 0, top + 1 - w)
    return nb


def _t(cls, family, seed, msv, top, at_log):
    return {"cls": cls, "nb": make_lengths(family, seed, msv, top), "msv": msv, "top": top, "at_log": at_log,
            "id": "%s:%s:%d:%d:%d@%d" % (cls, family, seed, msv, top, at_log)}


SEARCHED_TABLES = (                                    # (class, family, seed, maxSV, longest length, the huffLog at which the class is taken)
    ('fse', 'hist', 0, 64, 6, 11), ('fse', 'hist', 0, 100, 8, 8), ('fse', 'hist', 0, 100, 8, 12), ('fse', 'hist', 0, 128, 8, 8),
    ('one_weight', 'skew', 0, 2, 6, 11), ('one_weight', 'same', 0, 2, 12, 12), ('one_weight', 'same', 0, 2, 11, 11), ('one_weight', 'same', 0, 5, 12, 12),
    ('one_weight', 'same', 3, 128, 8, 8),
    ('no_weight_twice', 'hist', 0, 2, 12, 12), ('no_weight_twice', 'hist', 0, 2, 11, 11), ('no_weight_twice', 'hist', 0, 5, 12, 12),
    ('no_weight_twice', 'canon', 0, 2, 12, 12), ('no_weight_twice', 'distinct', 1, 12, 12, 12), ('no_weight_twice', 'distinct', 2, 8, 8, 8),
    ('m2', 'hist', 0, 21, 12, 12), ('m2', 'hist', 1, 21, 12, 12),
    ('m2', 'hist', 0, 255, 12, 12), ('m2', 'hist', 0, 255, 11, 11), ('m2', 'uniform', 0, 180, 11, 11), ('m2', 'hist', 2, 180, 11, 11),
    ('just_below_half', 'hist', 0, 64, 8, 8), ('just_below_half', 'hist', 0, 180, 11, 11), ('just_below_half', 'canon', 0, 30, 8, 8),
    ('just_below_half', 'canon', 0, 30, 8, 12),
    ('at_half', 'hist', 0, 40, 6, 11), ('at_half', 'canon', 0, 21, 6, 11), ('at_half', 'canon', 0, 40, 11, 11), ('at_half', 'skew', 0, 30, 12, 12),
    ('raw', 'hist', 0, 5, 11, 11), ('raw', 'hist', 0, 5, 8, 8), ('raw', 'hist', 0, 9, 12, 12), ('raw', 'hist', 0, 9, 11, 11),
    ('generic', 'hist', 0, 129, 12, 12), ('generic', 'hist', 0, 129, 11, 11), ('generic', 'hist', 0, 180, 12, 12), ('generic', 'same', 0, 129, 12, 12),
    ('msv_0', 'hist', 0, 0, 12, 12), ('msv_0', 'hist', 0, 0, 11, 11), ('msv_0', 'canon', 0, 0, 12, 12), ('msv_0', 'canon', 0, 0, 11, 11),
    ('msv_1', 'hist', 0, 1, 12, 12), ('msv_1', 'hist', 0, 1, 11, 11), ('msv_1', 'canon', 0, 1, 12, 12), ('msv_1', 'canon', 0, 1, 11, 11),
    # short lengths, so that the launch at huffLog 8 sees every class too
    ('msv_0', 'hist', 0, 0, 8, 8), ('msv_1', 'hist', 0, 1, 8, 8), ('generic', 'same', 0, 129, 8, 8), ('raw', 'uniform', 0, 9, 8, 8),
    ('m2', 'hist', 0, 255, 8, 8), ('m2', 'hist', 3, 180, 8, 8), ('m2', 'hist', 4, 21, 8, 8),
)


def writer_corpus():
    """length tables with their class at huffLog `at_log` (found by a seeded search with `writer_class`; the CPU test checks every label)"""
    return [_t(*row) for row in SEARCHED_TABLES]


def celt_rows(nb):
    """HUF_CElt words (val | nbBits << 16) of a length table: HUF_writeCTable reads the lengths only, so val is just the symbol"""
    return (np.arange(256, dtype=np.uint32) & 0xFFFF) | (nb.astype(np.uint32) << 16)


def refused_tables():
    """(nb, msv, huffLog, the device's result): a length above huffLog indexes beyond the reference's bitsToWeight[], huffLog 13 overruns it"""
    nb = np.zeros(256, np.uint8); nb[:40] = 5; nb[3] = 9
    ok = np.zeros(256, np.uint8); ok[:40] = 5
    return [{"cls": "length_above_log", "nb": nb, "msv": 39, "logs": (8,), "result": GENERIC},
            {"cls": "huff_log_13", "nb": ok, "msv": 39, "logs": (13,), "result": GENERIC},
            {"cls": "msv_256", "nb": ok, "msv": 256, "logs": HUFF_LOGS, "result": MSV_TOO_LARGE}]
