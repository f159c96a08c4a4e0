"""A corpus that reaches every branch of the two speculate / verify / repair kernels on purpose, each block labelled with what it reaches:
k_fse_encode_wave (csrc/fse_encode_wave.hip, model scripts/sim/wave_encoder_sim.py) and k_huf_decode_par (csrc/huf_decode_par.hip, model
scripts/sim/huf_par_sim.py).  Blocks come from fixed seeds and constructions; the seeds below were found once by `search()` (run this file:
`python tests/repair_corpus.py`) and rebuilding the corpus takes seconds.  Tables are the compiled reference's (the `checker`).

tests/test_repair_corpus.py checks on the CPU that every label is reached and that the corpus tells each broken model from the kernel's;
tests/test_gpu_repair_paths.py runs the corpus through the device against the reference and the models.
"""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", "sim", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


wsim = _load("wave_encoder_sim")
hsim = _load("huf_par_sim")

# ---------------------------------------------------------------------------------------------------------------------------- labels
# the branch list of the two kernels (the issue that introduced this corpus lists them); a branch added to a kernel needs a label here
ENC_LABELS = (
    ["tt4_rounds_%d" % k for k in range(7)] + ["tt4_rounds_7plus"] + ["tt8_rounds_%d" % k for k in range(7)] + ["tt8_rounds_7plus"] +
    ["sample_taken", "sample_taken_after_2_reruns", "merge_ck0", "merge_ck_mid", "merge_piece1", "rerun_to_end", "rerun_no_checkpoints",
     "warm_64", "warm_4096", "exact_start", "n_2048", "n_4097", "n_4098_m4096", "n_4099", "empty_ranges", "n_1MiB_every_gt1", "delta_all",
     "last_lane_delta", "wave_slow_fast", "wave_fast_slow", "odd_batch", "thin_one", "thin_all"])
HUF_LABELS = (
    ["h1_rounds_%d" % k for k in range(9)] + ["h1_over_8"] + ["h4_rounds_%d" % k for k in range(9)] + ["h4_over_8"] +
    ["pieces_1", "pieces_2", "pieces_3plus", "repair_later_piece", "spill", "min_bits_under", "min_bits_at", "dst_not_mult4",
     "verdict_fail", "prep_serial"])
MIN_COUNT = {}                     # label -> blocks (or waves) that must reach it; 1 where not listed
MIN_COUNT.update({"delta_all": 1, "sample_taken": 3, "merge_ck0": 2, "merge_piece1": 2, "rerun_to_end": 3, "exact_start": 3})


# ---------------------------------------------------------------------------------------------------------------------------- generators
def enc_random(seed):
    """the encoder search space at table log 11: slowly mixing blocks (probagen P80..P99, one dominant symbol, long runs) of assorted sizes"""
    rs = np.random.RandomState(seed)
    size = int(rs.choice([2048, 4097, 4098, 4099, 6000, 9000, 16384, 32768]))
    kind = int(rs.randint(0, 3))
    if kind == 0:
        return ("proba", int(rs.choice([80, 90, 95, 99])), size, int(rs.randint(1, 1 << 20)))
    if kind == 1:
        return ("dominant", size, int(rs.randint(1, 1 << 20)), float(rs.choice([0.9, 0.97, 0.995])), int(rs.randint(2, 30)))
    return ("runs", size, int(rs.randint(1, 1 << 20)), int(rs.randint(20, 2000)), int(rs.randint(2, 6)))


def enc_random12(seed):
    """the search space at table log 12: blocks of more than 16 KiB, the smallest that FSE_optimalTableLog(12, ..) gives 12 (states up
    to 8191, the warm-up from 1 << 12), mixing from fast (P14) to slow"""
    rs = np.random.RandomState(100000 + seed)
    size = int(rs.choice([16385, 20000, 32768, 32768, 49152]))
    kind = int(rs.randint(0, 3))
    if kind == 0:
        return ("proba", int(rs.choice([14, 30, 50, 70, 80, 90, 95, 99])), size, int(rs.randint(1, 1 << 20)))
    if kind == 1:
        return ("dominant", size, int(rs.randint(1, 1 << 20)), float(rs.choice([0.5, 0.8, 0.9, 0.97])), int(rs.randint(2, 60)))
    return ("runs", size, int(rs.randint(1, 1 << 20)), int(rs.randint(2, 400)), int(rs.randint(2, 12)))


ENC_SEARCH = {11: enc_random, 12: enc_random12}


def enc_bytes(orc, spec):
    kind = spec[0]
    if kind == "proba":
        _, P, size, seed = spec
        return orc.probagen_batch(P, 1, size, seed)[0]
    rs = np.random.RandomState(spec[2])
    size = spec[1]
    if kind == "dominant":                            # one symbol with probability p, k others evenly
        _, _, _, p, k = spec
        out = rs.randint(1, k + 1, size).astype(np.uint8)
        out[rs.random_sample(size) < p] = 0
        return out
    if kind == "runs":                                # runs of up to maxlen of a few symbols
        _, _, _, maxlen, k = spec
        out = np.zeros(size, np.uint8)
        pos = 0
        while pos < size:
            ln = int(rs.randint(1, maxlen)); out[pos:pos + ln] = rs.randint(0, k); pos += ln
        return out
    if kind == "singletons":                          # all zero but k distinct singletons: most ranges emit < 8 bits
        _, _, _, k = spec
        out = np.zeros(size, np.uint8)
        out[rs.choice(size, k, replace=False)] = np.arange(1, k + 1, dtype=np.uint8)
        return out
    if kind == "uniform":                             # k symbols evenly: fast mixing, short warm-up
        _, _, _, k = spec
        return rs.randint(0, k, size).astype(np.uint8)
    if kind == "one":                                 # one symbol: the table is built by hand (see enc_ctable)
        return np.zeros(size, np.uint8)
    if kind == "spaced":                              # zeros with a symbol every `period` bytes, none in lane `gap`'s range (source address 0 mod 64)
        _, _, _, period, gap = spec
        out = np.zeros(size, np.uint8)
        out[::period] = 1 + (np.arange(len(out[::period])) % 7)
        j0, j1 = wsim.cut(size, 0)[4][gap]
        out[size - j1:size - j0] = 0
        return out
    raise ValueError(kind)


def enc_ctable(orc, blk, tl_req, spec=None):
    """the reference's CTable for the block (FSE_optimalTableLog, FSE_normalizeCount, FSE_buildCTable); a one-symbol table by hand"""
    if spec is not None and spec[0] == "one":
        norm = np.array([1 << tl_req], np.int16)
        _, ct = orc.fse_build_ctable(norm, 0, tl_req)
        return ct
    mx, msv, cnt = orc.hist_count(blk)
    if mx == len(blk):
        return None                                   # one symbol: FSE_compress's RLE case, no table
    tl = orc.fse_optimal_tablelog(tl_req, len(blk), msv, 2)
    r, norm = orc.fse_normalize_count(tl, cnt, len(blk), msv)
    assert 0 < r < (1 << 63)
    _, ct = orc.fse_build_ctable(norm, msv, tl)
    return ct


ZERO = ("one", 32768, 0)                              # a partner that needs no repair round: every state merges after one symbol
FAST = ("proba", 14, 32768, 77)                       # fast mixing, but 30 links: one round

# found by search(): rounds -> seeds of ENC_SEARCH[table log] whose wave with ZERO needs that many (table log 12: tables of table log 12)
ENC_ROUNDS_SEEDS = {
    11: {1: [0], 2: [30], 3: [8], 4: [3], 5: [1], 6: [18], 7: [2], 8: [5], 15: [68]},
    12: {1: [3], 2: [6], 3: [1], 4: [5], 5: [12], 6: [91], 7: [43], 8: [44], 15: [0]},
}
# encoder groups: batches in order (waves = consecutive pairs); "stride" = source row stride, "base" the first row's address (mod 64)
ENC_FIXED = [
    dict(name="sizes", tl=11, blocks=[("proba", 80, 2048, 5), ("proba", 80, 4097, 5), ("proba", 80, 4098, 5), ("proba", 80, 4099, 5),
                                      ("proba", 95, 2048, 6), ("proba", 95, 4099, 6)]),
    dict(name="sizes12", tl=12, blocks=[("proba", 90, 4097, 8), ("proba", 90, 4098, 8), ("proba", 99, 2048, 9), ("proba", 99, 4099, 9)]),
    dict(name="empty_ranges", tl=11, blocks=[("proba", 80, 2050, 3), ("proba", 80, 2100, 3), ("proba", 90, 4160, 3)]),
    dict(name="slow_zero", tl=11, blocks=[("proba", 99, 32768, 21), ZERO, ZERO, ("proba", 99, 32768, 22), ("proba", 95, 9000, 23)]),
    dict(name="slow_zero12", tl=12, blocks=[ZERO, ("proba", 99, 32768, 24), ZERO, ZERO, FAST]),
    dict(name="thin", tl=12, blocks=[("singletons", 32768, 7, 40), ("singletons", 8192, 8, 3), ("one", 32768, 0), ("one", 4099, 0),
                                     ("uniform", 32768, 3, 200), ("uniform", 4099, 4, 250)]),
    dict(name="thin11", tl=11, blocks=[("singletons", 32768, 9, 40), ("singletons", 16384, 10, 12), ("spaced", 2048, 0, 16, 9),
                                       ("spaced", 32768, 0, 200, 20)]),
    dict(name="zero11", tl=11, blocks=[ZERO, ZERO, ("spaced", 2048, 0, 21, 3)]),
    dict(name="big", tl=11, blocks=[("proba", 95, 1 << 20, 31)]),
    dict(name="delta", tl=11, blocks=[("proba", 95, 32768, 41)] * 64, stride=32768 + 1),
    # delta carries the end of the block across a range bound: lastLane 22, not (m - 1) / C = 21
    dict(name="last_lane", tl=11, blocks=[("proba", 90, 4224, 42), ("proba", 95, 4224, 43)], stride=4224 + 64, base=60),
]


def huf_random(seed):
    """the Huff0 search space: a skewed background (symbol 0 rare enough to keep a two-bit code '11') with runs of symbol 0 -- a lane that
    enters such a run off the true codeword grid stays off it to the run's end -- 1X or 4X"""
    rs = np.random.RandomState(5000 + seed)
    size = int(rs.choice([8192, 16384, 32768]))
    form = int(rs.choice([1, 4]))
    nr = int(rs.randint(1, 4))
    runs = tuple((float(rs.uniform(0.0, 0.95)), int(rs.randint(50, 1500 if form == 4 else 2500))) for _ in range(nr))
    top = float(rs.choice([0.05, 0.12]))
    return ("zrun", seed, size, form, top, runs)


def huf_bytes(orc, spec):
    kind = spec[0]
    if kind == "zrun":
        _, seed, size, form, top, runs = spec
        rs = np.random.RandomState(seed)
        out = np.minimum(rs.geometric(0.15, size), 40).astype(np.uint8)
        out[rs.random_sample(size) < top] = 0
        for f, ln in runs:
            p = int(f * size); out[p:p + ln] = 0
        return out
    if kind == "proba":
        _, P, size, seed = spec[:4]
        return orc.probagen_batch(P, 1, size, seed)[0]
    raise ValueError(kind)


def huf_tables(orc, blk):
    mx, msv, cnt = orc.hist_count(blk)
    hl = orc.fse_optimal_tablelog(11, len(blk), msv, 1)
    mb, celt = orc.huf_build_ctable(cnt, msv, hl)
    hs, hdr = orc.huf_write_ctable(256, celt, msv, mb)
    _, dt = orc.huf_read_dtable_x1(hdr[:hs], 11)
    return celt, dt


# found by search(): (form, rounds) -> seeds of huf_random (rounds 99: beyond HPAR_MAX_REPAIR)
HUF_ROUNDS_SEEDS = {
    (1, 0): [9], (1, 1): [13], (1, 2): [26], (1, 3): [24], (1, 4): [15], (1, 5): [23], (1, 6): [74], (1, 7): [10], (1, 8): [60], (1, 99): [21],
    (4, 0): [0], (4, 1): [6], (4, 2): [33], (4, 3): [17], (4, 4): [46], (4, 5): [261], (4, 6): [119], (4, 7): [4], (4, 8): [91], (4, 99): [5],
}
# fixed Huff0 entries: (name, spec, form, dst_size or None, damage) -- damage = (byte, bit) flipped in the payload.  The sizes put the
# stream at 512 / 513 bytes (T0 just under / at HPAR_MIN_BITS); the two flips in a 1X stream's last bits fail the last piece's verdict, the
# first on its end alone (the count is right), the second on the count
HUF_FIXED = [
    ("min_bits_under_1x", ("proba", 14, 968, 3), 1, None, None),
    ("min_bits_at_1x", ("proba", 14, 970, 3), 1, None, None),
    ("min_bits_at_4x", ("proba", 14, 3924, 3), 4, None, None),
    ("dst_odd_4x", ("proba", 14, 10001, 3), 4, None, None),
    ("dst_odd_4x_2", ("proba", 80, 10002, 4), 4, None, None),
    ("pieces_1x", ("proba", 14, 32768, 5), 1, None, None),
    ("pieces_4x", ("proba", 2, 65536, 5), 4, None, None),
    ("spill_4x", ("proba", 90, 32768, 6), 4, None, None),
    ("spill_1x", ("proba", 95, 16384, 6), 1, None, None),
    ("prep_4x", ("proba", 80, 5000, 3), 4, None, None),
    ("verdict_end_1x", ("proba", 14, 16384, 5), 1, None, (0, 1)),
    ("verdict_count_1x", ("proba", 14, 16384, 5), 1, None, (1, 1)),
    ("short_dst_1x", ("proba", 14, 16384, 5), 1, 16383, None),
]


# ---------------------------------------------------------------------------------------------------------------------------- corpus
class EncGroup:
    def __init__(self, name, tl, specs, blocks, cts, stride, base=0):
        self.name, self.tl, self.specs, self.blocks, self.cts, self.base = name, tl, specs, blocks, cts, base
        self.stride = stride or (max(len(b) for b in blocks) + 63) // 64 * 64

    def addrs(self):
        return [(self.base + i * self.stride) % 64 for i in range(len(self.blocks))]

    def simulate(self, addrs=None, mut=None):
        addrs = self.addrs() if addrs is None else addrs
        Bs = [wsim.Block(b, ct, a, self.tl, mut=mut) for b, ct, a in zip(self.blocks, self.cts, addrs)]
        return wsim.simulate_batch(Bs), Bs


def enc_groups(orc):
    cache = {}

    def blk(spec):
        if spec not in cache:
            cache[spec] = enc_bytes(orc, spec)
        return cache[spec]
    out = []
    for tl, seeds in ENC_ROUNDS_SEEDS.items():
        for r, ss in sorted(seeds.items()):
            for s in ss:
                specs = [ENC_SEARCH[tl](s), ZERO]
                out.append(EncGroup("rounds%d_tl%d_s%d" % (r, tl, s), tl, specs, [blk(x) for x in specs], None, None))
    for g in ENC_FIXED:
        out.append(EncGroup(g["name"], g["tl"], g["blocks"], [blk(x) for x in g["blocks"]], None, g.get("stride"), g.get("base", 0)))
    for g in out:
        g.cts = [enc_ctable(orc, b, g.tl, sp) for b, sp in zip(g.blocks, g.specs)]
    return out


def enc_labels(group, waves):
    """labels -> count for one simulated group"""
    from collections import Counter
    lab = Counter()
    recs = [b for w in waves for b in w["blocks"]]
    for w in waves:
        # TT4: the batch's max table log <= 11 (4-byte entries); TT8: a table of table log 12 (13-bit states) -- the one that re-ran, or any
        # in a wave without repairs.  (A table of 11 or less in a batch of max table log 12 runs the TT8 template but earns no TT8 label.)
        on = [b for b in w["blocks"] if b["on"]]
        busy = [b for b in on if any(l["reruns"] for l in b["lanes"])] or on
        tt = "tt4" if group.tl <= 11 else ("tt8" if busy and max(b["tl"] for b in busy) == 12 else None)
        if tt:
            lab["%s_rounds_%s" % (tt, w["rounds"] if w["rounds"] < 7 else "7plus")] += 1
        bl = w["blocks"]
        if len(bl) == 2:
            slow = [any(l["reruns"] for l in b["lanes"]) for b in bl]
            quiet = [b["on"] and not any(l["reruns"] for l in b["lanes"]) for b in bl]
            if slow[0] and quiet[1]:
                lab["wave_slow_fast"] += 1
            if quiet[0] and slow[1]:
                lab["wave_fast_slow"] += 1
    if len(group.blocks) % 2 == 1 and len(group.blocks) > 1:
        lab["odd_batch"] += 1
    deltas = set()
    for r in recs:
        if not r["on"]:
            continue
        n = r["n"]
        lab.update({"n_2048": n == 2048, "n_4097": n == 4097, "n_4098_m4096": r["m"] == 4096, "n_4099": n == 4099,
                    "empty_ranges": r["lastLane"] < 31, "n_1MiB_every_gt1": n == 1 << 20 and r["every"] > 1,
                    "warm_64": r["warm"] == 64, "warm_4096": r["warm"] == 4096,
                    "last_lane_delta": r["lastLane"] < 31 and r["lastLane"] != (r["m"] - 1) // r["C"]})
        if r["C"] >= 64:
            deltas.add(r["delta"])
        if r["result"]:
            if r["thin"] == 1:
                lab["thin_one"] += 1
            if r["lastLane"] > 0 and r["thin"] == r["lastLane"]:
                lab["thin_all"] += 1
        rer = [x for l in r["lanes"] for x in l["reruns"]]
        lab.update({"exact_start": any(l["exact"] for l in r["lanes"]),
                    "sample_taken": any(l["takes"] for l in r["lanes"]),
                    "sample_taken_after_2_reruns": any(t >= 2 for l in r["lanes"] for t in l["takes"]),
                    "merge_ck0": any(x[0] == "merge" and x[2] == 0 for x in rer),
                    "merge_ck_mid": any(x[0] == "merge" and x[1] == 0 and x[2] > 0 for x in rer),
                    "merge_piece1": any(x[0] == "merge" and x[1] == 1 for x in rer),
                    "rerun_to_end": any(x[0] == "end" for x in rer),
                    "rerun_no_checkpoints": bool(rer) and r["every"] == 0x7FFFFFFF})
    if len(deltas) == 32:
        lab["delta_all"] += 1
    return +lab


class HufEntry:
    def __init__(self, name, blk, form, dst_size, payload, dt, oneshot):
        self.name, self.blk, self.form, self.dst_size, self.payload, self.dt, self.oneshot = name, blk, form, dst_size, payload, dt, oneshot

    def simulate(self, mut=None, decode=True):
        return hsim.simulate_block(self.payload, self.dt, self.dst_size, self.form, decode=decode, mut=mut)


def huf_entry(orc, name, spec, form=None, dst_size=None, damage=None):
    blk = huf_bytes(orc, spec)
    form = form or (spec[3] if spec[0] == "zrun" else 4)
    celt, dt = huf_tables(orc, blk)
    r, s = (orc.huf_compress1x_using_ctable if form == 1 else orc.huf_compress4x_using_ctable)(blk, celt)
    assert r > 0, name
    payload = s[:r].copy()
    if damage is not None:
        payload[damage[0]] ^= 1 << damage[1]
    oneshot = None
    if form == 4 and damage is None and dst_size is None:
        cs, c = orc.huf_compress2(blk, 255, 11)
        oneshot = c[:cs].copy() if cs > 1 else None
    return HufEntry(name, blk, form, len(blk) if dst_size is None else dst_size, payload, dt, oneshot)


def huf_entries(orc):
    out = []
    for (form, r), ss in sorted(HUF_ROUNDS_SEEDS.items()):
        for s in ss:
            out.append(huf_entry(orc, "h%d_rounds%d_s%d" % (form, r, s), huf_random(s)))
    for name, spec, form, dst, damage in HUF_FIXED:
        out.append(huf_entry(orc, name, spec, form, dst, damage))
    return out


def huf_labels(e, rec):
    from collections import Counter
    lab = Counter()
    f = "h%d" % e.form
    if rec["entered"]:
        for st in rec["streams"]:
            pcs = st["pieces"]
            fail = any(p.get("fail") == "rounds" for p in pcs)
            if fail:
                lab[f + "_over_8"] += 1
            else:
                lab["%s_rounds_%d" % (f, max(p["rounds"] for p in pcs))] += 1
            if not any(p.get("fail") for p in pcs):
                lab["pieces_%s" % (len(pcs) if len(pcs) < 3 else "3plus")] += 1
            lab["repair_later_piece"] += any(p["rounds"] for p in pcs[1:])
            lab["spill"] += any(p["spill"] for p in pcs)
            lab["verdict_fail"] += any(p.get("fail") == "verdict" for p in pcs)
            if st["T0"] - 4096 in range(8):
                lab["min_bits_at"] += 1
        if e.dst_size % 4:
            lab["dst_not_mult4"] += e.form == 4
    elif rec["reason"] == "block" and e.form == 1 and 4096 - 8 <= 8 * (len(e.payload) - 1) < 4096:
        lab["min_bits_under"] += 1
    if e.oneshot is not None:
        h, _ = e.oneshot_dt
        prec = hsim.simulate_block(e.oneshot[h:], e.oneshot_dt[1], e.dst_size, 4, oneshot=True, decode=False)
        lab["prep_serial"] += prec["reason"] == "prep"
    return +lab


def prepare_oneshot(orc, entries):
    for e in entries:
        if e.oneshot is not None:
            h, dt = orc.huf_read_dtable_x1(e.oneshot, 11)
            e.oneshot_dt = (h, dt)


# ---------------------------------------------------------------------------------------------------------------------------- search
def search(n_enc=160, n_huf=300, per=1, tls=(11, 12), huf=True):
    """development aid: the seeds behind ENC_ROUNDS_SEEDS and HUF_ROUNDS_SEEDS (prints them)"""
    from oracle.oracle import Checker
    orc = Checker()
    zero = enc_bytes(orc, ZERO)
    for tl in tls:
        found = {}
        zct = enc_ctable(orc, zero, tl, ZERO)
        for s in range(n_enc):
            spec = ENC_SEARCH[tl](s)
            b = enc_bytes(orc, spec)
            ct = enc_ctable(orc, b, tl)
            if ct is None or (ct[0] & 0xFFFF) != tl:
                continue
            g = EncGroup("", tl, [spec, ZERO], [b, zero], [ct, zct], None)
            waves, _ = g.simulate()
            r = waves[0]["rounds"]
            if len(found.setdefault(r, [])) < per:
                found[r].append(s)
        print("tl", tl, dict(sorted(found.items())))
    if not huf:
        return
    found = {}
    for s in range(n_huf):
        spec = huf_random(s)
        try:
            e = huf_entry(orc, "", spec)
        except AssertionError:
            continue
        rec = e.simulate(decode=False)
        if not rec["entered"]:
            continue
        pr = [p for st in rec["streams"] for p in st["pieces"]]
        r = 99 if any(p.get("fail") == "rounds" for p in pr) else max(p["rounds"] for p in pr)
        if len(found.setdefault((e.form, r), [])) < per:
            found[(e.form, r)].append(s)
    print("huf", dict(sorted(found.items())))


# ---------------------------------------------------------------------------------------------------------------------------- device
def enc_device_batch(g, torch):
    """the group's blocks in one device buffer, row b at base + b * stride; returns (src view, sizes or None, ctables, addresses mod 64)"""
    from oracle.oracle import fse_ctable_u32
    nb, maxn = len(g.blocks), max(len(b) for b in g.blocks)
    host = np.zeros(g.base + g.stride * (nb - 1) + maxn + 64, np.uint8)
    for i, b in enumerate(g.blocks):
        host[g.base + i * g.stride:g.base + i * g.stride + len(b)] = b
    buf = torch.from_numpy(host).cuda()
    src = buf.as_strided((nb, maxn), (g.stride, 1), g.base)
    uniform = all(len(b) == maxn for b in g.blocks)
    sizes = None if uniform else torch.tensor([len(b) for b in g.blocks], dtype=torch.int64, device="cuda")
    ct = np.zeros((nb, fse_ctable_u32(12, 255)), np.uint32)
    for i, c in enumerate(g.cts):
        ct[i, :len(c)] = c
    addrs = [(src.data_ptr() + i * g.stride) % 64 for i in range(nb)]
    return src, sizes, torch.from_numpy(ct.view(np.int32)).cuda(), addrs


def huf_device_batch(entries, torch, payloads=None):
    """(csrc, csizes, dtables, dst_sizes) of caller-table entries"""
    payloads = [e.payload for e in entries] if payloads is None else payloads
    cb = np.zeros((len(entries), max(len(p) for p in payloads) + 16), np.uint8)
    for i, p in enumerate(payloads):
        cb[i, :len(p)] = p
    dts = np.stack([np.pad(e.dt, (0, max(0, 4097 - len(e.dt))))[:4097] for e in entries]).astype(np.uint32)
    return (torch.from_numpy(cb).cuda(), torch.tensor([len(p) for p in payloads], dtype=torch.int64, device="cuda"),
            torch.from_numpy(dts.view(np.int32)).cuda(), torch.tensor([e.dst_size for e in entries], dtype=torch.int64, device="cuda"))


def device_stats(what, out_path):
    """child process (FSEHIP_LIB = an instrumented build): run the corpus through the caller-table batches and save the device's
    records -- `enc` (FSE_ENC_TIMING: rounds, nBad0, firstBad of every wave) or `huf1` / `huf4` (HPAR_STATS: repair rounds and bad links
    of every block), with the results and the bytes; `x2_1` / `x2_4`: the same record for the device entries of tests/huf_x2_par_corpus.py
    through HUF_decompress1X / 4X_usingDTable's batch.  The record is a device global that nothing zeroes: ONE decoding call per process"""
    import ctypes
    import torch
    from finitestateentropy_amd.api import FseHip
    from oracle.oracle import Checker
    hip, orc = FseHip(), Checker()
    save = {}
    if what == "enc":
        for gi, g in enumerate(enc_groups(orc)):
            src, sizes, ct, addrs = enc_device_batch(g, torch)
            dst, res = hip.fse_compress_using_ctable_batch(src, ct, max_table_log=g.tl, sizes=sizes)
            torch.cuda.synchronize()
            buf = np.zeros(4096 * 8, np.uint64)
            assert hip.lib.FSEHIP_debug_encTiming(buf.ctypes.data_as(ctypes.c_void_p)) == 0
            t = buf.reshape(4096, 8)[:len(g.blocks)]
            save["g%d_rec" % gi] = t[:, 4:7].astype(np.int64)
            save["g%d_addr" % gi] = np.array(addrs)
            save["g%d_res" % gi] = res.cpu().numpy()
            save["g%d_dst" % gi] = dst.cpu().numpy()
    else:
        form = int(what[3:])
        if what.startswith("x2_"):
            import huf_x2_par_corpus as pc
            es = [e for e in pc.build(orc.ref, orc) if e.form == form and not e.cpu_only]
            fn = hip.huf_decompress1x_using_dtable_batch if form == 1 else hip.huf_decompress4x_using_dtable_batch
        else:
            es = [e for e in huf_entries(orc) if e.form == form]
            fn = hip.huf_decompress1x1_using_dtable_batch if form == 1 else hip.huf_decompress4x1_using_dtable_batch
        c, cs, dt, ds = huf_device_batch(es, torch)
        out, res = fn(c, cs, dt, ds)
        torch.cuda.synchronize()
        buf = np.zeros(4096 * 8, np.uint64)
        assert hip.lib.FSEHIP_debug_hparStats(buf.ctypes.data_as(ctypes.c_void_p)) == 0
        save["rec"] = buf.reshape(4096, 8)[:len(es)].astype(np.int64)
        save["res"] = res.cpu().numpy()
        save["out"] = out.cpu().numpy()
    np.savez(out_path, **save)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    if len(sys.argv) > 1 and sys.argv[1] == "device":
        device_stats(sys.argv[2], sys.argv[3])
    else:
        search()
