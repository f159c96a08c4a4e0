"""Contents and oracle frames shared by the device-frame tests (test_frame_dev_plan.py, test_gpu_frame_device.py): built once per
session, never changed.  At 1 KB blocks (block-size id 0) the contents produce all three block kinds and every header form."""
import numpy as np

BSID = 0
_CACHE = {}


def contents(oracle):
    """[(name, bytes)] in batch order"""
    if "contents" not in _CACHE:
        rng = np.random.default_rng(17)
        P = lambda p, n, seed: oracle.probagen_batch(p, 1, n, seed)[0]
        _CACHE["contents"] = [
            ("empty", np.zeros(0, np.uint8)),
            ("one_byte", np.array([0x5A], np.uint8)),
            ("four_syms_15", rng.integers(0, 4, 15, dtype=np.uint8)),
            ("four_syms_16", rng.integers(0, 4, 16, dtype=np.uint8)),
            ("four_syms_17", rng.integers(0, 4, 17, dtype=np.uint8)),
            ("p14_1024", P(14, 1024, 31)),
            ("p14_1025", P(14, 1025, 32)),
            ("p80_3077", P(80, 3 * 1024 + 5, 33)),
            ("noise_2500", rng.integers(0, 256, 2500, dtype=np.uint8)),
            ("rle_blocks", np.concatenate([np.full(1024, 9, np.uint8), np.full(1024, 200, np.uint8), np.full(123, 1, np.uint8)])),
            ("mixed", np.concatenate([P(20, 1024, 34), rng.integers(0, 256, 1024, dtype=np.uint8), np.full(1024, 5, np.uint8), P(50, 700, 35)])),
            ("empty_again", np.zeros(0, np.uint8)),
            ("p14_1100_blocks", P(14, 1100 * 1024 + 7, 36)),
        ]
    return _CACHE["contents"]


def frames(oracle, codec, bsid=BSID):
    """the oracle's frame of every content: [bytes]"""
    key = ("frames", codec, bsid)
    if key not in _CACHE:
        out = []
        for _, data in contents(oracle):
            r, buf = oracle.frame_compress(data, bsid, codec)
            out.append(buf[:r].copy())
        _CACHE[key] = out
    return _CACHE[key]


def header_forms(frame):
    """{(block type, full-size flag)} of an intact frame's blocks (format: programs/fileio.c:266-285)"""
    bs = 1024 << int(frame[4])
    forms, ip = set(), 5
    while (frame[ip] >> 6) != 3:
        b0 = int(frame[ip]); ip += 1
        bt, full, r = b0 >> 6, bool(b0 & 0x20), bs
        if not full:
            r = (int(frame[ip]) << 8) + int(frame[ip + 1]); ip += 2
        if bt == 0:
            c = (int(frame[ip]) << 8) + int(frame[ip + 1]); ip += 2
        else:
            c = r if bt == 1 else 1
        forms.add((bt, full)); ip += c
    return forms


def block_count(n, bsid=BSID):
    bs = 1024 << bsid
    return (n + bs - 1) // bs


def bound(n, bsid=BSID):
    """FSEHIP_frame_compressBound, restated: magic + id, the content, 5 header bytes per block, the end mark"""
    return 5 + n + 5 * block_count(n, bsid) + 3


def big_frames(oracle):
    """a 150000-byte P14 content at block-size ids 2 and 5, both codecs: [(content, frame)]"""
    if "big" not in _CACHE:
        data = oracle.probagen_batch(14, 1, 150000, 9)[0]
        out = []
        for bsid in (2, 5):
            for codec in (0, 1):
                r, buf = oracle.frame_compress(data, bsid, codec)
                out.append((data, buf[:r].copy()))
        _CACHE["big"] = out
    return _CACHE["big"]


def crafted_short_block(oracle, codec):
    """A frame whose first block announces a full 1 KB block (flag 0x20) but carries the payload of a 700-byte one, followed by a real
    full block: -> (a | b, frame).  With FSE payloads the first block regenerates 700 bytes into a capacity of 1024, so everything behind
    it lands 324 bytes lower than the headers announce; with Huff0 payloads the announced size is the exact size and the block fails."""
    key = ("crafted", codec)
    if key not in _CACHE:
        a = oracle.probagen_batch(14, 1, 700, 3)[0]
        b = oracle.probagen_batch(14, 1, 1024, 4)[0]
        ra, fa = oracle.frame_compress(a, 0, codec)
        rb, fb = oracle.frame_compress(b, 0, codec)
        fa, fb = fa[:ra], fb[:rb]
        assert fa[5] == 0x00 and fb[5] == 0x20, "a: compressed, partial; b: compressed, full"
        csa = (int(fa[8]) << 8) + int(fa[9]); pa = fa[10:10 + csa]
        csb = (int(fb[6]) << 8) + int(fb[7]); pb = fb[8:8 + csb]
        assert 10 + csa + 3 == ra and 8 + csb + 3 == rb
        ab = np.concatenate([a, b])
        crc = (oracle.xxh32(ab) >> 5) & 0x3FFFFF
        frame = np.concatenate([fa[:5], np.array([0x20, csa >> 8, csa & 0xFF], np.uint8), pa, np.array([0x20, csb >> 8, csb & 0xFF], np.uint8), pb,
                                np.array([0xC0 | (crc >> 16), (crc >> 8) & 0xFF, crc & 0xFF], np.uint8)]).astype(np.uint8)
        _CACHE[key] = (ab, frame)
    return _CACHE[key]
