"""Frames shared by the frame-inspection tests (test_frame_inspect.py, test_gpu_frame_inspect.py): the oracle's frames of frame_dev_corpus, the
two crafted frames, and every short one of them truncated at every byte and with single bits flipped -- built once per session, never
changed -- beside a Python restatement of FSEHIP_frame_inspect (include/fsehip.h; format: programs/fileio.c:266-285)."""
import numpy as np

import frame_dev_corpus as fdc

GENERIC, SRC_WRONG, CORRUPT = 1, 3, 4
MAGIC = {0x183E2309: 0, 0x183E3309: 1}
SHORT = 6000            # base frames below this many bytes get the damaged variants
FLIPS = 400
_CACHE = {}


def inspect(frame):
    """FSEHIP_FrameInfo of a frame as a dict, and the call's return value: -> (result, info)"""
    f = np.asarray(frame, dtype=np.uint8)
    n = len(f)
    info = dict(content_bound=0, n_blocks=0, status=0, checksum22=0, codec=0, block_size_id=0, reserved=bytes(6))

    def done(status=0):
        info["status"] = status
        return ((1 << 64) - status if status else info["content_bound"]), info

    if n < 8:
        return done(SRC_WRONG)
    magic = int(f[0]) | int(f[1]) << 8 | int(f[2]) << 16 | int(f[3]) << 24
    if magic not in MAGIC or f[4] > 6:
        return done(GENERIC)
    info["codec"], info["block_size_id"] = MAGIC[magic], int(f[4])
    bs = 1024 << int(f[4])
    ip = 5
    while True:
        if ip >= n:
            return done(SRC_WRONG)
        b0 = int(f[ip]); ip += 1
        bt, r = b0 >> 6, bs
        if bt == 3:
            if ip + 2 > n:
                return done(SRC_WRONG)
            info["checksum22"] = int(f[ip + 1]) + (int(f[ip]) << 8) + ((b0 & 0x3F) << 16)
            return done()
        if not b0 & 0x20:
            if ip + 2 > n:
                return done(SRC_WRONG)
            r = (int(f[ip]) << 8) + int(f[ip + 1]); ip += 2
        if bt == 0:
            if ip + 2 > n:
                return done(SRC_WRONG)
            c = (int(f[ip]) << 8) + int(f[ip + 1]); ip += 2
        else:
            c = r if bt == 1 else 1
        if ip + c > n:
            return done(SRC_WRONG)
        if r > bs:
            return done(CORRUPT)
        info["content_bound"] += r; info["n_blocks"] += 1
        ip += c


def bases(oracle):
    """[(name, frame, content, block-size id or None)]: id None = not written by the oracle's writer (the crafted frames)"""
    if "bases" not in _CACHE:
        out = []
        for codec in (0, 1):
            for (name, data), f in zip(fdc.contents(oracle), fdc.frames(oracle, codec)):
                out.append(("%s/c%d" % (name, codec), f, data, fdc.BSID))
        for k, (data, f) in enumerate(fdc.big_frames(oracle)):
            out.append(("big%d" % k, f, data, int(f[4])))
        for codec in (0, 1):
            ab, f = fdc.crafted_short_block(oracle, codec)
            out.append(("crafted/c%d" % codec, f, ab, None))
        _CACHE["bases"] = out
    return _CACHE["bases"]


def corpus(oracle):
    """[(kind, base index, frame)], kind in base / cut / flip / head: the base frames, then for every base frame shorter than SHORT bytes every
    truncation, FLIPS single-bit flips at positions drawn from default_rng(5), and every bit of bytes 4 to 11"""
    if "corpus" not in _CACHE:
        base = bases(oracle)
        out = [("base", b, f) for b, (_, f, _, _) in enumerate(base)]
        rng = np.random.default_rng(5)
        for b, (_, f, _, _) in enumerate(base):
            if len(f) >= SHORT:
                continue
            out += [("cut", b, f[:cut].copy()) for cut in range(len(f))]
            for bit in rng.integers(0, 8 * len(f), FLIPS):
                g = f.copy(); g[int(bit) >> 3] ^= 1 << (int(bit) & 7); out.append(("flip", b, g))
            for bit in range(8 * 4, min(8 * 12, 8 * len(f))):
                g = f.copy(); g[bit >> 3] ^= 1 << (bit & 7); out.append(("head", b, g))
        _CACHE["corpus"] = out
    return _CACHE["corpus"]


def inspected(oracle):
    """the restatement's (result, info) of every frame of corpus(), in its order"""
    if "inspected" not in _CACHE:
        _CACHE["inspected"] = [inspect(f) for _, _, f in corpus(oracle)]
    return _CACHE["inspected"]
