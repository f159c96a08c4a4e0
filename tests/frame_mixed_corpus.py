"""Contents, oracle frames and the choice rule shared by the mixed packed writer's tests (test_frame_mixed_model.py, test_gpu_frame_mixed.py):
built once per session, never changed.  Plain Python and numpy, never the library.  The contents are small -- at block-size id 0 (1 KB
blocks) a few KB make several blocks, at id 5 every content is one block -- and cover: nothing, one and two bytes; RLE blocks; raw blocks;
a strongly and a mildly skewed source around the block size; and the first 16 KB of the four planes of the issue's table (the planes of a
bf16 tensor and of its XOR with the tensor one training step earlier), on which the two coders disagree in both directions."""
import numpy as np

import planes_corpus as pc
import planes_delta_corpus as pdc

BSIDS = (0, 5)
TOLERANCES = (0, 20, 50, 1000)
GENERIC, TOO_SMALL = -1, -2
_CACHE = {}


def expected_choice(F, H, tol):
    """the codec of FSEHIP_CODECS_CHOOSE for a frame whose FSE frame takes F and whose Huff0 frame takes H (negative: an error), and its result:
    Huff0 iff H * 1000 <= F * (1000 + tol) in integers; an error on one side takes the other; on both, codec 0 and F's error"""
    F, H = int(F), int(H)
    if H < 0:
        return 0, F
    if F < 0:
        return 1, H
    return (1, H) if H * 1000 <= F * (1000 + int(tol)) else (0, F)


def update_planes():
    """the four planes of the issue's table, whole: [(name, bytes)] -- planes 0 and 1 of the new tensor, planes 0 and 1 of new XOR old"""
    if "planes" not in _CACHE:
        old, new = pdc.bf16_update_pair()
        plain, delta = pc.planes_of(new, 2), pc.planes_of(old ^ new, 2)
        _CACHE["planes"] = [("plain_plane0", np.ascontiguousarray(plain[0])), ("plain_plane1", np.ascontiguousarray(plain[1])),
                            ("delta_plane0", np.ascontiguousarray(delta[0])), ("delta_plane1", np.ascontiguousarray(delta[1]))]
    return _CACHE["planes"]


def contents(oracle):
    """[(name, bytes)] in batch order"""
    if "contents" not in _CACHE:
        rng = np.random.default_rng(41)
        P = lambda p, n, seed: oracle.probagen_batch(p, 1, n, seed)[0]
        _CACHE["contents"] = [
            ("empty", np.zeros(0, np.uint8)),
            ("one_byte", np.array([0x5A], np.uint8)),
            ("two_bytes", np.array([3, 200], np.uint8)),
            ("rle_3000", np.full(3000, 77, np.uint8)),
            ("noise_2500", rng.integers(0, 256, 2500, dtype=np.uint8)),
            ("p80_1024", P(80, 1024, 51)),
            ("p80_1025", P(80, 1025, 52)),
            ("p80_4097", P(80, 4097, 53)),
            ("p14_5000", P(14, 5000, 54)),
        ] + [(name + "_16k", data[:16384].copy()) for name, data in update_planes()]
    return _CACHE["contents"]


def frames(oracle, bsid, codec):
    """the oracle's frame of every content: [bytes]"""
    key = ("frames", bsid, codec)
    if key not in _CACHE:
        out = []
        for _, data in contents(oracle):
            r, buf = oracle.frame_compress(data, bsid, codec)
            out.append(buf[:r].copy())
        _CACHE[key] = out
    return _CACHE[key]


def choices(oracle, bsid, tol):
    """[codec] the rule gives over the corpus from the oracle's frame sizes"""
    return [expected_choice(len(f), len(h), tol)[0] for f, h in zip(frames(oracle, bsid, 0), frames(oracle, bsid, 1))]


def block_count(n, bsid):
    bs = 1024 << bsid
    return (n + bs - 1) // bs
