"""The numpy model of the tensor digest and the gate (include/fsehip.h, "tensor digests and checked deltas"): a pure numpy XXH32 that runs many
streams of one length side by side (the 64 lane streams of every full tile of a tensor in one go), the tile digest, the tensor digest, and the
gate as a function of integers.  Nothing here calls the library; test_planes_digest_model.py pins the XXH32 to the oracle's."""
import numpy as np

T = 32768
S0, S1 = 0, 0x9E3779B1
P1, P2, P3, P4, P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
GENERIC, SRC_WRONG, CORRUPT = -1, -3, -4
M32 = np.uint64(0xFFFFFFFF)


def _rotl(x, r):
    return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & M32


def _mul(x, p):                                             # (32 x 32 bits in uint64: no overflow)
    return (x * np.uint64(p)) & M32


def xxh32_rows(rows, seed):
    """XXH32 of every row of a 2-D uint8 array (all rows have one length) -> uint64 array of values below 2**32"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    m, n = rows.shape
    seed = np.uint64(seed)
    nst = n // 16
    if nst:
        w = rows[:, :16 * nst].reshape(m, nst, 4, 4).astype(np.uint64)
        w = w[..., 0] | (w[..., 1] << np.uint64(8)) | (w[..., 2] << np.uint64(16)) | (w[..., 3] << np.uint64(24))        # little-endian dwords
        v = np.empty((m, 4), np.uint64)
        v[:] = [(int(seed) + P1 + P2) & 0xFFFFFFFF, (int(seed) + P2) & 0xFFFFFFFF, int(seed), (int(seed) - P1) & 0xFFFFFFFF]
        for s in range(nst):
            v = _mul(_rotl((v + _mul(w[:, s], P2)) & M32, 13), P1)
        h = (_rotl(v[:, 0], 1) + _rotl(v[:, 1], 7) + _rotl(v[:, 2], 12) + _rotl(v[:, 3], 18)) & M32
    else:
        h = np.full(m, (int(seed) + P5) & 0xFFFFFFFF, np.uint64)
    h = (h + np.uint64(n)) & M32
    at = 16 * nst
    while at + 4 <= n:
        b = rows[:, at:at + 4].astype(np.uint64)
        x = b[:, 0] | (b[:, 1] << np.uint64(8)) | (b[:, 2] << np.uint64(16)) | (b[:, 3] << np.uint64(24))
        h = _mul(_rotl((h + _mul(x, P3)) & M32, 17), P4)
        at += 4
    while at < n:
        h = _mul(_rotl((h + _mul(rows[:, at].astype(np.uint64), P5)) & M32, 11), P1)
        at += 1
    h ^= h >> np.uint64(15)
    h = _mul(h, P2)
    h ^= h >> np.uint64(13)
    h = _mul(h, P3)
    h ^= h >> np.uint64(16)
    return h


def xxh32(data, seed=0):
    return int(xxh32_rows(np.asarray(data, np.uint8).reshape(1, -1), seed)[0])


def _fold(h):
    """h: (tiles, 64) lane hashes -> (tiles, 2) lo and hi"""
    H = h.astype("<u4").view(np.uint8).reshape(len(h), 256)
    return np.stack([xxh32_rows(H, S0), xxh32_rows(H, S1)], axis=1)


def lane_streams(tile):
    """the 64 lane streams of one tile by the definition: pieces of 16 bytes, piece q to lane q mod 64, in rising q"""
    tile = np.asarray(tile, np.uint8)
    pieces = [tile[k:k + 16] for k in range(0, len(tile), 16)]
    return [np.concatenate(pieces[l::64]) if pieces[l::64] else np.zeros(0, np.uint8) for l in range(64)]


def tile_digest(tile):
    """one tile, lane by lane, straight from the definition -> (lo, hi)"""
    assert len(tile) <= T
    h = np.array([xxh32(s, S0) for s in lane_streams(tile)], np.uint64)
    lo, hi = _fold(h.reshape(1, 64))[0]
    return int(lo), int(hi)


def tile_digests(data):
    """every tile of a tensor -> (nt, 2): the full tiles vectorised over tiles and lanes, the partial one by tile_digest"""
    data = np.asarray(data, np.uint8)
    full = len(data) // T
    out = np.zeros(((len(data) + T - 1) // T, 2), np.uint64)
    if full:
        # byte 1024 r + 16 l + j of a tile is byte 16 r + j of lane l's stream
        streams = data[:full * T].reshape(full, T // 1024, 64, 16).transpose(0, 2, 1, 3).reshape(full * 64, T // 64)
        out[:full] = _fold(xxh32_rows(streams, S0).reshape(full, 64))
    if len(data) > full * T:
        out[full] = tile_digest(data[full * T:])
    return out


def tensor_digest(data):
    data = np.asarray(data, np.uint8)
    A = np.concatenate([tile_digests(data).astype("<u4").reshape(-1).view(np.uint8), np.array([len(data)], "<u8").view(np.uint8)])
    return xxh32(A, S0) | (xxh32(A, S1) << 32)


def digest_batch(flat, offsets, capacity=None):
    """FSEHIP_tensor_digest_dbatch -> (digests, results)"""
    capacity = len(flat) if capacity is None else capacity
    digs, res = [], []
    for a, b in zip(offsets[:-1], offsets[1:]):
        ok = a <= b <= capacity
        digs.append(tensor_digest(flat[a:b]) if ok else 0)
        res.append(b - a if ok else GENERIC)
    return digs, res


def gate_cases():
    """(name, F, E, digests, digest results, expected, frame_first) -- the cases both gate tests run: all pass, all fail, alternating, a failing
    first and a failing last tensor, a digest error against a mismatch, E = 1, 2 and 4, a segFirst with unequal counts, values beyond nFrames"""
    rng = np.random.default_rng(77)
    cases = []
    for E in (1, 2, 4):
        nT = 5
        F = [int(x) for x in np.concatenate([[3], 3 + np.cumsum(rng.integers(8, 90, nT * E))])]
        want = [int(x) for x in rng.integers(0, 1 << 63, nT, dtype=np.int64)]
        sizes = [int(x) for x in rng.integers(0, 5000, nT)]
        for name, bad in (("pass", ()), ("fail", range(nT)), ("alternating", (0, 2, 4)), ("first", (0,)), ("last", (nT - 1,))):
            got = [w ^ (1 << (7 * i)) if i in bad else w for i, w in enumerate(want)]
            cases.append(("%s E=%d" % (name, E), F, E, got, sizes, want, None))
        res = list(sizes)
        res[1] = GENERIC                                      # a digest error on a matching digest, a mismatch beside it
        cases.append(("error and mismatch E=%d" % E, F, E, [want[0], want[1], want[2] ^ 1, want[3], want[4]], res, want, None))
        # segments: unequal counts per plane, a tensor without frames, and a tail beyond nFrames that is clamped
        counts = [int(x) for x in rng.integers(1, 4, nT * E)]
        counts[E:2 * E] = [0] * E
        first = [int(x) for x in np.concatenate([[0], np.cumsum(counts)])]
        nF = first[-1]
        Fs = [int(x) for x in np.concatenate([[0], np.cumsum(rng.integers(8, 40, nF))])]
        for name, bad in (("pass", ()), ("fail", range(nT)), ("alternating", (1, 3)), ("first", (0,)), ("last", (nT - 1,))):
            got = [w ^ 2 if i in bad else w for i, w in enumerate(want)]
            cases.append(("seg %s E=%d" % (name, E), Fs, E, got, sizes, want, first))
        beyond = [f if k < 3 * E else f + 100 for k, f in enumerate(first)]
        cases.append(("seg clamped E=%d" % E, Fs, E, [w ^ 4 if i in (2, 4) else w for i, w in enumerate(want)], sizes, want, beyond))
    return cases


def gate(F, E, digests, digest_results, expected, frame_first=None):
    """FSEHIP_tensor_gate_dbatch on integers -> (G, gate results)"""
    nF, nT = len(F) - 1, len(expected)
    if frame_first is None:
        assert nF == nT * E
        first = [i * E for i in range(nT + 1)]
    else:
        assert len(frame_first) == nT * E + 1
        first = [min(int(frame_first[i * E]), nF) for i in range(nT + 1)]
    G, R = [int(x) for x in F], []
    for i in range(nT):
        ok = digest_results[i] >= 0 and digests[i] == expected[i]
        R.append(digest_results[i] if ok or digest_results[i] < 0 else CORRUPT)
        if not ok:
            for q in range(first[i], first[i + 1]):
                G[q] = int(F[first[i + 1]])
    return G, R
