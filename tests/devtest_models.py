"""Models of the device building blocks that tests/device/devtest.hip wraps (dev_common.h, wave_glue.h, planes_dev.h, bitreader.h, wb_scan_excl and
wb_bytesum of fse_wave_build.h), written from each operation's definition on numpy arrays and Python integers, not from the headers' code:
prefix sums are cumulative sums per group in unbounded integers reduced mod 2^32 / 2^64, zigzag works on signed Python-sized integers, the
(de)interleavers are a reshape and a transpose, the bit reader reads a big integer from its top.  tests/test_devtest_model.py pins the models to
hand-written cases; tests/test_gpu_devtest.py puts the kernels against them.  Every comparison is exact."""
import numpy as np

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
WIDTHS, ELEMS, STRIDES = (8, 16, 32, 64), (1, 2, 4, 8), (2, 3, 4, 5, 6, 7, 8)
OPS = ("add", "max", "min")                              # the b of group_scan_incl / group_reduce
IDENT = {"add": 0, "max": 0, "min": M32}
LANES = np.arange(64)

# ---- the table of operations: (name, a, b) -> (dwords in, dwords out) per work item; a == -1: a run-time argument ----
BR_STREAM, BR_STEPS, FS_CELLS, FS_STEPS = 32, 64, 32, 32


def table():
    t = {}
    for W in WIDTHS:
        for b in range(3):
            t[("group_scan_incl", W, b)] = (1, 1)
            t[("group_reduce", W, b)] = (1, 1)
        for name in ("group_last", "wg_sum", "wg_max", "wg_min", "wg_any", "wg_scan_excl", "wg_suffix_min_excl"):
            t[(name, W, 0)] = (1, 1)
        for name in ("group_scan_incl_add64", "group_last64", "wg_sum64", "wg_scan_excl64"):
            t[(name, W, 0)] = (2, 2)
    for D in (1, 2, 4, 8, 16, 32):
        t[("lane_xor", D, 0)] = (1, 1)
    t[("lane_xor_any", -1, 0)] = (1, 1)
    for name in ("wave_max_u32", "wave_max_i32", "wb_bytesum"):
        t[(name, 0, 0)] = (1, 1)
    t[("wb_scan_excl", 0, 0)] = (1, 2)
    t[("pp_add16x2", 0, 0)] = t[("pp_add8x4", 0, 0)] = (2, 1)
    for E in ELEMS:
        t[("pl_zz", E, 0)] = t[("pl_unzz", E, 0)] = (4, 2)
        for b in (0, 1):
            t[("pl_sub4", E, b)] = (8, 4)
            t[("pp_prev", E, b)] = (1, 4 * E)
        t[("pl_deinterleave", E, 0)] = t[("pl_interleave", E, 0)] = (4 * E, 4 * E)
        t[("pp_prefix", E, 0)] = (4 * E, 4 * E + 2)
        t[("pp_carry", E, 0)] = (4 * E + 2, 4 * E)
        for S in STRIDES:
            t[("ps_prev", E, S)] = t[("ps_prev", E, S + 16)] = (1, 4 * E)
        t[("ps_unpack", E, 0)] = (4 * E, 32)
        t[("ps_pack", E, 0)] = (32, 4 * E)
        t[("pl_share", E, 0)] = (9, 10)
    for S in STRIDES:
        for T in (4, 8):
            t[("ps_rotate", S, T)] = (2 * S + 1, 2 * S)
    t[("pl_size", 0, 0)] = t[("pl_start", 0, 0)] = (4, 2)
    t[("pl_find", -1, 0)] = (2, 4)
    t[("pl_last_le", -1, 0)] = (2, 2)
    t[("bitreader", 0, 0)] = (2 + BR_STREAM // 4 + BR_STEPS, 6 + 5 * BR_STEPS)
    t[("fse_step", -1, 0)] = (3 + BR_STREAM // 4 + FS_CELLS, 2 + 5 * FS_STEPS)
    return t


# ---- cross-lane: v is (waves, 64); a group of W lanes is lanes g W .. g W + W - 1 ----
def _grp(v, W):
    v = np.asarray(v)
    return v.astype(object).reshape(v.shape[0], 64 // W, W)


def _out(x, bits):
    x = x.reshape(x.shape[0], 64)
    return (x % (1 << bits)).astype(np.uint64 if bits == 64 else np.uint32)


def scan_incl(v, W, op, bits=32):
    """lane i of a group: op over lanes first .. i of its group (sums mod 2^bits)"""
    g = _grp(v, W)
    r = {"add": np.cumsum(g, axis=2), "max": np.maximum.accumulate(g, axis=2), "min": np.minimum.accumulate(g, axis=2)}[op]
    return _out(r, bits)


def group_last(v, W, bits=32):
    """every lane: the value of its group's last lane"""
    g = _grp(v, W)
    return _out(np.repeat(g[:, :, -1:], W, axis=2), bits)


def reduce(v, W, op, bits=32):
    """every lane: op over all lanes of its group"""
    g = _grp(v, W)
    r = {"add": g.sum(axis=2, keepdims=True), "max": g.max(axis=2, keepdims=True), "min": g.min(axis=2, keepdims=True)}[op]
    return _out(np.repeat(r, W, axis=2), bits)


def scan_excl(v, W, bits=32):
    """lane i: the sum of the lanes of its group in front of it"""
    g = _grp(v, W)
    return _out(np.cumsum(g, axis=2) - g, bits)


def lane_xor(v, d):
    return np.asarray(v)[:, LANES ^ d]


def wave_max_i32(v):
    s = np.asarray(v, dtype=np.uint32).view(np.int32)
    return np.repeat(s.max(axis=1, keepdims=True), 64, axis=1).view(np.uint32)


def group_any(p, W):
    g = (np.asarray(p) != 0).reshape(-1, 64 // W, W)
    return np.repeat(g.any(axis=2, keepdims=True), W, axis=2).reshape(-1, 64).astype(np.uint32)


def suffix_min_excl(v, W):
    """lane i: the minimum of the lanes of its group above it; 0xFFFFFFFF for the group's last lane"""
    g = _grp(v, W)
    r = np.full(g.shape, M32, dtype=object)
    for i in range(W - 1):
        r[:, :, i] = g[:, :, i + 1:].min(axis=2)
    return _out(r, 32)


def bytesum(v):
    return np.asarray(v, dtype=np.uint32).reshape(-1, 1).view(np.uint8).astype(np.uint32).sum(axis=1).reshape(np.shape(v))


# ---- plane arithmetic ----
def zz_int(t, b, E):
    """zigzag of the signed difference t - b of two E-byte elements: 0, -1, 1, -2, .. -> 0, 1, 2, 3, .."""
    w = 8 * E
    d = (t - b) % (1 << w)
    s = d - (1 << w) if d >> (w - 1) else d
    return 2 * s if s >= 0 else -2 * s - 1


def unzz_int(z, b, E):
    s = z // 2 if z % 2 == 0 else -(z + 1) // 2
    return (b + s) % (1 << (8 * E))


def zz(t, b, E):
    """zz_int on arrays: int64 arithmetic below 8 bytes, Python integers at 8"""
    if E == 8:
        return np.array([zz_int(int(x), int(y), 8) for x, y in zip(np.ravel(t), np.ravel(b))], dtype=np.uint64).reshape(np.shape(t))
    w = 8 * E
    d = (np.asarray(t).astype(np.int64) - np.asarray(b).astype(np.int64)) % (1 << w)
    s = np.where(d >> (w - 1), d - (1 << w), d)
    return np.where(s >= 0, 2 * s, -2 * s - 1).astype(np.uint64)


def unzz(z, b, E):
    if E == 8:
        return np.array([unzz_int(int(x), int(y), 8) for x, y in zip(np.ravel(z), np.ravel(b))], dtype=np.uint64).reshape(np.shape(z))
    z, b = np.asarray(z).astype(np.int64), np.asarray(b).astype(np.int64)
    s = np.where(z % 2 == 0, z // 2, -((z + 1) // 2))
    return ((b + s) % (1 << (8 * E))).astype(np.uint64)


def elems(raw, E):
    """bytes (.., 16 E) -> little-endian elements (.., 16)"""
    return np.ascontiguousarray(raw, dtype=np.uint8).view("<u%d" % E)


def as_bytes(x, E):
    return np.ascontiguousarray(np.asarray(x).astype("<u%d" % E)).view(np.uint8)


def sub4(w, b, E, inv):
    """w, b: bytes (n, 16) holding whole elements -> zigzag(w - b), or (inv) b + unzigzag(w), element by element"""
    f = unzz if inv else zz
    return as_bytes(f(elems(w, E), elems(b, E), E), E)


def deinterleave(chunk, E):
    """(n, 16 E) bytes of 16 elements -> (n, E, 16): plane p holds byte p of each element"""
    return np.ascontiguousarray(np.asarray(chunk, dtype=np.uint8).reshape(-1, 16, E).transpose(0, 2, 1))


def interleave(planes, E):
    return np.ascontiguousarray(np.asarray(planes, dtype=np.uint8).reshape(-1, E, 16).transpose(0, 2, 1)).reshape(-1, 16 * E)


def prev(buf, off, E, S, run_start):
    """the 16 elements in front of those of the chunk at buf[off:], S elements back; the first S are 0 where the chunk starts a run"""
    buf = np.asarray(buf, dtype=np.uint8)
    out = np.zeros(16 * E, dtype=np.uint8)
    if run_start:
        out[S * E:] = buf[off:off + (16 - S) * E]
    else:
        out[:] = buf[off - S * E:off + (16 - S) * E]
    return out


def add_lanes(x, y, E):
    """x + y on the E-byte fields of dwords"""
    a, b = np.asarray(x, dtype=np.uint32).reshape(-1, 1).view("<u%d" % E), np.asarray(y, dtype=np.uint32).reshape(-1, 1).view("<u%d" % E)
    return (a + b).astype("<u%d" % E).view(np.uint32).reshape(np.shape(x))


def prefix(chunk, E):
    """(n, 16 E) bytes -> the inclusive prefix sums of the 16 elements mod 2^(8 E) as bytes, and the last one"""
    e = elems(chunk, E).astype(object if E == 8 else np.uint64)        # (16 elements below 2^32 sum to less than 2^36)
    c = np.cumsum(e, axis=1) % (1 << (8 * E))
    return as_bytes(c.astype(np.uint64), E), c[:, -1].astype(np.uint64)


def carry(chunk, c, E):
    """every element plus c, mod 2^(8 E)"""
    if E == 8:
        e, c = elems(chunk, E).astype(object), np.asarray(c).astype(object)
    else:
        e, c = elems(chunk, E).astype(np.uint64), np.asarray(c, dtype=np.uint64) % np.uint64(1 << (8 * E))
    return as_bytes(((e + c.reshape(-1, 1)) % (1 << (8 * E))).astype(np.uint64), E)


def rotate(v, r, S):
    """out[k] = v[(k + r) mod S]"""
    v = np.asarray(v)
    return np.stack([v[np.arange(len(v)), (k + np.asarray(r)) % S] for k in range(S)], axis=1)


# ---- index logic ----
def pl_size(n, p, E):
    """bytes of plane p of a tensor of n bytes: the k < n with k mod E == p"""
    return (n - 1 - p) // E + 1 if n > p else 0          # p, p + E, .. up to the last one below n


def pl_start(n, p, E):
    return sum(pl_size(n, q, E) for q in range(p))


def share_range(s0, n, lo, T, E):
    """[e0, e1): the elements (element e starts at flat byte s0 + e E, there are ceil(n / E)) whose first byte lies in [lo, lo + T)"""
    first = s0 + np.arange(-(-n // E), dtype=np.int64) * E
    hit = np.nonzero((first >= lo) & (first < lo + T))[0]
    return (int(hit[0]), int(hit[-1]) + 1) if len(hit) else None


def last_le(keys, q):
    """the largest j with keys[j] <= q for keys that do not decrease; 0 where there is none"""
    hit = [j for j, k in enumerate(keys) if k <= q]
    return hit[-1] if hit else 0


def find(S, w, tile_log):
    """the largest i with floor(S[i] / T) + i <= w, or None"""
    hit = [i for i, s in enumerate(S) if (s >> tile_log) + i <= w]
    return hit[-1] if hit else None


# ---- the LIFO bit reader (the format: the stream is read from its end; the highest set bit of the last byte marks the end) ----
UNFINISHED, END_OF_BUFFER, COMPLETED, OVERFLOW = 0, 1, 2, 3
ERRORS = {"GENERIC": 1, "srcSize_wrong": 3, "corruption_detected": 4}      # include/fsehip.h: init returns (size_t)-code


def init_return(m):
    """what init returns for the model m: the stream's size, or the error as (size_t)-code"""
    return m.n if m.status is None else (1 << 64) - ERRORS[m.status]


class BitModel:
    """The stream as one integer V (byte 0 lowest); P = the number of bits still to read, the next read takes bits [P - nb, P).  The reader's
    window is the 8 bytes at `at` (the whole stream, zero-extended, below 8 bytes) with `used` bits consumed from its top: P = 8 at + 64 - used."""

    def __init__(self, stream):
        self.n = len(stream)
        self.V = int.from_bytes(bytes(stream), "little")
        self.ok = self.n >= 1 and stream[-1] != 0
        self.status = None
        if self.n < 1:
            self.status = "srcSize_wrong"
        elif stream[-1] == 0:
            self.status = "GENERIC" if self.n >= 8 else "corruption_detected"
        self.at = max(self.n - 8, 0)
        self.used = 0
        if self.ok:
            P = 8 * (self.n - 1) + int(stream[-1]).bit_length() - 1
            self.used = 8 * self.at + 64 - P

    @property
    def P(self):
        return 8 * self.at + 64 - self.used

    @property
    def win(self):
        return (self.V >> (8 * self.at)) & M64

    def read(self, nb):
        """the next nb bits; None once the window is exhausted (the reader's value is then unspecified)"""
        v = (self.V >> (self.P - nb)) & ((1 << nb) - 1) if self.used + nb <= 64 else None
        self.used += nb
        return v

    def reload(self):
        """move the window down by the whole bytes consumed, as far as the stream's start allows"""
        if self.used > 64:
            return OVERFLOW
        if self.at >= 8:
            self.at -= self.used // 8
            self.used %= 8
            return UNFINISHED
        if self.at == 0:
            return END_OF_BUFFER if self.used < 64 else COMPLETED
        nbytes, res = self.used // 8, UNFINISHED
        if nbytes > self.at:
            nbytes, res = self.at, END_OF_BUFFER
        self.at -= nbytes
        self.used -= 8 * nbytes
        return res


def run_script(stream, steps):
    """steps: ("read" | "fast" | "reload", nb) -> (model after init, [(value or status, at, used, win)])"""
    m = BitModel(stream)
    rows = [(None, m.at, m.used, m.win)]
    for op, nb in steps:
        v = m.reload() if op == "reload" else m.read(nb)
        rows.append((v, m.at, m.used, m.win))
    return m, rows


def fse_steps(stream, cells, state, steps):
    """cell = nbBits << 24 | symbol << 16 | newState base: the symbol of the state's cell, then state = base + nbBits fresh bits; a reload behind
    every step -> [(symbol, state, status, at, used)]"""
    m = BitModel(stream)
    rows = []
    for _ in range(steps):
        c = cells[state]
        low = m.read(c >> 24)
        state = (c & 0xFFFF) + low
        rows.append(((c >> 16) & 0xFF, state, m.reload(), m.at, m.used))
    return rows
