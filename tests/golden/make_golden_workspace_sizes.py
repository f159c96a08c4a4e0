"""Generate tests/golden/workspace_sizes.json: what every *_workspaceSize export of libfsehip.so returns on a grid of arguments, and
FSEHIP_FSE_optimalTableLog on a grid of in-contract arguments.  Both are arithmetic on the arguments: no GPU is needed.

The fixture pins the numbers of the library it was generated from; tests/test_workspace_sizes.py holds every later library to them (a
caller that sized its workspace once keeps working).  It was generated from the commit before the C ABI file was split by layer:

    python tests/golden/make_golden_workspace_sizes.py [path/to/libfsehip.so]

Regenerate it only when a workspace is meant to change size."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")

N_BLOCKS = (0, 1, 2, 63, 64, 65, 131071, 131072, 131073, 1000000)
LOGS = (0, 5, 9, 11, 12, 13)
# name -> argument tuples; the batch calls take (nBlocks) or (nBlocks, tableLog / maxLog)
BY_BLOCKS = ("HUF_compress_batch", "HUF_decompress_batch", "FSE_buildCTable_batch", "HUF_buildCTable_batch", "HUF_readDTableX1_batch",
             "HUF_readDTableX2_batch", "compact_batch", "FSE_compressU16_batch", "FSE_decompressU16_batch")
BY_BLOCKS_AND_LOG = ("FSE_compress_batch", "FSE_decompress_batch", "FSE_buildDTable_batch", "FSE_buildDTable_fromNorm_batch")
FRAMES = (1, 3)
FRAME_BLOCKS = (1, 65, 131073)
BY_FRAME = {      # the device frame calls: (nFrames, maxTotalBlocks[, blockSizeId, codec]) or (nFrames)
    "frame_compress_dbatch": [(f, b, i, c) for f in FRAMES for b in FRAME_BLOCKS for i in (0, 5) for c in (0, 1)],
    "frame_compress_packed_dbatch": [(f, b, i, c) for f in FRAMES for b in FRAME_BLOCKS for i in (0, 5) for c in (0, 1)],
    "frame_decompress_dbatch": [(f, b) for f in FRAMES for b in FRAME_BLOCKS],
    "frame_decompress_packed_dbatch": [(f, b) for f in FRAMES for b in FRAME_BLOCKS],
    "frame_plan_dbatch": [(f,) for f in FRAMES + (1000,)],
}
# FSE_optimalTableLog(maxTableLog, srcSize, maxSymbolValue) inside its contract: srcSize > 1, maxSymbolValue >= 1
OTL_GRID = [(tl, n, msv) for tl in (0, 5, 9, 11, 12, 13) for n in (2, 3, 17, 255, 256, 1000, 4096, 65536, 131072, 1 << 20) for msv in (1, 2, 15, 127, 255)]


def grid():
    g = {}
    for name in BY_BLOCKS:
        g[name] = [(n,) for n in N_BLOCKS]
    for name in BY_BLOCKS_AND_LOG:
        g[name] = [(n, tl) for n in N_BLOCKS for tl in LOGS]
    g.update(BY_FRAME)
    return g


def call(lib, name, args):
    fn = getattr(lib, "FSEHIP_%s_workspaceSize" % name)
    fn.restype = ctypes.c_size_t
    fn.argtypes = ([ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_int] if len(args) == 4 else
                   [ctypes.c_size_t, ctypes.c_uint] if name in BY_BLOCKS_AND_LOG else [ctypes.c_size_t] * len(args))
    return int(fn(*args))


def optimal_table_log(lib, tl, n, msv):
    fn = lib.FSEHIP_FSE_optimalTableLog
    fn.restype = ctypes.c_uint
    fn.argtypes = [ctypes.c_uint, ctypes.c_size_t, ctypes.c_uint]
    return int(fn(tl, n, msv))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "finitestateentropy_amd", "csrc", "libfsehip.so")
    lib = ctypes.CDLL(path)
    sizes = {name: [[list(a), call(lib, name, a)] for a in argsets] for name, argsets in sorted(grid().items())}
    otl = [[list(a), optimal_table_log(lib, *a)] for a in OTL_GRID]
    with open(OUT, "w") as f:
        json.dump({"workspaceSize": sizes, "optimalTableLog": otl}, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, sum(len(v) for v in sizes.values()), "sizes,", len(otl), "table logs")


if __name__ == "__main__":
    main()
