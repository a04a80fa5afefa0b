"""TEST INFRASTRUCTURE (never imported by the product): the shape tables of tests/test_gpu_w8_wide.py -- FP8 weights at 9-64 rows on the
MFMA weight-streaming forms (csrc/skinny_fp8.hip) -- kept here so that the CPU module (tests/test_w8_wide_host.py)
checks the exact designs' bound at every K the GPU module uses, and replays the slice rule.

A chunk is 256 k at MT <= 2 (M <= 32) and 128 k above; slices are cut in units of 256 k.
  K = 256     one unit: a single chunk (two at MT >= 3), no chunk in flight behind the first
  K = 512     two units: the smallest split over K (one unit per slice)
  K = 1,024   four chunks: the two-deep request ring wraps
  K = 4,096   the 7B width                     K = 11,008  43 units: an odd chunk count, uneven slices (N = 4,096: 4 slices of 10 or 11 units)
N: 8,200 and 4,104 are no multiples of the 16 rows per wave nor of the workgroup's 32-64: the last workgroup is ragged.
"""
M_TILES = (5, 9, 16, 17, 32, 33, 48, 49, 64)              # both sides of every m-tile boundary (MT = 1 .. 4), from the entry's first row count
NSPLIT = [(8200, 256), (8200, 1024), (12288, 4096)]       # (N, K): N >= 8192, whole K per wave
NSPLIT_M = M_TILES
SPLITK = [(512, 512), (4096, 4096), (4096, 11008)]        # N < 8192, N % 64 == 0, with a workspace
SPLITK_M = (9, 17, 33, 64)
NARROW = [(1536, 512), (4104, 256)]                       # no workspace | N % 64 != 0 and a single unit: the unsplit form
NARROW_M = (9, 64)
GATE = [(64, 256), (1408, 4096), (64, 11008)]             # (I, K), both layouts
GATE_M = (5, 9, 17, 64)


def slices(N, K):
    """The slice count of evo_linear_skinny_w8 with a large enough workspace (include/evo_mi355x.h): a workgroup per CU, at most 8, a
    256-k unit or more each; 1 = unsplit."""
    if N >= 8192 or N % 64:
        return 1
    return max(1, min(8, K // 256, (256 + N // 64 - 1) // (N // 64)))


def all_reductions():
    return sorted({k for _, k in NSPLIT + SPLITK + NARROW + GATE})
