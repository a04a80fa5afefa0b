"""TEST INFRASTRUCTURE (never imported by the product): the routing of the row-invariant dense launches (csrc/gemv_inv.hip,
csrc/skinny_nw.h) restated in plain Python -- which kernel form a layer shape takes, into how many slices its K is
split, and where the slices' boundaries fall in k for either chunk length.  tests/test_batch_invariant_host.py holds the restatement
against the figures section 25 quotes; the GPU modules (tests/test_gpu_rowinv_rows.py) import it for the slab count they read off a
NaN-filled workspace and for the list of shapes.

    N >= 16384 / 12288 / 8192      wide launch, 4 / 3 / 2 waves per workgroup, no split
    N <  8192                      split over K, 4 waves (2 below N = 2048), rowinv_slices(N, K) slices of whole 256-k units
    gate                           4 waves, no split
    MT = ceil(M / 16)              m tiles of 16 batch rows; a staged chunk is KC = 8 MFMA steps (256 k) at MT <= 2, 4 steps (128 k) above
"""

WIDE_N = 8192
UNIT = 256                                      # the k unit of SLICE256
ROUTES = ("wide2", "wide3", "wide4", "split2", "split4", "gate")

# the five layers of the 7B step: (N, K) of the linear entry, and the gate's (I, K)
LINEAR_7B = [(12288, 4096), (4096, 4096), (4096, 11008), (512, 4096)]
GATE_7B = (11008, 4096)
# the smallest shape of each route: the three tests/test_gpu_rowinv.py lacks, and its own two wide ones (2 and 4 waves)
LINEAR_SMALL = [(12288, 256), (512, 2304), (4096, 2816), (8192, 256), (16384, 256)]
EVERY_M = list(range(1, 65))


def mt_of(M):
    """m tiles of 16 rows (for_mt, csrc/skinny_nw.h)."""
    assert 1 <= M <= 64
    return (M + 15) // 16


def kc_of(mt):
    """MFMA steps of 32 k per staged chunk."""
    return 8 if mt <= 2 else 4


def waves(N):
    """Waves per workgroup of the linear entry, by N alone."""
    if N >= 16384:
        return 4
    if N >= 12288:
        return 3
    if N >= WIDE_N:
        return 2
    return 2 if N < 2048 else 4


def rowinv_slices(N, K):
    """Slices of a narrow layer's K (0: the wide launch, which does not split): a workgroup per CU where the layer allows it, at most 8,
    at least one 256-k unit each."""
    if N >= WIDE_N:
        return 0
    groups = N // (32 if N < 2048 else 64)
    return min((256 + groups - 1) // groups, K // UNIT, 8)


def route(N, K):
    """The launch form of evo_linear_rowinv_bf16 at (N, K): one of ROUTES."""
    assert K % UNIT == 0 and N % 64 == 0
    return ("wide" if N >= WIDE_N else "split") + str(waves(N))


def boundaries(K, slices, kc, unit256):
    """The slices' boundaries in k, [0, ..., K] (slices + 1 entries), as skinny_nw_kernel cuts them at a chunk length of `kc` MFMA steps:
    in units of 256 k (SLICE256, the invariant entry) or in chunks (the default SPLITK)."""
    assert K % UNIT == 0 and kc in (4, 8) and 1 <= slices
    chunk = 32 * kc
    n_chunk_all = K // chunk
    per_unit = 8 // kc                                               # chunks per 256 k
    n_cut, cut = (n_chunk_all // per_unit, per_unit) if unit256 else (n_chunk_all, 1)
    return [n_cut * y // slices * cut * chunk for y in range(slices + 1)]


def slice_units(N, K):
    """256-k units per slice of the invariant entry at (N, K)."""
    s = rowinv_slices(N, K)
    b = boundaries(K, s, 8, True)
    return [(b[i + 1] - b[i]) // UNIT for i in range(s)]


def all_cuts(k_max=11008):
    """Every (K, slices) the entry can meet: K a multiple of 256 up to k_max, 1 .. min(8, K / 256) slices."""
    return [(K, s) for K in range(UNIT, k_max + 1, UNIT) for s in range(1, min(8, K // UNIT) + 1)]


def reached(linear_cases, gate_ms):
    """{(route, MT)} of (N, K, M) triples of the linear entry and of the row counts the gate is run at."""
    got = {(route(N, K), mt_of(M)) for N, K, M in linear_cases}
    return got | {("gate", mt_of(M)) for M in gate_ms}
