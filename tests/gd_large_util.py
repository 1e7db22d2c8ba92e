"""Helpers of tests/test_gd_large_cpu.py and tests/test_gpu_gd_large.py: the launch arithmetic of BP guided decimation's
large build (QBP_OPT_GD_MEM; gd_large_lds_bytes of qbp_gd.hpp and the grid of gd_launch in qbp.hip) restated in Python
beside record_kernel_util's restatement of the LDS build -- usable without a GPU."""
import record_kernel_util as ru

MEM_LDS, MEM_LARGE, MEM_AUTO = 0, 1, 2       # values of QBP_OPT_GD_MEM
# wavefronts per CU at the large build's registers: min-sum 6 per SIMD (80 registers), sum-product 4 (109); the LDS
# build has 7 and 5 (28 and 20 per CU)
LARGE_WAVES_PER_CU = {False: 24, True: 16}   # by `sum_product`


def gd_large_lds_words(m, n):
    """The head words, syndrome bits, two parity buffers and two n-bit maps (decimated, sign), to an even count."""
    mw, nw = (m + 31) >> 5, (n + 31) >> 5
    return (ru.GD_HEAD_WORDS + 3 * mw + 2 * nw + 1) & ~1


def gd_large_lds_bytes(m, n, tables):
    """(sum-product) numpy's tables, V[n] doubles, the words."""
    return (ru.np_lds_bytes() if tables else 0) + 8 * n + 4 * gd_large_lds_words(m, n)


def gd_large_grid(sh, B, num_cu, sum_product, blocks_per_cu=0):
    lds = gd_large_lds_bytes(sh.m, sh.n, sum_product)
    per_cu = max(1, min(LARGE_WAVES_PER_CU[bool(sum_product)] // (ru.gd_threads(sh) // 64), ru.LDS_LIMIT // lds))
    if blocks_per_cu > 0:
        per_cu = blocks_per_cu
    return max(1, min(B, num_cu * per_cu))


def first_n_beyond_the_limit(m, tables):
    """The smallest n whose large build does not fit 160 KiB with m checks."""
    n = 1
    while gd_large_lds_bytes(m, n, tables) <= ru.LDS_LIMIT:
        n += 1
    return n


def first_rounds_beyond_the_lds_build(tables):
    """The first round count of the [[72,12,6]] phenomenological matrix whose LDS build passes 160 KiB."""
    return ru.largest_rounds(lambda sh: ru.gd_lds_bytes(sh.m, sh.n, sh.E, tables)) + 1
