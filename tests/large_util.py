"""Helpers of tests/test_{relay,layered,gd}_large_cpu.py, tests/test_gpu_{relay,layered,gd}_large.py and
tests/test_msg_mem_cpu.py: the launch arithmetic of the large builds of Relay-BP, layered BP and BP guided decimation
(QBP_OPT_RELAY_MEM, QBP_OPT_LAYERED_MEM, QBP_OPT_GD_MEM; the *_large_lds_bytes of the kernel headers and the grids of
relay_launch, layered_launch and gd_launch in qbp.hip) restated in Python beside record_kernel_util's restatement of
the LDS builds -- usable without a GPU."""
import record_kernel_util as ru

MEM_LDS, MEM_LARGE, MEM_AUTO = 0, 1, 2       # values of the three options (qbp_msg_mem.hpp)


def first_n_beyond_the_limit(large_lds_bytes):
    """The smallest n whose large build, ``large_lds_bytes(n)`` bytes, does not fit 160 KiB."""
    n = 1
    while large_lds_bytes(n) <= ru.LDS_LIMIT:
        n += 1
    return n


# ---- Relay-BP ------------------------------------------------------------------------------------------------------
RELAY_LARGE_WAVES_PER_CU = 24                # 6 wavefronts per SIMD at the large build's registers (LDS build: 7, 28)


def relay_lds_words(m):
    return (8 + 3 * ((m + 31) >> 5) + 1) & ~1


def relay_large_lds_bytes(m, n, records=False):
    """V[n] doubles, the bookkeeping words, and (records build) a byte per variable."""
    return 8 * n + 4 * relay_lds_words(m) + (((n + 7) & ~7) if records else 0)


def relay_large_grid(sh, B, num_cu):
    lds = relay_large_lds_bytes(sh.m, sh.n)
    per_cu = max(1, min(RELAY_LARGE_WAVES_PER_CU // (ru.relay_threads(sh) // 64), ru.LDS_LIMIT // lds))
    return max(1, min(B, num_cu * per_cu))


# ---- layered BP ----------------------------------------------------------------------------------------------------
def layered_slot_words(m):
    return (ru.LAYERED_SLOT_HEAD + ((m + 31) >> 5) + 1) & ~1


def layered_large_lds_bytes(m, n, S, tables):
    """numpy's tables (sum-product), V[S][n] doubles, the workgroup words and S times the slot words."""
    return (ru.np_lds_bytes() if tables else 0) + 8 * S * n + 4 * (ru.LAYERED_WG_WORDS + S * layered_slot_words(m))


def layered_build_lds(sh, S, tables, large):
    return layered_large_lds_bytes(sh.m, sh.n, S, tables) if large else ru.layered_lds_bytes(sh.m, sh.n, sh.E, S, tables)


def layered_slots(sh, max_width, B, tables, opt_slots, large):
    """ru.layered_slots with the build's own LDS figure."""
    S = opt_slots
    if S <= 0:
        S = max(1, min(ru.LAYERED_MAX_SLOTS, ru.LAYERED_THREADS // max(1, max_width)))
        while S > 1 and layered_build_lds(sh, S, tables, large) > 80 * 1024:
            S -= 1
    while S > 1 and layered_build_lds(sh, S, tables, large) > ru.LDS_LIMIT:
        S -= 1
    return max(1, min(S, B))


def layered_grid(sh, S, B, num_cu, tables, large, blocks_per_cu=0):
    per_cu = max(1, min(5, ru.LDS_LIMIT // layered_build_lds(sh, S, tables, large)))
    if blocks_per_cu > 0:
        per_cu = blocks_per_cu
    return max(1, min(-(-B // S), num_cu * per_cu))


def layered_auto_is_large(sh):
    """QBP_OPT_LAYERED_MEM = 2: the large build where the single-slot LDS build, counted with the tables, passes 160 KiB."""
    return ru.layered_lds_bytes(sh.m, sh.n, sh.E, 1, True) > ru.LDS_LIMIT


def layered_n_limit(m):
    """The largest n qbp_layered_configure accepts under modes 1 and 2 with m checks."""
    return (ru.LDS_LIMIT - layered_large_lds_bytes(m, 0, 1, True)) // 8


# ---- BP guided decimation ------------------------------------------------------------------------------------------
# wavefronts per CU at the large build's registers: min-sum 6 per SIMD (80 registers), sum-product 4 (109); the LDS
# build has 7 and 5 (28 and 20 per CU)
GD_LARGE_WAVES_PER_CU = {False: 24, True: 16}   # by `sum_product`


def gd_large_lds_words(m, n):
    """The head words, syndrome bits, two parity buffers and two n-bit maps (decimated, sign), to an even count."""
    mw, nw = (m + 31) >> 5, (n + 31) >> 5
    return (ru.GD_HEAD_WORDS + 3 * mw + 2 * nw + 1) & ~1


def gd_large_lds_bytes(m, n, tables):
    """(sum-product) numpy's tables, V[n] doubles, the words."""
    return (ru.np_lds_bytes() if tables else 0) + 8 * n + 4 * gd_large_lds_words(m, n)


def gd_large_grid(sh, B, num_cu, sum_product, blocks_per_cu=0):
    lds = gd_large_lds_bytes(sh.m, sh.n, sum_product)
    per_cu = max(1, min(GD_LARGE_WAVES_PER_CU[bool(sum_product)] // (ru.gd_threads(sh) // 64), ru.LDS_LIMIT // lds))
    if blocks_per_cu > 0:
        per_cu = blocks_per_cu
    return max(1, min(B, num_cu * per_cu))


def gd_first_rounds_beyond_the_lds_build(tables):
    """The first round count of the [[72,12,6]] phenomenological matrix whose LDS build passes 160 KiB."""
    return ru.largest_rounds(lambda sh: ru.gd_lds_bytes(sh.m, sh.n, sh.E, tables)) + 1
