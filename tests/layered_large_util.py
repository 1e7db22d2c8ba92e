"""Helpers of tests/test_layered_large_cpu.py and tests/test_gpu_layered_large.py: the launch arithmetic of layered BP's
large build (QBP_OPT_LAYERED_MEM; layered_large_lds_bytes of qbp_layered.hpp, layered_slots and the grid of
layered_launch in qbp.hip) restated in Python beside record_kernel_util's restatement of the LDS build -- usable
without a GPU."""
import record_kernel_util as ru

MEM_LDS, MEM_LARGE, MEM_AUTO = 0, 1, 2       # values of QBP_OPT_LAYERED_MEM


def slot_words(m):
    return (ru.LAYERED_SLOT_HEAD + ((m + 31) >> 5) + 1) & ~1


def layered_large_lds_bytes(m, n, S, tables):
    """numpy's tables (sum-product), V[S][n] doubles, the workgroup words and S times the slot words."""
    return (ru.np_lds_bytes() if tables else 0) + 8 * S * n + 4 * (ru.LAYERED_WG_WORDS + S * slot_words(m))


def lds_bytes(sh, S, tables, large):
    return layered_large_lds_bytes(sh.m, sh.n, S, tables) if large else ru.layered_lds_bytes(sh.m, sh.n, sh.E, S, tables)


def layered_slots(sh, max_width, B, tables, opt_slots, large):
    """ru.layered_slots with the build's own LDS figure."""
    S = opt_slots
    if S <= 0:
        S = max(1, min(ru.LAYERED_MAX_SLOTS, ru.LAYERED_THREADS // max(1, max_width)))
        while S > 1 and lds_bytes(sh, S, tables, large) > 80 * 1024:
            S -= 1
    while S > 1 and lds_bytes(sh, S, tables, large) > ru.LDS_LIMIT:
        S -= 1
    return max(1, min(S, B))


def layered_grid(sh, S, B, num_cu, tables, large, blocks_per_cu=0):
    per_cu = max(1, min(5, ru.LDS_LIMIT // lds_bytes(sh, S, tables, large)))
    if blocks_per_cu > 0:
        per_cu = blocks_per_cu
    return max(1, min(-(-B // S), num_cu * per_cu))


def auto_is_large(sh):
    """QBP_OPT_LAYERED_MEM = 2: the large build where the single-slot LDS build, counted with the tables, passes 160 KiB."""
    return ru.layered_lds_bytes(sh.m, sh.n, sh.E, 1, True) > ru.LDS_LIMIT


def n_limit(m):
    """The largest n qbp_layered_configure accepts under modes 1 and 2 with m checks."""
    return (ru.LDS_LIMIT - layered_large_lds_bytes(m, 0, 1, True)) // 8
