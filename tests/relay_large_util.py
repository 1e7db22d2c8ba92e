"""Helpers of tests/test_relay_large_cpu.py and tests/test_gpu_relay_large.py: the launch arithmetic of Relay-BP's large
build (QBP_OPT_RELAY_MEM; relay_large_lds_bytes of qbp_relay.hpp and the grid of relay_launch in qbp.hip) restated in
Python beside record_kernel_util's restatement of the LDS build -- usable without a GPU."""
import record_kernel_util as ru

MEM_LDS, MEM_LARGE, MEM_AUTO = 0, 1, 2       # values of QBP_OPT_RELAY_MEM
LARGE_WAVES_PER_CU = 24                      # 6 wavefronts per SIMD at the large build's registers (LDS build: 7, 28)


def relay_lds_words(m):
    return (8 + 3 * ((m + 31) >> 5) + 1) & ~1


def relay_large_lds_bytes(m, n, records=False):
    """V[n] doubles, the bookkeeping words, and (records build) a byte per variable."""
    return 8 * n + 4 * relay_lds_words(m) + (((n + 7) & ~7) if records else 0)


def relay_large_grid(sh, B, num_cu):
    lds = relay_large_lds_bytes(sh.m, sh.n)
    per_cu = max(1, min(LARGE_WAVES_PER_CU // (ru.relay_threads(sh) // 64), ru.LDS_LIMIT // lds))
    return max(1, min(B, num_cu * per_cu))


def first_n_beyond_the_limit(m, records=False):
    """The smallest n whose large build does not fit 160 KiB with m checks."""
    n = 1
    while relay_large_lds_bytes(m, n, records) <= ru.LDS_LIMIT:
        n += 1
    return n
