// Host build of qbp_msg_mem.hpp for tests/test_msg_mem_cpu.py: the choice between a family's LDS build and its large
// build, with a refusal formatter that records what it was told.
#include <stddef.h>

#include "../../qldpc_amd/csrc/qbp_msg_mem.hpp"

extern "C" {

unsigned long long msg_mem_limit() { return qbp::MSG_MEM_LDS_LIMIT; }

// out[0]: ok; out[1]: large; out[2]: calls of the formatter; out[3]: the build it was told (1 large), out[4]: the bytes
void msg_mem_choose(int mode, unsigned long long lds_need, unsigned long long large_need, unsigned long long* out)
{
    out[2] = out[3] = out[4] = 0;
    const qbp::MsgMemChoice c =
        qbp::msg_mem_choose(mode, (size_t)lds_need, (size_t)large_need, [out](bool large_build, size_t need) {
            ++out[2];
            out[3] = large_build;
            out[4] = need;
        });
    out[0] = c.ok;
    out[1] = c.large;
}

}  // extern "C"
