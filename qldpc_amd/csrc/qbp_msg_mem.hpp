// Where a record's messages live in Relay-BP, layered BP and BP guided decimation, and its rows of [H | residual] in
// localized statistics decoding: the one statement of the choice between a family's two builds.  Host only, plain
// integers, no HIP: qbp.hip feeds it the handle's option and the LDS sizes as the family counts them,
// tests/_shim/msg_mem_shim.cpp builds it with a host compiler.
//
// The option (QBP_OPT_RELAY_MEM, QBP_OPT_LAYERED_MEM, QBP_OPT_GD_MEM, QBP_OPT_LSD_MEM) of a family:
//   0  the kernel keeps a record's whole state in LDS (the LDS build);
//   1  the messages (LSD: the rows) in a global workspace (the large build);
//   2  the large build where the LDS build does not fit the LDS.
// Under 0 a matrix whose LDS build passes the limit is refused; under 1 and 2 one whose large build passes it.  A
// limit of a build that is no byte count (lsd_kernel's 2048 rows) is fed as a size beyond the limit.
#pragma once

#include <stddef.h>

namespace qbp {

enum MsgMemFamily { MSG_MEM_RELAY = 0, MSG_MEM_LAYERED, MSG_MEM_GD, MSG_MEM_LSD, MSG_MEM_FAMILIES };
enum MsgMemMode { MSG_MEM_LDS = 0, MSG_MEM_LARGE = 1, MSG_MEM_AUTO = 2 };

constexpr size_t MSG_MEM_LDS_LIMIT = (size_t)160 * 1024;     // the LDS of a CU: a workgroup's state fits or is refused

struct MsgMemChoice {
    bool ok;        // false: refused, and `refuse` has written the message
    bool large;     // the build of a launch (of a refusal: the build whose size was over the limit)
};

// mode: the family's option.  lds_need, large_need: dynamic LDS bytes of the LDS build and of the large build.
// refuse(large, need): called once where the build the mode allows needs `need` > MSG_MEM_LDS_LIMIT bytes; writes the
// family's message for that build.
template <class Refuse>
MsgMemChoice msg_mem_choose(int mode, size_t lds_need, size_t large_need, Refuse&& refuse)
{
    const bool allows_large = mode != MSG_MEM_LDS;
    const size_t need = allows_large ? large_need : lds_need;
    if (need > MSG_MEM_LDS_LIMIT) {
        refuse(allows_large, need);
        return {false, allows_large};
    }
    return {true, mode == MSG_MEM_AUTO ? lds_need > MSG_MEM_LDS_LIMIT : allows_large};
}

}  // namespace qbp
