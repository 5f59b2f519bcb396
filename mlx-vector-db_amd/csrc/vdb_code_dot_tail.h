// vdb_code_dot_tail.h: what the two forms of the code-dot search share on the device (vdb_code_dot.hip,
// vdb_code_dot_mfma.hip): the load of eight query values and the write of one result slot from a list
// entry.
#pragma once
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_code_dot_plan.h"

namespace vdb {

// Eight int8 values from p as one word, value i in byte i.  A query row starts a multiple of 8 bytes
// past `queries`, so one test of that pointer (`aligned`, uniform) decides for every load of a launch.
__device__ __forceinline__ uint64_t cd_load8(const int8_t* p, bool aligned) {
    if (aligned) return *reinterpret_cast<const uint64_t*>(p);
    uint64_t v = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) v |= (uint64_t)(uint8_t)p[i] << (8 * i);
    return v;
}

// key = the list key of the entry (the score less `bias`, exact in fp32), r = the row or the sentinel
// ("no result": INT32_MIN / -1).
__device__ __forceinline__ void code_dot_write(const CodeDotArgs& a, int b, int e, float key, int32_t bias, uint32_t r) {
    const bool valid = r != 0xFFFFFFFFu;
    const size_t o = (size_t)b * a.k + e;
    a.out_s[o] = valid ? (int32_t)key + bias : kCdNoScore;
    a.out_i[o] = valid ? (int64_t)((uint64_t)r + (uint64_t)a.index_offset) : (int64_t)-1;
}

}  // namespace vdb
