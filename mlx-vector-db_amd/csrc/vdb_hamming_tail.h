// vdb_hamming_tail.h: what the two forms of the Hamming search share on the device (vdb_hamming.hip,
// vdb_hamming_mfma.hip): the write of one result slot from a list entry.
#pragma once
#include "vdb_common.h"
#include "vdb_internal.h"

namespace vdb {

// key = the negated distance, r = the row or the sentinel ("no result": -1 / -1).
__device__ __forceinline__ void hamming_write(const HammingArgs& a, int b, int e, float key, uint32_t r) {
    const bool valid = r != 0xFFFFFFFFu;
    const size_t o = (size_t)b * a.k + e;
    a.out_d[o] = valid ? (int32_t)(-key) : -1;
    a.out_i[o] = valid ? (int64_t)((uint64_t)r + (uint64_t)a.index_offset) : (int64_t)-1;
}

}  // namespace vdb
