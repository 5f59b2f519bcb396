// vdb_jaccard_tail.h: what the two forms of the Jaccard search share on the device (vdb_jaccard.hip,
// vdb_jaccard_mfma.hip): the write of one result slot.  The ranking keys identify a ratio, not its
// numerator and denominator, so the slot's i and u are counted again from the winner's row and the
// query: k rows of W words per query, next to nothing beside the scan.
#pragma once
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_jaccard_plan.h"

namespace vdb {

// r = the row of query b's slot e, or the sentinel ("no result": -1 / -1 / -1).
__device__ __forceinline__ void jaccard_write(const JaccardArgs& a, int b, int e, uint32_t r) {
    const size_t o = (size_t)b * a.k + e;
    if (r == 0xFFFFFFFFu) {
        a.out_n[o] = -1;
        a.out_u[o] = -1;
        a.out_i[o] = (int64_t)-1;
        return;
    }
    const uint8_t* q = a.queries + (size_t)b * a.n_bytes;
    int i = 0, xp = 0, qp = 0;
    for (int w = 0; w < a.W; ++w) {
        const uint64_t xw = a.codes[ham_word_index((int64_t)r, w, a.W)];
        const uint64_t qw = ham_word_of(q, a.n_bytes, w);
        i += __popcll(xw & qw);
        xp += __popcll(xw);
        qp += __popcll(qw);
    }
    a.out_n[o] = i;
    a.out_u[o] = qp + xp - i;
    a.out_i[o] = (int64_t)((uint64_t)r + (uint64_t)a.index_offset);
}

}  // namespace vdb
