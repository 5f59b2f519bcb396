// vdb_compact_plan.h — the host arithmetic of vdb_index_remove (vdb_api.cpp) and of its kernels
// (vdb_compact.hip): mask words, chunk bounds and the extents of the vacated tail.  Plain C++
// with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/remove_plan_check.cpp).
#pragma once
#include <stdint.h>

namespace vdb {

// Words of the remove bitmap one workgroup of the keep-count scan handles (256 threads x 4).
constexpr int64_t kScanWgWords = 1024;
// Most bytes of the gather's scratch rows (as an add's staging, vdb_index_add).
constexpr int64_t kRemoveScratchBytes = 256ll << 20;
// Bytes per scratch row beside its Dp floats: nrm64 (8), inv32, sq32, rinit32 (4 each).
constexpr int64_t kRowScalarBytes = 20;

inline int64_t remove_mask_words(int64_t count) { return (count + 31) / 32; }

// The bits of mask word w that name rows below count.
inline uint32_t remove_valid_bits(int64_t w, int64_t count) {
    const int64_t left = count - w * 32;
    if (left >= 32) return 0xFFFFFFFFu;
    if (left <= 0) return 0u;
    return (1u << left) - 1u;
}

// Mask words per chunk: knob_rows ("remove_chunk", 0 = by bytes) rounded down to whole words, at
// least one word, at most what kRemoveScratchBytes holds.
inline int64_t remove_chunk_words(int64_t knob_rows, int Dp) {
    const int64_t per_row = (int64_t)Dp * 4 + kRowScalarBytes;
    int64_t rows = kRemoveScratchBytes / per_row;
    if (knob_rows > 0 && knob_rows < rows) rows = knob_rows;
    return rows / 32 > 0 ? rows / 32 : 1;
}

// Chunks cover the words [first_word, n_words) in ascending order, chunk_words each.
inline int64_t remove_n_chunks(int64_t first_word, int64_t n_words, int64_t chunk_words) {
    return first_word >= n_words ? 0 : (n_words - first_word + chunk_words - 1) / chunk_words;
}
struct RemoveChunk {
    int64_t w0, w1;  // source words [w0, w1): rows [32 w0, min(32 w1, count))
};
inline RemoveChunk remove_chunk(int64_t first_word, int64_t n_words, int64_t chunk_words, int64_t c) {
    RemoveChunk k;
    k.w0 = first_word + c * chunk_words;
    k.w1 = k.w0 + chunk_words < n_words ? k.w0 + chunk_words : n_words;
    return k;
}

// What is rebuilt and zeroed once the rows have moved (rows; 128 = a super tile of the tiled
// copies, whose bytes are contiguous per super tile):
//   rebuild0            first row whose candidate copies are rebuilt (its word's first row)
//   [rebuild0, new_count)   the int8 copy, row by row
//   [rebuild0, tiles_end)   the tiled split / fp32 copy, whole tiles: rows past new_count are
//                           zero in X by then, so their tiles come out zero
//   [new_count, rowz_end)   the int8 copy's rows zeroed one by one (the partial super tile)
//   [tiles_end, st_end)     whole super tiles of both tiled copies zeroed by memset
//   [new_count, old_count)  the row-major arrays zeroed by memset
struct RemoveTail {
    int64_t rebuild0, tiles_end, rowz_end, st_end;
};
inline RemoveTail remove_tail(int64_t first_word, int64_t new_count, int64_t old_count) {
    RemoveTail t;
    t.rebuild0 = first_word * 32;
    t.tiles_end = (new_count + 127) / 128 * 128;
    t.st_end = (old_count + 127) / 128 * 128;
    t.rowz_end = old_count < t.tiles_end ? old_count : t.tiles_end;
    return t;
}

}  // namespace vdb
