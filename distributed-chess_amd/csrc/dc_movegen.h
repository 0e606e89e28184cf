// dc_movegen.h -- launch wrappers of the legal-move list kernels (dc_movegen.hip).
#pragma once
#include "dc_kernels.h"

namespace dc {

// One lane per position, 256 positions per block; a batch of at most one
// block takes the fused kernel (count, scan and emit in one launch).
constexpr u32 kLegalBlock = 256;

// status bits (include/dchess.h DC_ST_*)
enum : u32 { ST_CHECK = 1, ST_NO_MOVES = 2, ST_DEAD = 4 };

// n <= kLegalBlock.  offsets[0..n] = exclusive prefix of the counts, status[i]
// (optional), *total = offsets[n]; moves (optional) is filled only when the
// total fits `cap`.  done / seq: the completion flag of dc_moves.hip's
// publish_done (pinned I/O), or nullptr.
hipError_t launch_legal_small(hipStream_t st, u32 rules, const DevPos* pos, u32 n, u32* offsets, uint8_t* status,
                              uint16_t* moves, u32 cap, u64* total, u32* done, u32 seq);
// Any n: offsets[i] = exclusive prefix of the counts inside i's block,
// block_sum[b] = the block's count.
hipError_t launch_legal_count(hipStream_t st, u32 rules, const DevPos* pos, u32 n, u32* offsets, uint8_t* status,
                              u32* block_sum);
// One workgroup: block_base = exclusive prefix of block_sum (its low 32 bits),
// *offsets_n = the total's low 32 bits, *total = the 64-bit total.
hipError_t launch_legal_scan(hipStream_t st, const u32* block_sum, u32 n_blocks, u32* block_base, u32* offsets_n,
                             u64* total);
// offsets[i] += block_base[i / kLegalBlock] (the sizing call; the fill call's
// emit kernel does it itself).
hipError_t launch_legal_fixup(hipStream_t st, u32* offsets, u32 n, const u32* block_base);
// Writes every position's moves at its final offset and the final offsets;
// nothing at or past moves[limit].
hipError_t launch_legal_emit(hipStream_t st, u32 rules, const DevPos* pos, u32 n, u32* offsets, const u32* block_sum,
                             const u32* block_base, uint16_t* moves, u32 limit);

}  // namespace dc
