/*
 * dchess.h -- C ABI of the MI355X chess state-transition engine.
 *
 * Drop-in boundary for the reference's move-validation call surface
 * (dorlneylon/distributed-chess @ 2024-10-22, core/src/chess.rs):
 *
 *   reference (Rust inherent methods)                      replaced by
 *   -----------------------------------------------------  ------------------------------
 *   GameState::validate_move(&self,&Position,&Position)    dc_validate_batch (n >= 1)
 *       core/src/chess.rs:82-98, called from
 *       core/src/consensus/hotstuff.rs:138 (is_valid_tx)
 *   GameState::apply_move(&mut self,Position,Position)     dc_apply_batch
 *       core/src/chess.rs:43-80, called from
 *       core/src/consensus/hotstuff.rs:52 (commit_block)
 *   GameState::new / Board::new                            dc_startpos
 *       core/src/chess.rs:12-20, :383-434
 *   proto GameState.board (core/proto/game.proto:7-40)     dc_pos_from_cells / dc_pos_to_cells
 *   Position{x,y} pairs (core/proto/query.proto:46-49)     dc_move_pack
 *   AppError::InternalGameError(String)                    dc_verdict_message
 *       core/src/errors.rs:9, strings chess.rs:104-121
 *   (absent in the reference)                  dc_replay, dc_gen_games, dc_perft
 *
 * Conventions
 *   - Every call returns int status: DC_SUCCESS (0) or a negative DC_E* code.
 *     Nothing panics or aborts across the ABI; a rejected move is a verdict
 *     (data), never an error.
 *   - Buffers are caller-owned HOST memory unless the name ends in _device,
 *     in which case they are device pointers on the context's device.
 *   - A dc_ctx is bound to one device and one HIP stream and is not thread-safe:
 *     use one context per thread.  Host-memory calls block until results are
 *     on the host (wrap them in tokio::task::spawn_blocking on the Rust side).
 *   - All arithmetic is integer; results are bit-exact with the reference.
 *
 * There is no CPU fallback behind this ABI: if no gfx950 device is present,
 * dc_ctx_create fails with DC_ENODEV.
 */
#ifndef DCHESS_H
#define DCHESS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status */
#define DC_SUCCESS 0
#define DC_EINVAL (-1)       /* bad argument (null pointer, bad cell, bad turn, bad FEN) */
#define DC_EHIP (-2)         /* HIP runtime failure */
#define DC_ENOMEM (-3)       /* device or host allocation failed */
#define DC_ENODEV (-4)       /* no usable gfx950 device */
#define DC_ERCCL (-5)        /* RCCL failure (dc_multi_*) */
#define DC_EUNSUPPORTED (-6) /* request outside what this build supports */

/* ----------------------------------------------------------------- verdicts
 * In the reference's check order (chess.rs:82-125), with OOR first because the
 * reference indexes both squares before any rule check (chess.rs:85,92). */
#define DC_V_OK 0
#define DC_V_NO_PIECE 1   /* "No piece at the source location"     chess.rs:104-106 */
#define DC_V_WRONG_TURN 2 /* "It's not this piece's turn to move"  chess.rs:113-115 */
#define DC_V_ILLEGAL 3    /* "Invalid move for the piece"          chess.rs:119-121 */
#define DC_V_OOR 4        /* coordinate >= 8: the reference panics (chess.rs:85,92) */

/* ------------------------------------------------------------------- rules */
#define DC_RULES_REF 0  /* bit-exact with core/src/chess.rs (geometry only) */
#define DC_RULES_FIDE 1 /* standard chess: castling, en passant, promotion, no self-check */

/* ---------------------------------------------------------------- position
 * Quad-bitboard: square s = 8*x + y (x = row, 0 = White's back rank; y = column),
 * the 4-bit nibble of square s is (bb[0]>>s &1) | (bb[1]>>s &1)<<1 | ... :
 *   bb[0]            : 1 = black piece
 *   bb[1],bb[2],bb[3]: bits 0,1,2 of the kind code
 *                      P=1 N=2 K=3 OTHER=4 B=5 R=6 Q=7   (0 = empty square)
 * so  diagonal sliders = bb[3]&bb[1], orthogonal sliders = bb[3]&bb[2].
 * OTHER is a piece whose kind string is not one of "P","N","B","R","Q","K":
 * it never moves (chess.rs:210) but blocks and can be captured.
 * stm: side to move, 0 White / 1 Black (proto Color, game.proto:20-23).
 * castle (FIDE): bit0 White O-O, bit1 White O-O-O, bit2 Black O-O, bit3 Black O-O-O.
 * ep (FIDE): en-passant target square or -1.  Both are ignored under DC_RULES_REF. */
typedef struct dc_pos {
  uint64_t bb[4];
  uint8_t stm;
  uint8_t castle;
  int8_t ep;
  uint8_t reserved0;
  uint32_t reserved1;
} dc_pos; /* 40 bytes */

/* -------------------------------------------------------------------- moves
 * uint16: from | to<<6 | promo<<12, promo 0 none, 1 N, 2 B, 3 R, 4 Q (FIDE only;
 * ignored under REF, where a Position pair carries no promotion).
 * Bit 15 (DC_MOVE_OOR) marks a move with a coordinate >= 8: verdict DC_V_OOR.
 * 0xFFFF (DC_MOVE_NONE) pads replay games that ended: skipped, not counted. */
#define DC_MOVE_OOR 0x8000u
#define DC_MOVE_NONE 0xFFFFu

/* Cell encoding of dc_pos_from_cells / dc_pos_to_cells (the proto board flattened):
 * cells[8*x+y] = -1 for an empty cell, else color*8 + kind with
 * kind 0 P, 1 N, 2 B, 3 R, 4 Q, 5 K, 6 OTHER; color 0 White, 1 Black. */
#define DC_CELL_EMPTY (-1)

typedef struct dc_ctx dc_ctx;

typedef struct dc_replay_stats {
  uint64_t validated;  /* non-sentinel plies (accepted + rejected) */
  uint64_t accepted;
  uint64_t rejected;
  uint64_t digest_sum; /* sum of per-game final-state digests (mod 2^64) */
  uint64_t digest_xor; /* xor of per-game final-state digests */
} dc_replay_stats;

typedef struct dc_kernel_stats {
  uint64_t launches;  /* launches of the kernel since the last reset */
  double total_ms;    /* summed HIP-event duration of those launches */
  uint64_t units;     /* work units those launches processed (leaves, moves, ...) */
} dc_kernel_stats;

/* ------------------------------------------------------------------ context */
int dc_ctx_create(int device, dc_ctx** out);
int dc_ctx_destroy(dc_ctx* ctx);
int dc_ctx_device(const dc_ctx* ctx);
/* hipStream_t of the context, as void* (so callers can order their own work). */
void* dc_ctx_stream(dc_ctx* ctx);
const char* dc_strerror(int status);
/* Exact reference error text for verdicts 1..3 (chess.rs:104-121); "" for OK. */
const char* dc_verdict_message(uint8_t verdict);
/* 100, or 101 from the library that has the per-game-start calls
 * (dc_replay_outcome_starts, dc_replay_san_starts, dc_san_resolve_starts). */
int dc_version(void);

/* Per-kernel HIP-event timing (enable, read, reset).  Kernel names:
 * "validate", "replay", "gen_games", "expand_count", "expand_write", "count1", "count2",
 * "legal_count" (units: positions), "legal_emit" (units: moves); beside them
 * "legal_scan", "legal_fixup" and, for batches of at most 256, "legal_small";
 * "replay_outcome" and "replay_san" (units: moves consumed);
 * "san_resolve" (units: tokens other than DC_SAN_TOKEN_NONE);
 * "replay_outcome_starts", "replay_san_starts" and "san_resolve_starts": the
 * per-game-start forms of those three, same units. */
int dc_ctx_set_profiling(dc_ctx* ctx, int enable);
int dc_ctx_kernel_stats(dc_ctx* ctx, const char* kernel, dc_kernel_stats* out);
int dc_ctx_reset_stats(dc_ctx* ctx);

/* Device memory owned by the caller, on the context's device (for the *_device
 * entry points, so a host program needs no other GPU runtime). */
int dc_device_alloc(dc_ctx* ctx, size_t bytes, void** d_ptr);
int dc_device_free(dc_ctx* ctx, void* d_ptr);
int dc_memcpy_h2d(dc_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int dc_memcpy_d2h(dc_ctx* ctx, void* dst, const void* d_src, size_t bytes);

/* ----------------------------------------------------------------- adapters
 * Pure data-layout conversions on the host (no rule evaluation). */
int dc_startpos(dc_pos* out); /* Board::new + turn White, chess.rs:12-20,383-434 */
int dc_pos_from_cells(const int8_t cells[64], uint8_t turn, dc_pos* out);
int dc_pos_to_cells(const dc_pos* pos, int8_t cells[64], uint8_t* turn);
int dc_pos_from_fen(const char* fen, dc_pos* out);
/* Position{x,y} pair -> move word; any coordinate >= 8 sets DC_MOVE_OOR. */
uint16_t dc_move_pack(uint32_t from_x, uint32_t from_y, uint32_t to_x, uint32_t to_y);
/* A block's Transaction.action lists (core/proto/query.proto:46-49, the u32
 * Position pairs of is_valid_tx's action[0..2], hotstuff.rs:138) -> move words:
 * actions[4i .. 4i+4) = from.x, from.y, to.x, to.y (the dc_verify_tx_batch
 * layout, so one packed block feeds both checks); moves[i] = dc_move_pack of
 * them, DC_MOVE_OOR for any coordinate >= 8 (where the reference panics). */
int dc_move_pack_batch(const uint32_t* actions, uint32_t n, uint16_t* moves);

/* ------------------------------------------------------------- validation
 * verdicts[i] = verdict of moves[i] in pos[i] (rules per call). */
int dc_validate_batch(dc_ctx* ctx, uint32_t rules, const dc_pos* pos, const uint16_t* moves, uint32_t n,
                      uint8_t* verdicts);
/* Validate and, where accepted, make the move in place (pos[i] updated, turn
 * flipped); rejected positions are left untouched (chess.rs:44-46).
 * info[i] (optional) = moved kind (cell kind 0..6) | 8 if the target held a piece,
 * which is what update_history needs (chess.rs:156-167). */
int dc_apply_batch(dc_ctx* ctx, uint32_t rules, dc_pos* pos, const uint16_t* moves, uint32_t n,
                   uint8_t* verdicts, uint8_t* info);

/* ------------------------------------------------------------ legal moves
 * The legal moves and the game status of n positions, as a dense CSR:
 * offsets (required, n + 1 entries) is the exclusive prefix sum of the
 * positions' move counts (offsets[0] = 0, *total = offsets[n]; no gaps, no
 * per-position cap), and moves[offsets[i] .. offsets[i+1]) are pos[i]'s moves
 * as move words in (from, to, promo) order: from ascending, then to, then
 * promo N, B, R, Q -- the order of dc_gen_games' k-th legal move (dc_perft's
 * root_moves are the same moves in its generator's order).  Under DC_RULES_REF the
 * list is every (from, to) dc_validate_batch accepts, under DC_RULES_FIDE
 * every (from, to, promo) (positions with at most one king per side, as
 * everywhere under FIDE).  stm is taken as stm & 1; castle and ep are ignored
 * under REF.
 * status (optional, n entries) holds DC_ST_* bits; total is optional.
 * moves == NULL or moves_cap == 0 only sizes: offsets, status and total are
 * written, DC_SUCCESS.  0 < moves_cap < total writes offsets, status and
 * total, nothing into moves, and returns DC_EINVAL; nothing is ever written
 * at or past moves[moves_cap].  A total of 2^32 or more is DC_EUNSUPPORTED.
 * The _device form takes device pointers (total stays a host pointer) and
 * returns once the results are complete. */
#define DC_ST_CHECK 1u    /* FIDE: the side to move's king is attacked */
#define DC_ST_NO_MOVES 2u /* no legal move (FIDE: CHECK|NO_MOVES = checkmate, NO_MOVES alone = stalemate) */
#define DC_ST_DEAD 4u     /* FIDE: insufficient material -- only kings, knights and bishops, and at most
                             one knight or bishop in all, or no knight and all bishops on one square colour */
int dc_legal_moves_batch(dc_ctx* ctx, uint32_t rules, const dc_pos* pos, uint32_t n, uint32_t* offsets,
                         uint8_t* status, uint16_t* moves, uint32_t moves_cap, uint32_t* total);
int dc_legal_moves_batch_device(dc_ctx* ctx, uint32_t rules, const dc_pos* d_pos, uint32_t n, uint32_t* d_offsets,
                                uint8_t* d_status, uint16_t* d_moves, uint32_t moves_cap, uint32_t* total);

/* The live validator (opt-in, per context): with lease_us > 0, every
 * dc_validate_batch / dc_apply_batch call of at most 64 moves on this context
 * is served by one resident GPU wave that polls a pinned mailbox (no kernel
 * launch per call) -- the n = 1 call is_valid_tx makes before a replica signs
 * its vote (core/src/consensus/hotstuff.rs:138, :52).  Results are identical
 * to the launched path.  The wave leaves after lease_us microseconds without a
 * call (at most 60 s; the next call restarts it), on dc_live_validator(ctx, 0)
 * and in dc_ctx_destroy.  At most one wave is resident per process: a live
 * call that starts its context's wave stops the others' first.  Every other
 * call of this library that uses the device (perft, replay, hashing,
 * signatures, launched validate / apply, device memory, dc_ctx_destroy) stops
 * the resident wave first and keeps new ones from starting until it returns:
 * HIP maps a process's streams onto a few hardware queues, and work queued
 * behind a resident wave -- and hipFree, which waits for every stream -- would
 * otherwise wait for its lease.  GPU work the CALLER issues itself (its own
 * kernels, hipDeviceSynchronize, hipFree) while a wave is resident can wait
 * for the lease: switch the validator off (lease 0) before such work. */
int dc_live_validator(dc_ctx* ctx, uint32_t lease_us);

/* ------------------------------------------------------------------ replay
 * Replays n_games games of n_plies ply-major moves (moves[ply*n_games + g])
 * from *start (NULL = startpos).  Per ply: verdict; apply only if accepted
 * (core/src/consensus/hotstuff.rs:52-56).  bitmap (optional) is ply-major
 * [n_plies][ceil(n_games/64)] of accept bits (bits past the last game are 0);
 * digests (optional) [n_games] are the final-state digests.  A digest covers
 * the piece placement and the side to move, not the castling rights or the
 * en-passant square (DC_RULES_FIDE): two games that differ only in those have
 * equal digests, and differ in the accept bits of their later moves.  A
 * DC_MOVE_NONE ply is skipped: not counted, and the turn does not flip; a
 * flagged word (bit 15) counts as validated and rejected. */
int dc_replay(dc_ctx* ctx, uint32_t rules, const dc_pos* start, const uint16_t* moves, uint32_t n_games,
              uint32_t n_plies, uint64_t* bitmap, uint64_t* digests, dc_replay_stats* stats);
int dc_replay_device(dc_ctx* ctx, uint32_t rules, const dc_pos* start, const uint16_t* d_moves,
                     uint32_t n_games, uint32_t n_plies, uint64_t* d_bitmap, uint64_t* d_digests,
                     dc_replay_stats* stats);

/* Replay for a resyncing replica (the history-rebuild path): dc_replay plus
 * info (ply-major [n_plies][n_games] bytes, like the moves): for an accepted
 * ply the moved piece's cell kind (0 P .. 5 K) | 8 if the target held a piece
 * -- dc_apply_batch's info, what update_history needs (chess.rs:156-167) --
 * and 0xFF for a rejected or DC_MOVE_NONE ply.  RULES_REF only (else
 * DC_EUNSUPPORTED), and n_games * n_plies * 2 < 4 GiB per call.
 * Replaces commit_block's per-move apply_move + update_history loop
 * (core/src/consensus/hotstuff.rs:41-56) for a whole move log at once. */
int dc_replay_info(dc_ctx* ctx, uint32_t rules, const dc_pos* start, const uint16_t* moves, uint32_t n_games,
                   uint32_t n_plies, uint64_t* bitmap, uint64_t* digests, uint8_t* info, dc_replay_stats* stats);
int dc_replay_info_device(dc_ctx* ctx, uint32_t rules, const dc_pos* start, const uint16_t* d_moves,
                          uint32_t n_games, uint32_t n_plies, uint64_t* d_bitmap, uint64_t* d_digests,
                          uint8_t* d_info, dc_replay_stats* stats);
/* GameState::update_history (chess.rs:127-184) over one game's plies, on the
 * host: history (NUL-terminated UTF-8, NULL = "") followed by one
 * "N. <notation>" token pair per accepted ply (info != 0xFF), numbered as the
 * reference numbers them (N = 1 + the whitespace-separated tokens already
 * present: 1, 3, 5, ...).  moves/info of ply p at [p * stride] (stride =
 * n_games for a column of dc_replay_info's ply-major arrays).  *out_len = the
 * result's length; out (capacity out_cap, incl. the NUL) receives it, or
 * DC_EINVAL if out_cap is too small (out_cap = 0 only sizes it). */
int dc_history_append(const char* history, const uint16_t* moves, const uint8_t* info, uint32_t n_plies,
                      size_t stride, char* out, size_t out_cap, size_t* out_len);

/* ------------------------------------------------------------ game outcome
 * dc_replay under DC_RULES_FIDE that also adjudicates: for every game, the
 * ply at which it ended and how.  A replica replaying a move log calls it
 * before it votes; plies past end_ply belong to no game and are to be rejected.
 *
 * Layout as dc_replay: moves ply-major (moves[ply*n_games + g]), start NULL =
 * startpos, DC_MOVE_NONE skipped.  A rejected move leaves the position, the
 * clock and the occurrence counts untouched; it counts in stats->validated and
 * stats->rejected.
 * Terminal check: on the start position and on the position after every
 * accepted move, in the priority checkmate > stalemate > dead > fivefold >
 * seventy-five (checkmate on the move that completes 75 moves wins, FIDE
 * 9.6.2; the others are all draws, the order only fixes the code).  Once a game
 * is terminal its remaining moves are neither validated nor applied, their
 * bitmap bits are 0, they do not count in stats, and the game's digest is the
 * terminal position's (dc_replay's digest of the game cut at end_ply).
 * Half-move clock: starts at start_halfmove (<= 150, else DC_EINVAL), returns
 * to 0 on a pawn move or a capture (en passant included), else goes up by 1.
 * Position identity (FIDE 9.2.2): same piece placement, side to move and
 * castling rights; the en-passant square is part of it only where at least one
 * en-passant capture is legal (a capture by a pinned pawn is not).
 * Occurrences are counted from start on, start being occurrence 1 (earlier
 * positions are unknown); only positions since the last clock reset can match.
 * Positions are compared whole, never by hash.  The claimable draws are left
 * to the caller: repeats >= 3 (threefold) and halfmove >= 100 (fifty moves) on
 * the final position do not end a game.
 * counts (optional, DC_GO_COUNT entries): counts[k] = games with result k,
 * reduced on the device.  bitmap, digests and stats as dc_replay's (optional);
 * outcomes is required.  Any n_games dc_replay serves: the games are
 * adjudicated in chunks, so the history memory stays bounded.
 * Kernel timing name: "replay_outcome" (units: moves consumed).
 * The _device form takes d_moves, d_outcomes, d_bitmap and d_digests in device
 * memory; counts and stats stay host pointers. */
#define DC_GO_ONGOING      0
#define DC_GO_WHITE_WINS   1  /* Black is checkmated */
#define DC_GO_BLACK_WINS   2  /* White is checkmated */
#define DC_GO_STALEMATE    3
#define DC_GO_DEAD         4  /* DC_ST_DEAD's definition, unchanged */
#define DC_GO_FIVEFOLD     5  /* FIDE 9.6.1 */
#define DC_GO_SEVENTYFIVE  6  /* FIDE 9.6.2: half-move clock reached 150 */
#define DC_GO_COUNT        7
typedef struct dc_game_outcome {
  uint8_t result;    /* DC_GO_* */
  uint8_t repeats;   /* occurrences of the FINAL position, itself included (>= 1) */
  uint16_t halfmove; /* half-move clock of the final position */
  uint32_t end_ply;  /* plies consumed: index + 1 of the move that ended the game,
                        0 if the start position is already terminal, n_plies if ongoing */
} dc_game_outcome;   /* 8 bytes */
/* outcomes / d_outcomes: dc_game_outcome[n_games], declared void* (the Rust
 * binding's type check, tests/test_abi.py, knows a fixed set of struct names). */
int dc_replay_outcome(dc_ctx* ctx, const dc_pos* start, uint32_t start_halfmove, const uint16_t* moves,
                      uint32_t n_games, uint32_t n_plies, void* outcomes, uint64_t* bitmap, uint64_t* digests,
                      uint64_t* counts, dc_replay_stats* stats);
int dc_replay_outcome_device(dc_ctx* ctx, const dc_pos* start, uint32_t start_halfmove, const uint16_t* d_moves,
                             uint32_t n_games, uint32_t n_plies, void* d_outcomes, uint64_t* d_bitmap,
                             uint64_t* d_digests, uint64_t* counts, dc_replay_stats* stats);
/* dc_replay_outcome with a start position and a half-move clock PER GAME, and
 * the position each game stopped in: a puzzle set, an opening-suite match file
 * or a set of adjourned games is one batch, not one batch per start.
 * starts[g] is game g's start position (starts NULL: every game begins at the
 * start position); start_halfmoves[g] its half-move clock (NULL: all 0).
 * Everything else means what it means in dc_replay_outcome: layout,
 * DC_MOVE_NONE, terminal priority, position identity, occurrences counted from
 * each game's own start, the chunking, counts and stats.
 * finals (optional, n_games entries): finals[g] is the position in which game
 * g stopped -- the one after its last accepted move before end_ply, its start
 * if none was accepted -- written as dc_apply_batch leaves a dc_pos after the
 * same accepted moves: stm, castle = the remaining rights, ep = the square
 * behind a pawn that just moved two ranks or -1, the reserved fields 0.  With
 * outcomes[g].halfmove it is what dc_pos_to_fen needs, and what a later
 * *_starts call needs to go on with the game.  Occurrences are counted from
 * each CALL's start: a continuation knows nothing of the positions before it,
 * so repeats and a fivefold ending can differ from the unsplit replay's.
 * Host form: any starts[g].stm > 1 or start_halfmoves[g] > 150 is DC_EINVAL,
 * found before any device work, nothing written.  n_games == 0 is a
 * successful no-op; NULL rules as dc_replay_outcome's.
 * _device form: d_starts, d_start_halfmoves and d_finals are device pointers
 * like d_moves (each may be NULL, with the meaning above); the host cannot
 * look into them, so nothing is rejected: a lane takes stm & 1, castle & 15,
 * an ep outside 0..63 as none (as every DC_RULES_FIDE kernel reads a dc_pos)
 * and min(start_halfmoves[g], 150) -- a clock above 150 behaves as 150, so the
 * game is over at ply 0 (seventy-five, unless the start is mate, stalemate or
 * dead), and the position history is never indexed outside its slots 0..150.
 * Kernel timing name: "replay_outcome_starts" (units: moves consumed). */
int dc_replay_outcome_starts(dc_ctx* ctx, const dc_pos* starts, const uint16_t* start_halfmoves,
                             const uint16_t* moves, uint32_t n_games, uint32_t n_plies, void* outcomes,
                             uint64_t* bitmap, uint64_t* digests, uint64_t* counts, dc_replay_stats* stats,
                             dc_pos* finals);
int dc_replay_outcome_starts_device(dc_ctx* ctx, const dc_pos* d_starts, const uint16_t* d_start_halfmoves,
                                    const uint16_t* d_moves, uint32_t n_games, uint32_t n_plies, void* d_outcomes,
                                    uint64_t* d_bitmap, uint64_t* d_digests, uint64_t* counts,
                                    dc_replay_stats* stats, dc_pos* d_finals);
/* The half-move clock and full-move number of a FEN (its fifth and sixth
 * fields, which dc_pos_from_fen does not keep), on the host; absent fields
 * give 0 and 1.  Either output may be NULL. */
int dc_fen_clocks(const char* fen, uint32_t* halfmove, uint32_t* fullmove);

/* ------------------------------------------------- notation (SAN, PGN, FEN)
 * dc_replay_san is dc_replay_outcome -- same arguments, same outcomes, bitmap,
 * digests, counts and stats -- that also says what was played: san (required)
 * is ply-major [n_plies][n_games] bytes, laid out like the moves.  It is the
 * DC_RULES_FIDE counterpart of dc_replay_info + dc_history_append: a replica
 * that resyncs a standard-chess move log gets its move text from one replay.
 *
 * The byte of an accepted ply:
 *   bits 0-2  the moved piece's cell kind (0 P, 1 N, 2 B, 3 R, 4 Q, 5 K)
 *   bit 3     DC_SAN_CAPTURE: the target held a piece, or en passant
 *             (the low four bits are dc_replay_info's info)
 *   bit 4     DC_SAN_FILE:  the origin file must be written
 *   bit 5     DC_SAN_RANK:  the origin rank must be written
 *   bit 6     DC_SAN_CHECK: the move leaves the opponent's king attacked
 *   bit 7     DC_SAN_MATE:  ... and the opponent without a legal move (CHECK is set too)
 * A rejected ply, a DC_MOVE_NONE ply and every ply at or past the game's
 * end_ply hold 0xFF (kind 7 does not exist, so 0xFF is no move's byte).
 * Disambiguation (FIDE C.10.3, PGN 8.2.3.4), knights, bishops, rooks and queens
 * only: let `others` be the other pieces of the mover's kind and colour that
 * can LEGALLY move to the same square -- a pinned piece whose move would leave
 * its pin line does not count, and no pinned piece counts while its side is in
 * check.  None: neither flag.  None of them on the mover's file: FILE.  Else
 * none of them on the mover's rank: RANK.  Else both.  Pawns and kings never
 * carry the flags (the formatter writes a capturing pawn's file by rule).
 * CHECK and MATE are the adjudication of the position the move leads to, which
 * the replay makes anyway.
 * Kernel timing name: "replay_san" (units: moves consumed).
 * The _device form takes d_moves, d_outcomes, d_san, d_bitmap and d_digests in
 * device memory; counts and stats stay host pointers. */
#define DC_SAN_CAPTURE 0x08u
#define DC_SAN_FILE    0x10u
#define DC_SAN_RANK    0x20u
#define DC_SAN_CHECK   0x40u
#define DC_SAN_MATE    0x80u
int dc_replay_san(dc_ctx* ctx, const dc_pos* start, uint32_t start_halfmove, const uint16_t* moves,
                  uint32_t n_games, uint32_t n_plies, void* outcomes, uint8_t* san, uint64_t* bitmap,
                  uint64_t* digests, uint64_t* counts, dc_replay_stats* stats);
int dc_replay_san_device(dc_ctx* ctx, const dc_pos* start, uint32_t start_halfmove, const uint16_t* d_moves,
                         uint32_t n_games, uint32_t n_plies, void* d_outcomes, uint8_t* d_san, uint64_t* d_bitmap,
                         uint64_t* d_digests, uint64_t* counts, dc_replay_stats* stats);
/* dc_replay_san with dc_replay_outcome_starts' per-game starts, clocks and
 * finals (same meaning, same checks).  Kernel timing name: "replay_san_starts". */
int dc_replay_san_starts(dc_ctx* ctx, const dc_pos* starts, const uint16_t* start_halfmoves, const uint16_t* moves,
                         uint32_t n_games, uint32_t n_plies, void* outcomes, uint8_t* san, uint64_t* bitmap,
                         uint64_t* digests, uint64_t* counts, dc_replay_stats* stats, dc_pos* finals);
int dc_replay_san_starts_device(dc_ctx* ctx, const dc_pos* d_starts, const uint16_t* d_start_halfmoves,
                                const uint16_t* d_moves, uint32_t n_games, uint32_t n_plies, void* d_outcomes,
                                uint8_t* d_san, uint64_t* d_bitmap, uint64_t* d_digests, uint64_t* counts,
                                dc_replay_stats* stats, dc_pos* d_finals);
/* The SAN token of one accepted move, on the host: out receives at most 7
 * characters and the NUL.  Piece letter (none for a pawn), origin file and
 * rank as the flags say, "x" for a capture, the target square; a capturing
 * pawn writes its file ("exd5", en passant too, no suffix); "=N" / "=B" / "=R"
 * / "=Q" from the move word's promo field; "O-O" / "O-O-O" for a king move of
 * two files; then "#" if MATE, else "+" if CHECK.  DC_EINVAL for san = 0xFF, a
 * kind above 5, a move with DC_MOVE_OOR, or a promo field that does not fit the
 * kind (any on a piece, above 4, or a pawn reaching the last rank without). */
int dc_san_format(uint16_t move, uint8_t san, char out[8]);
/* The PGN movetext of one game, on the host, as one line with single spaces:
 * "1. e4 e5 2. Nf3 ... <result>".  moves/san of ply p at [p * stride] (stride =
 * n_games for a column of dc_replay_san's arrays); plies whose byte is 0xFF
 * are skipped.  The first written move is numbered first_fullmove and made by
 * first_stm (0 White, 1 Black: the line then begins "N... ").  The line ends
 * with the token of result (a DC_GO_* code): "1-0", "0-1", "1/2-1/2" for the
 * four draws, "*" for DC_GO_ONGOING; a game without moves is that token alone.
 * out, out_cap and out_len as dc_history_append's: out_cap = 0 only sizes,
 * a capacity that is too small is DC_EINVAL. */
int dc_pgn_movetext(const uint16_t* moves, const uint8_t* san, uint32_t n_plies, size_t stride,
                    uint32_t first_fullmove, uint8_t first_stm, uint8_t result, char* out, size_t out_cap,
                    size_t* out_len);
/* The FEN of a position, on the host: the inverse of dc_pos_from_fen plus
 * dc_fen_clocks (PGN needs it for a game that does not begin at the start
 * position).  Sizing as above.  DC_EUNSUPPORTED if the board holds a piece of
 * kind OTHER; DC_EINVAL for stm > 1 or ep outside -1..63. */
int dc_pos_to_fen(const dc_pos* pos, uint32_t halfmove, uint32_t fullmove, char* out, size_t out_cap,
                  size_t* out_len);

/* ---------------------------------------------------------- notation input
 * The way back: SAN / PGN movetext -> move words.  A host parser turns text
 * into one token word per written move; dc_san_resolve finds, per position and
 * on the device, the one legal move a token means (DC_RULES_FIDE only).
 *
 * Token word (uint32, ply-major [n_plies][n_games] like the moves):
 *   bits 0-5    target square (8*x+y)
 *   bits 6-8    piece kind, cell kind 0 P .. 5 K
 *   bits 9-11   promotion 0 none, 1 N, 2 B, 3 R, 4 Q
 *   bit  12     origin file given       bits 13-15  origin file
 *   bit  16     origin rank given       bits 17-19  origin rank
 *   bit  20     O-O                     bit  21     O-O-O
 *               (with either castle bit, bits 0-19 are 0)
 *   bit  22     "x" written   bit 23  "+" written   bit 24  "#" written
 *   bits 25-31  0
 * Bits 22-24 are recorded by the parser and ignored by the resolver.
 * DC_SAN_TOKEN_NONE means "no move": skipped, the turn does not flip
 * (DC_MOVE_NONE's meaning). */
#define DC_SAN_TOKEN_NONE (0xFFFFFFFFu)
#define DC_PGN_DRAW 3 /* dc_pgn_parse_movetext's result for "1/2-1/2" */
/* One SAN token, on the host (no context):
 *   [KQRBN]? [a-h]? [1-8]? x? [a-h][1-8] (=[QRBN])? [+#]? [!?]*
 * or O-O / O-O-O (letter O or digit 0) with the same suffixes.  No piece
 * letter means a pawn; letters are case-sensitive ("bxc3" is a pawn, "Bxc3" a
 * bishop).  Everything dc_san_format writes parses, and so do the long forms
 * ("Ng1f3", "e2e4").  Anything else is DC_EINVAL: an empty string, "e.p.", a
 * promotion on a piece letter, trailing characters. */
int dc_san_parse(const char* text, size_t len, uint32_t* token);
/* One game's movetext, on the host: the token of written move k goes to
 * tokens[k * stride] (stride 0 counts as 1).  Skipped: move numbers ("12.",
 * "12..."), {...} comments, ";" comments to the end of the line, "$n" NAGs and
 * nested "( ... )" variations.  Reading stops after the first result token:
 * *result is 0 for "*" or the end of the text, 1 for "1-0", 2 for "0-1" (the
 * DC_GO_* codes) and DC_PGN_DRAW for "1/2-1/2".  *first_fullmove / *first_stm
 * come from the first move number seen before any move ("N..." means Black;
 * defaults 1 and 0).  *consumed is the number of bytes read through the result
 * token, so a caller can walk a stream of games.  Sizing as dc_pgn_movetext's:
 * with tokens NULL or cap 0 only *n_tokens and the other outputs are written;
 * with 0 < cap < *n_tokens the call is DC_EINVAL, *n_tokens set and nothing
 * written past cap.  A word that is neither skippable nor a SAN token is
 * DC_EINVAL with *consumed the offset of that word.  n_tokens is required, the
 * other outputs may be NULL.  Tag pairs ("[Event ...]") are not read here. */
int dc_pgn_parse_movetext(const char* text, size_t len, uint32_t* tokens, size_t stride, uint32_t cap,
                          uint32_t* n_tokens, uint8_t* result, uint32_t* first_fullmove, uint8_t* first_stm,
                          size_t* consumed);

/* dc_san_resolve: tokens -> move words, one game per lane, from start (NULL:
 * the start position).  Per ply: DC_SAN_TOKEN_NONE gives DC_MOVE_NONE and
 * changes nothing.  Otherwise the side to move's pieces that fit the token and
 * may LEGALLY move to its target are counted (pins, checks and en-passant
 * legality decide, never geometry alone):
 *   piece tokens (N B R Q K)  own pieces of the kind, on the origin file / rank
 *                             if given; a K token never means a castle
 *   castle tokens             the king, two files towards h (O-O) or a (O-O-O)
 *   pawn tokens               own pawns on the origin file, or on the TARGET's
 *                             file if none is given ("e4" is the push even when
 *                             "dxe4" is legal; "exd6" a capture, en passant
 *                             included), on the origin rank if given; the promo
 *                             field must be 1..4 exactly when the target is on
 *                             the last rank, else the token has no match
 * Exactly one: its move word (promo field included) is written, the move made
 * and the turn flipped.  Otherwise one of the flagged words below is written,
 * the position stays, and the next token is tried against it.  The flagged
 * words have bit 15 set, which dc_replay* counts as validated and rejected: a
 * resolved array can go to dc_replay_outcome / dc_replay_san as it is.
 * first_bad[g] (optional) is the first ply of game g with a flagged word, or
 * n_plies; counts (optional, host) has DC_SR_COUNT entries summed over the batch.
 * The resolver does not adjudicate and keeps neither history nor clocks: after
 * mate or stalemate every token is DC_MOVE_NOMATCH by itself (no legal move),
 * but after a fivefold, 75-move or dead-position ending it goes on resolving;
 * dc_replay_outcome on the resolved moves cuts the game at end_ply.
 * n_games == 0 or n_plies == 0 is a successful no-op (first_bad all 0).
 * DC_EINVAL: start->stm > 1, or NULL tokens / moves with n_games && n_plies.
 * Kernel timing name: "san_resolve" (units: tokens other than NONE).
 * The _device form takes d_tokens, d_moves and d_first_bad in device memory. */
#define DC_MOVE_NOMATCH   0x8001u /* no legal move fits the token */
#define DC_MOVE_AMBIGUOUS 0x8002u /* two or more legal moves fit */
#define DC_MOVE_MALFORMED 0x8003u /* kind > 5, promo > 4, reserved bits, both castle bits, castle with other
                                     fields, promo on a piece */
#define DC_SR_TOKENS    0 /* tokens other than DC_SAN_TOKEN_NONE */
#define DC_SR_RESOLVED  1
#define DC_SR_NOMATCH   2
#define DC_SR_AMBIGUOUS 3
#define DC_SR_MALFORMED 4
#define DC_SR_COUNT     5
int dc_san_resolve(dc_ctx* ctx, const dc_pos* start, const uint32_t* tokens, uint32_t n_games, uint32_t n_plies,
                   uint16_t* moves, uint32_t* first_bad, uint64_t* counts);
int dc_san_resolve_device(dc_ctx* ctx, const dc_pos* start, const uint32_t* d_tokens, uint32_t n_games,
                          uint32_t n_plies, uint16_t* d_moves, uint32_t* d_first_bad, uint64_t* counts);
/* dc_san_resolve with a start position per game (starts NULL: the start
 * position for all) and, optionally, finals[g] = the position after game g's
 * last resolved move (its start if none), written as dc_replay_outcome_starts
 * writes it.  The host form rejects any starts[g].stm > 1 with DC_EINVAL before
 * any device work; the _device form takes d_starts and d_finals in device
 * memory and reads stm & 1.  With n_plies == 0 first_bad is all 0 and finals
 * are the starts.  Kernel timing name: "san_resolve_starts". */
int dc_san_resolve_starts(dc_ctx* ctx, const dc_pos* starts, const uint32_t* tokens, uint32_t n_games,
                          uint32_t n_plies, uint16_t* moves, uint32_t* first_bad, uint64_t* counts, dc_pos* finals);
int dc_san_resolve_starts_device(dc_ctx* ctx, const dc_pos* d_starts, const uint32_t* d_tokens, uint32_t n_games,
                                 uint32_t n_plies, uint16_t* d_moves, uint32_t* d_first_bad, uint64_t* counts,
                                 dc_pos* d_finals);

/* Seeded synthetic games: rng = splitmix64 from seed ^ game_id;
 * per ply one draw r: (r & 0xFF) < noise_per_256 -> move (r>>8)&0xFFF, else the
 * ((r>>32)*n>>32)-th legal move in (from, to, promo) order; no legal move ->
 * DC_MOVE_NONE for the rest of the game.  Output ply-major [n_plies][n_games]. */
int dc_gen_games(dc_ctx* ctx, uint32_t rules, uint64_t seed, uint64_t first_game, uint32_t n_games,
                 uint32_t n_plies, uint32_t noise_per_256, uint16_t* out);
int dc_gen_games_device(dc_ctx* ctx, uint32_t rules, uint64_t seed, uint64_t first_game, uint32_t n_games,
                        uint32_t n_plies, uint32_t noise_per_256, uint16_t* d_out);

/* ------------------------------------------------------------- state hash
 * The hash a replica compares before voting: keccak256(serde_json(GameState))
 * (core/src/consensus/hotstuff.rs:153-166 calculate_game_state_hash; the same
 * keccak-of-JSON as BlockBuilder::build, core/src/consensus/types.rs:45-55).
 *
 * dc_keccak256: alloy-primitives keccak256 (Keccak-256, padding 0x01..0x80)
 * of one byte string, on the host -- the single-state path of the host
 * mirrors.
 *
 * dc_state_hash: for every game of a replay batch, the hash of its FINAL
 * GameState, on the GPU: start (dc_pos; NULL = startpos; turn = start.stm)
 * plus the game's accepted moves (RULES_REF, chess.rs:43-80), each one's
 * notation appended to `history` (chess.rs:127-184; the start history is
 * shared by all games, NUL-terminated UTF-8, "" for GameState::new).  Player
 * names: UTF-8 bytes names[names_off[2g] .. names_off[2g+1]) (white) and
 * [names_off[2g+1] .. names_off[2g+2]) (black); names_off has 2*n_games+1
 * entries.  hashes[32 g .. 32 g + 32) = the 32 digest bytes (alloy B256;
 * "0x" + hex of them is calculate_game_state_hash's String).  A start board
 * holding pieces of unknown kind returns DC_EUNSUPPORTED (their proto kind
 * string is not representable in a dc_pos).
 *
 * dc_state_hash_device: the same with d_names, d_names_off, d_moves and
 * d_hashes in device memory (raw UTF-8, as for dc_state_hash; history stays a
 * host string).  serde_json's escaping of the names runs on the device; a
 * decreasing offset pair is taken as an empty name (dc_state_hash rejects it
 * with DC_EINVAL).  Escaped text past 4 GiB returns DC_EUNSUPPORTED. */
int dc_keccak256(const void* data, size_t len, uint8_t out[32]);
int dc_state_hash(dc_ctx* ctx, const dc_pos* start, const char* history, const char* names,
                  const uint32_t* names_off, const uint16_t* moves, uint32_t n_games, uint32_t n_plies,
                  uint8_t* hashes);
int dc_state_hash_device(dc_ctx* ctx, const dc_pos* start, const char* history, const char* d_names,
                         const uint32_t* d_names_off, const uint16_t* d_moves, uint32_t n_games, uint32_t n_plies,
                         uint8_t* d_hashes);

/* ---------------------------------------------------- transaction signatures
 * The other per-transaction check of is_valid_tx (core/src/consensus/hotstuff.rs:139):
 * App::validate_signature (hotstuff.rs:168-208), batched on the GPU.  Per
 * transaction i:
 *   strings[str_off[4i+0] .. str_off[4i+1])  white_player (UTF-8)
 *   strings[str_off[4i+1] .. str_off[4i+2])  black_player
 *   strings[str_off[4i+2] .. str_off[4i+3])  signature (hex text, 64 bytes r||s)
 *   strings[str_off[4i+3] .. str_off[4i+4])  pub_key (hex text: 33, 64 or 65 bytes)
 *   actions[4i .. 4i+4) = action[0].x, action[0].y, action[1].x, action[1].y
 *   turns[i] (optional; NULL or -1 = skip) = the game's turn: after a valid
 *   signature, pub_key must equal the string of the player to move
 *   (hotstuff.rs:141-148), else DC_SIG_WRONG_OWNER.
 * The signed message is serde_json {"whitePlayer","blackPlayer","action":[{x,y},{x,y}]}
 * (hotstuff.rs:169-179), hashed with SHA-256; verification follows
 * libsecp256k1 0.7.1 (Message mod n, parse_standard_slice, parse_slice,
 * verify without a low-s rule).  Verdicts in the reference's check order: */
#define DC_SIG_OK 0
#define DC_SIG_BAD_SIG_HEX 1  /* hex::decode(signature) failed            hotstuff.rs:183-184 */
#define DC_SIG_BAD_SIG 2      /* Signature::parse_standard_slice failed    hotstuff.rs:186-191 */
#define DC_SIG_BAD_PK_HEX 3   /* hex::decode(pub_key) failed               hotstuff.rs:193-194 */
#define DC_SIG_BAD_PK 4       /* PublicKey::parse_slice failed             hotstuff.rs:195-200 */
#define DC_SIG_INVALID 5      /* verify() false: "invalid signature"       hotstuff.rs:202-206 */
#define DC_SIG_WRONG_OWNER 6  /* pub_key is not the mover: "invalud turn"  hotstuff.rs:141-148 */
int dc_verify_tx_batch(dc_ctx* ctx, const char* strings, const uint32_t* str_off, const uint32_t* actions,
                       const int8_t* turns, uint32_t n, uint8_t* verdicts);
int dc_verify_tx_batch_device(dc_ctx* ctx, const char* d_strings, const uint32_t* d_str_off,
                              const uint32_t* d_actions, const int8_t* d_turns, uint32_t n, uint8_t* d_verdicts);
/* Text for a DC_SIG_* verdict ("" for OK; codes 5 and 6 are the reference's strings). */
const char* dc_sig_verdict_message(uint8_t verdict);

/* -------------------------------------------------------------------- perft
 * perft(pos, depth) = number of leaf nodes of the move tree (under
 * REF the tree is every (from,to) pair validate_move accepts).  divide[i] is the
 * count below root move root_moves[i]; both arrays need room for 256 entries
 * (pass NULL to skip).  Root moves are in (from, to, promo) order. */
int dc_perft(dc_ctx* ctx, uint32_t rules, const dc_pos* pos, uint32_t depth, uint64_t* divide,
             uint16_t* root_moves, uint32_t* n_root, uint64_t* total);
/* One shard of perft for data-parallel runs: the frontier at ply `split_depth`
 * (N nodes) is built deterministically, and this call counts only the subtrees
 * of the STRIDED shard of it -- frontier nodes shard, shard + n_shards,
 * shard + 2*n_shards, ... < N (the front end selects them by index: REF depth
 * 6/7 at split 3 in k_front, else k_make_count over the top kernel's move
 * words; strided shards hold equal leaf counts to about 1 %, contiguous ones
 * did not).  Summing divide[] over all shards (e.g. an RCCL all-reduce) gives
 * dc_perft's result exactly. */
int dc_perft_shard(dc_ctx* ctx, uint32_t rules, const dc_pos* pos, uint32_t depth, uint32_t split_depth,
                   uint32_t shard, uint32_t n_shards, uint64_t* divide, uint16_t* root_moves,
                   uint32_t* n_root, uint64_t* total);

/* ------------------------------------------------------- perft statistics
 * The columns of the published perft tables: every counter classifies the LAST
 * move of a line, the move that reaches a leaf at ply `depth`.  totals
 * (required) has room for DC_PS_COUNT entries; rows (NULL to skip) for
 * 256 * DC_PS_COUNT: rows[DC_PS_COUNT * i + k] is counter k below root move
 * root_moves[i].  root_moves / n_root are dc_perft's, in its root-move order.
 * DC_RULES_FIDE: CAPTURES includes en passant; CASTLES = king moves of two
 * files; CHECKS = the side now to move has its king attacked (discovered and
 * double checks included); DOUBLE = two or more checkers; DISCOVERED = exactly
 * one checker that is not the piece that moved (not on the move's `to` square,
 * where a promoted piece stands; not the castled rook; an en-passant capture
 * whose check runs through the vacated squares is discovered); CHECKMATES /
 * STALEMATES = the child has no legal move, with / without check; a side with
 * no king is never in check.  DC_RULES_REF (no check concept): NODES,
 * CAPTURES (dc_apply_batch's capture bit) and KING_CAPTURES; the rest are 0.
 * Depth 0: NODES 1 (shard 0), n_root 0; depth 1 classifies the root's own
 * moves.  Errors as dc_perft_shard's; totals and rows summed over the shards of
 * one (split_depth, n_shards) equal the unsharded result exactly. */
#define DC_PS_NODES         0  /* leaf moves = dc_perft's count */
#define DC_PS_CAPTURES      1  /* target square held a piece, or en passant */
#define DC_PS_EP            2
#define DC_PS_CASTLES       3
#define DC_PS_PROMOTIONS    4  /* each of the four promotion moves counts once */
#define DC_PS_CHECKS        5  /* the move leaves the opponent's king attacked */
#define DC_PS_DISCOVERED    6
#define DC_PS_DOUBLE        7
#define DC_PS_CHECKMATES    8
#define DC_PS_STALEMATES    9
#define DC_PS_KING_CAPTURES 10 /* REF: the captured piece is a king; FIDE: 0 */
#define DC_PS_COUNT         11
int dc_perft_stats(dc_ctx* ctx, uint32_t rules, const dc_pos* pos, uint32_t depth, uint64_t* totals,
                   uint64_t* rows, uint16_t* root_moves, uint32_t* n_root);
int dc_perft_stats_shard(dc_ctx* ctx, uint32_t rules, const dc_pos* pos, uint32_t depth, uint32_t split_depth,
                         uint32_t shard, uint32_t n_shards, uint64_t* totals, uint64_t* rows,
                         uint16_t* root_moves, uint32_t* n_root);

/* n_runs perfts of *pos (depth >= 2; shard as dc_perft_shard) enqueued back to
 * back on the context stream with no host round trip between them.  Run i
 * leaves its result in DEVICE memory d_out[258 i .. 258 i + 258):
 *   [0, 256) divide per root move (0 past n_root; root-move order as dc_perft)
 *   [256]    n_root | overflow << 32  (overflow != 0: redo with dc_perft_shard)
 *   [257]    total leaves of this shard
 * Returns once the runs are enqueued; dc_ctx_synchronize (or an event on
 * dc_ctx_stream) orders the caller after them.  For throughput work (a suite
 * of repeated perfts, the bench's timed steps, a device-side all-reduce of
 * each run's divide vector). */
int dc_perft_repeat_device(dc_ctx* ctx, uint32_t rules, const dc_pos* pos, uint32_t depth, uint32_t split_depth,
                           uint32_t shard, uint32_t n_shards, uint32_t n_runs, uint64_t* d_out);

/* perft of a batch of n_pos (1..DC_PERFT_BATCH_MAX) positions with the same side
 * to move, counted as one tree: their root moves (at most 256 in all; more is
 * DC_EUNSUPPORTED) share the divide tags, so every level -- the final stage's
 * included -- holds all positions and runs one grid instead of one per position
 * (a perft suite: BASELINE configs[2], the six published positions at depth 5).
 * totals[i] = perft(pos[i], depth); divide / root_moves as dc_perft over the
 * concatenated root moves, root_pos[k] = the position root move k belongs to
 * (each may be NULL; room for 256 entries). */
#define DC_PERFT_BATCH_MAX 8
int dc_perft_batch(dc_ctx* ctx, uint32_t rules, const dc_pos* pos, uint32_t n_pos, uint32_t depth, uint64_t* totals,
                   uint64_t* divide, uint16_t* root_moves, uint8_t* root_pos, uint32_t* n_root);
/* n_runs batch perfts enqueued as dc_perft_repeat_device does (depth >= 2, one
 * shard): run i's 258-word record in DEVICE memory holds the concatenated
 * divide ([257] = the batch's total); per-position totals are the sums of the
 * divide entries over dc_perft_batch's root_pos. */
int dc_perft_batch_repeat_device(dc_ctx* ctx, uint32_t rules, const dc_pos* pos, uint32_t n_pos, uint32_t depth,
                                 uint32_t split_depth, uint32_t n_runs, uint64_t* d_out);
/* Blocks until all work queued on the context stream has finished. */
int dc_ctx_synchronize(dc_ctx* ctx);

/* ------------------------------------------------------------- multi-GPU
 * One process, n_devices GPUs, one RCCL communicator (ncclCommInitAll); device
 * i counts strided shard i of the frontier (dc_perft_shard) and divide[] is
 * combined with ncclAllReduce(ncclUint64, ncclSum) over xGMI. */
int dc_multi_perft(const int* devices, int n_devices, uint32_t rules, const dc_pos* pos, uint32_t depth,
                   uint64_t* divide, uint16_t* root_moves, uint32_t* n_root, uint64_t* total);

/* Replay shard contract: game ids [0, n_games) are split into
 * contiguous ranges of whole 64-game bitmap words -- with W = ceil(n_games/64)
 * words and P = ceil(W/n_shards), shard s holds games [min(n_games, min(W, sP)*64),
 * min(n_games, min(W, (s+1)P)*64)) -- so its ply-major accept bitmap is the
 * word-column block [first/64, first/64 + ceil(count/64)) of every ply row of
 * the whole batch's bitmap.  Data-parallel callers (one process per GPU)
 * replay their own range and combine: validated / accepted / rejected /
 * digest_sum add (mod 2^64), digest_xor xors, bitmaps are gathered. */
int dc_replay_shard_range(uint64_t n_games, uint32_t shard, uint32_t n_shards, uint64_t* first, uint64_t* count);
/* The combine of the shards' bitmaps (host memory): gathered = n_shards blocks
 * [n_plies][per] with per = ceil(ceil(n_games/64) / n_shards) (each shard's
 * ply-major bitmap padded to `per` words per row, as a gather collects them);
 * bitmap = the whole batch's [n_plies][ceil(n_games/64)].  dc_multi_replay's
 * last step, and the layout a torch.distributed caller's gather produces. */
int dc_replay_scatter_shards(uint64_t n_games, uint32_t n_shards, uint32_t n_plies, const uint64_t* gathered,
                             uint64_t* bitmap);
/* The seeded games [0, n_games) (dc_gen_games' generator: seed, n_plies,
 * noise_per_256) generated and replayed on n_devices GPUs of one process,
 * shard i on device i.  bitmap (optional, HOST) = the whole batch's ply-major
 * [n_plies][ceil(n_games/64)] accept bitmap: the shards' bitmaps are gathered
 * to devices[0] with ncclGather over xGMI, then copied out; stats = the
 * combined counters. */
int dc_multi_replay(const int* devices, int n_devices, uint32_t rules, uint64_t seed, uint64_t n_games,
                    uint32_t n_plies, uint32_t noise_per_256, uint64_t* bitmap, dc_replay_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* DCHESS_H */
