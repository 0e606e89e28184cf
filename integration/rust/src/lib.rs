//! UNVERIFIED (no cargo/rustc in this image; text-checked against
//! include/dchess.h by tests/test_abi.py::test_rust_binding_matches_header).
//!
//! `sys`: every entry point of include/dchess.h, one to one.
//! `Engine`: a safe, panic-free layer -- every non-zero status becomes
//! `DcError`, which the reference maps into its `AppError` (core/src/errors.rs).
//! `apply_move` / `validate_move`: the reference's GameState methods
//! (core/src/chess.rs:43-125) over the proto board flattened to 64 cells.
//! See INTEGRATION.md.
#![allow(non_camel_case_types)]

use std::ffi::{CStr, CString};
use std::os::raw::{c_char, c_int, c_void};

pub mod sys {
    use std::os::raw::{c_char, c_int, c_void};

    #[repr(C)]
    #[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
    pub struct dc_pos {
        pub bb: [u64; 4],
        pub stm: u8,
        pub castle: u8,
        pub ep: i8,
        pub reserved0: u8,
        pub reserved1: u32,
    }

    #[repr(C)]
    #[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
    pub struct dc_replay_stats {
        pub validated: u64,
        pub accepted: u64,
        pub rejected: u64,
        pub digest_sum: u64,
        pub digest_xor: u64,
    }

    #[repr(C)]
    #[derive(Clone, Copy, Default, Debug)]
    pub struct dc_kernel_stats {
        pub launches: u64,
        pub total_ms: f64,
        pub units: u64,
    }

    /// One game's adjudication (dc_replay_outcome), 8 bytes.
    #[repr(C)]
    #[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
    pub struct dc_game_outcome {
        pub result: u8,
        pub repeats: u8,
        pub halfmove: u16,
        pub end_ply: u32,
    }

    pub enum dc_ctx {}

    pub const DC_SUCCESS: c_int = 0;
    pub const DC_EINVAL: c_int = -1;
    pub const DC_EHIP: c_int = -2;
    pub const DC_ENOMEM: c_int = -3;
    pub const DC_ENODEV: c_int = -4;
    pub const DC_ERCCL: c_int = -5;
    pub const DC_EUNSUPPORTED: c_int = -6;
    pub const DC_RULES_REF: u32 = 0;
    pub const DC_RULES_FIDE: u32 = 1;
    pub const DC_V_OK: u8 = 0;
    pub const DC_V_NO_PIECE: u8 = 1;
    pub const DC_V_WRONG_TURN: u8 = 2;
    pub const DC_V_ILLEGAL: u8 = 3;
    pub const DC_V_OOR: u8 = 4;
    pub const DC_MOVE_OOR: u16 = 0x8000;
    pub const DC_MOVE_NONE: u16 = 0xFFFF;
    pub const DC_CELL_EMPTY: i8 = -1;
    pub const DC_ST_CHECK: u8 = 1;
    pub const DC_ST_NO_MOVES: u8 = 2;
    pub const DC_ST_DEAD: u8 = 4;
    pub const DC_GO_ONGOING: u8 = 0;
    pub const DC_GO_WHITE_WINS: u8 = 1;
    pub const DC_GO_BLACK_WINS: u8 = 2;
    pub const DC_GO_STALEMATE: u8 = 3;
    pub const DC_GO_DEAD: u8 = 4;
    pub const DC_GO_FIVEFOLD: u8 = 5;
    pub const DC_GO_SEVENTYFIVE: u8 = 6;
    pub const DC_GO_COUNT: usize = 7;
    pub const DC_SAN_CAPTURE: u8 = 0x08;
    pub const DC_SAN_FILE: u8 = 0x10;
    pub const DC_SAN_RANK: u8 = 0x20;
    pub const DC_SAN_CHECK: u8 = 0x40;
    pub const DC_SAN_MATE: u8 = 0x80;
    pub const DC_SAN_TOKEN_NONE: u32 = 0xFFFF_FFFF;
    pub const DC_PGN_DRAW: u8 = 3;
    pub const DC_MOVE_NOMATCH: u16 = 0x8001;
    pub const DC_MOVE_AMBIGUOUS: u16 = 0x8002;
    pub const DC_MOVE_MALFORMED: u16 = 0x8003;
    pub const DC_SR_TOKENS: usize = 0;
    pub const DC_SR_RESOLVED: usize = 1;
    pub const DC_SR_NOMATCH: usize = 2;
    pub const DC_SR_AMBIGUOUS: usize = 3;
    pub const DC_SR_MALFORMED: usize = 4;
    pub const DC_SR_COUNT: usize = 5;
    pub const DC_PS_NODES: usize = 0;
    pub const DC_PS_CAPTURES: usize = 1;
    pub const DC_PS_EP: usize = 2;
    pub const DC_PS_CASTLES: usize = 3;
    pub const DC_PS_PROMOTIONS: usize = 4;
    pub const DC_PS_CHECKS: usize = 5;
    pub const DC_PS_DISCOVERED: usize = 6;
    pub const DC_PS_DOUBLE: usize = 7;
    pub const DC_PS_CHECKMATES: usize = 8;
    pub const DC_PS_STALEMATES: usize = 9;
    pub const DC_PS_KING_CAPTURES: usize = 10;
    pub const DC_PS_COUNT: usize = 11;
    pub const DC_SIG_OK: u8 = 0;
    pub const DC_SIG_BAD_SIG_HEX: u8 = 1;
    pub const DC_SIG_BAD_SIG: u8 = 2;
    pub const DC_SIG_BAD_PK_HEX: u8 = 3;
    pub const DC_SIG_BAD_PK: u8 = 4;
    pub const DC_SIG_INVALID: u8 = 5;
    pub const DC_SIG_WRONG_OWNER: u8 = 6;

    extern "C" {
        // context
        pub fn dc_ctx_create(device: c_int, out: *mut *mut dc_ctx) -> c_int;
        pub fn dc_ctx_destroy(ctx: *mut dc_ctx) -> c_int;
        pub fn dc_ctx_device(ctx: *const dc_ctx) -> c_int;
        pub fn dc_ctx_stream(ctx: *mut dc_ctx) -> *mut c_void;
        pub fn dc_strerror(status: c_int) -> *const c_char;
        pub fn dc_verdict_message(verdict: u8) -> *const c_char;
        pub fn dc_version() -> c_int;
        pub fn dc_ctx_set_profiling(ctx: *mut dc_ctx, enable: c_int) -> c_int;
        pub fn dc_ctx_kernel_stats(ctx: *mut dc_ctx, kernel: *const c_char, out: *mut dc_kernel_stats) -> c_int;
        pub fn dc_ctx_reset_stats(ctx: *mut dc_ctx) -> c_int;
        pub fn dc_device_alloc(ctx: *mut dc_ctx, bytes: usize, d_ptr: *mut *mut c_void) -> c_int;
        pub fn dc_device_free(ctx: *mut dc_ctx, d_ptr: *mut c_void) -> c_int;
        pub fn dc_memcpy_h2d(ctx: *mut dc_ctx, d_dst: *mut c_void, src: *const c_void, bytes: usize) -> c_int;
        pub fn dc_memcpy_d2h(ctx: *mut dc_ctx, dst: *mut c_void, d_src: *const c_void, bytes: usize) -> c_int;
        // adapters
        pub fn dc_startpos(out: *mut dc_pos) -> c_int;
        pub fn dc_pos_from_cells(cells: *const i8, turn: u8, out: *mut dc_pos) -> c_int;
        pub fn dc_pos_to_cells(pos: *const dc_pos, cells: *mut i8, turn: *mut u8) -> c_int;
        pub fn dc_pos_from_fen(fen: *const c_char, out: *mut dc_pos) -> c_int;
        pub fn dc_move_pack(from_x: u32, from_y: u32, to_x: u32, to_y: u32) -> u16;
        pub fn dc_move_pack_batch(actions: *const u32, n: u32, moves: *mut u16) -> c_int;
        // validation
        pub fn dc_validate_batch(ctx: *mut dc_ctx, rules: u32, pos: *const dc_pos, moves: *const u16, n: u32,
                                 verdicts: *mut u8) -> c_int;
        pub fn dc_apply_batch(ctx: *mut dc_ctx, rules: u32, pos: *mut dc_pos, moves: *const u16, n: u32,
                              verdicts: *mut u8, info: *mut u8) -> c_int;
        pub fn dc_live_validator(ctx: *mut dc_ctx, lease_us: u32) -> c_int;
        // legal moves
        pub fn dc_legal_moves_batch(ctx: *mut dc_ctx, rules: u32, pos: *const dc_pos, n: u32, offsets: *mut u32,
                                    status: *mut u8, moves: *mut u16, moves_cap: u32, total: *mut u32) -> c_int;
        pub fn dc_legal_moves_batch_device(ctx: *mut dc_ctx, rules: u32, d_pos: *const dc_pos, n: u32,
                                           d_offsets: *mut u32, d_status: *mut u8, d_moves: *mut u16,
                                           moves_cap: u32, total: *mut u32) -> c_int;
        // replay
        pub fn dc_replay(ctx: *mut dc_ctx, rules: u32, start: *const dc_pos, moves: *const u16, n_games: u32,
                         n_plies: u32, bitmap: *mut u64, digests: *mut u64, stats: *mut dc_replay_stats) -> c_int;
        pub fn dc_replay_device(ctx: *mut dc_ctx, rules: u32, start: *const dc_pos, d_moves: *const u16,
                                n_games: u32, n_plies: u32, d_bitmap: *mut u64, d_digests: *mut u64,
                                stats: *mut dc_replay_stats) -> c_int;
        pub fn dc_replay_outcome(ctx: *mut dc_ctx, start: *const dc_pos, start_halfmove: u32, moves: *const u16,
                                 n_games: u32, n_plies: u32, outcomes: *mut c_void, bitmap: *mut u64,
                                 digests: *mut u64, counts: *mut u64, stats: *mut dc_replay_stats) -> c_int;
        pub fn dc_replay_outcome_device(ctx: *mut dc_ctx, start: *const dc_pos, start_halfmove: u32,
                                        d_moves: *const u16, n_games: u32, n_plies: u32, d_outcomes: *mut c_void,
                                        d_bitmap: *mut u64, d_digests: *mut u64, counts: *mut u64,
                                        stats: *mut dc_replay_stats) -> c_int;
        pub fn dc_replay_outcome_starts(ctx: *mut dc_ctx, starts: *const dc_pos, start_halfmoves: *const u16,
                                        moves: *const u16, n_games: u32, n_plies: u32, outcomes: *mut c_void,
                                        bitmap: *mut u64, digests: *mut u64, counts: *mut u64,
                                        stats: *mut dc_replay_stats, finals: *mut dc_pos) -> c_int;
        pub fn dc_replay_outcome_starts_device(ctx: *mut dc_ctx, d_starts: *const dc_pos,
                                               d_start_halfmoves: *const u16, d_moves: *const u16, n_games: u32,
                                               n_plies: u32, d_outcomes: *mut c_void, d_bitmap: *mut u64,
                                               d_digests: *mut u64, counts: *mut u64, stats: *mut dc_replay_stats,
                                               d_finals: *mut dc_pos) -> c_int;
        pub fn dc_fen_clocks(fen: *const c_char, halfmove: *mut u32, fullmove: *mut u32) -> c_int;
        // notation
        pub fn dc_replay_san(ctx: *mut dc_ctx, start: *const dc_pos, start_halfmove: u32, moves: *const u16,
                             n_games: u32, n_plies: u32, outcomes: *mut c_void, san: *mut u8, bitmap: *mut u64,
                             digests: *mut u64, counts: *mut u64, stats: *mut dc_replay_stats) -> c_int;
        pub fn dc_replay_san_device(ctx: *mut dc_ctx, start: *const dc_pos, start_halfmove: u32,
                                    d_moves: *const u16, n_games: u32, n_plies: u32, d_outcomes: *mut c_void,
                                    d_san: *mut u8, d_bitmap: *mut u64, d_digests: *mut u64, counts: *mut u64,
                                    stats: *mut dc_replay_stats) -> c_int;
        pub fn dc_replay_san_starts(ctx: *mut dc_ctx, starts: *const dc_pos, start_halfmoves: *const u16,
                                    moves: *const u16, n_games: u32, n_plies: u32, outcomes: *mut c_void,
                                    san: *mut u8, bitmap: *mut u64, digests: *mut u64, counts: *mut u64,
                                    stats: *mut dc_replay_stats, finals: *mut dc_pos) -> c_int;
        pub fn dc_replay_san_starts_device(ctx: *mut dc_ctx, d_starts: *const dc_pos, d_start_halfmoves: *const u16,
                                           d_moves: *const u16, n_games: u32, n_plies: u32, d_outcomes: *mut c_void,
                                           d_san: *mut u8, d_bitmap: *mut u64, d_digests: *mut u64,
                                           counts: *mut u64, stats: *mut dc_replay_stats,
                                           d_finals: *mut dc_pos) -> c_int;
        pub fn dc_san_format(move_: u16, san: u8, out: *mut c_char) -> c_int;
        pub fn dc_pgn_movetext(moves: *const u16, san: *const u8, n_plies: u32, stride: usize, first_fullmove: u32,
                               first_stm: u8, result: u8, out: *mut c_char, out_cap: usize,
                               out_len: *mut usize) -> c_int;
        pub fn dc_pos_to_fen(pos: *const dc_pos, halfmove: u32, fullmove: u32, out: *mut c_char, out_cap: usize,
                             out_len: *mut usize) -> c_int;
        // notation input
        pub fn dc_san_parse(text: *const c_char, len: usize, token: *mut u32) -> c_int;
        pub fn dc_pgn_parse_movetext(text: *const c_char, len: usize, tokens: *mut u32, stride: usize, cap: u32,
                                     n_tokens: *mut u32, result: *mut u8, first_fullmove: *mut u32,
                                     first_stm: *mut u8, consumed: *mut usize) -> c_int;
        pub fn dc_san_resolve(ctx: *mut dc_ctx, start: *const dc_pos, tokens: *const u32, n_games: u32,
                              n_plies: u32, moves: *mut u16, first_bad: *mut u32, counts: *mut u64) -> c_int;
        pub fn dc_san_resolve_device(ctx: *mut dc_ctx, start: *const dc_pos, d_tokens: *const u32, n_games: u32,
                                     n_plies: u32, d_moves: *mut u16, d_first_bad: *mut u32,
                                     counts: *mut u64) -> c_int;
        pub fn dc_san_resolve_starts(ctx: *mut dc_ctx, starts: *const dc_pos, tokens: *const u32, n_games: u32,
                                     n_plies: u32, moves: *mut u16, first_bad: *mut u32, counts: *mut u64,
                                     finals: *mut dc_pos) -> c_int;
        pub fn dc_san_resolve_starts_device(ctx: *mut dc_ctx, d_starts: *const dc_pos, d_tokens: *const u32,
                                            n_games: u32, n_plies: u32, d_moves: *mut u16, d_first_bad: *mut u32,
                                            counts: *mut u64, d_finals: *mut dc_pos) -> c_int;
        pub fn dc_replay_info(ctx: *mut dc_ctx, rules: u32, start: *const dc_pos, moves: *const u16, n_games: u32,
                              n_plies: u32, bitmap: *mut u64, digests: *mut u64, info: *mut u8,
                              stats: *mut dc_replay_stats) -> c_int;
        pub fn dc_replay_info_device(ctx: *mut dc_ctx, rules: u32, start: *const dc_pos, d_moves: *const u16,
                                     n_games: u32, n_plies: u32, d_bitmap: *mut u64, d_digests: *mut u64,
                                     d_info: *mut u8, stats: *mut dc_replay_stats) -> c_int;
        pub fn dc_history_append(history: *const c_char, moves: *const u16, info: *const u8, n_plies: u32,
                                 stride: usize, out: *mut c_char, out_cap: usize, out_len: *mut usize) -> c_int;
        pub fn dc_gen_games(ctx: *mut dc_ctx, rules: u32, seed: u64, first_game: u64, n_games: u32, n_plies: u32,
                            noise_per_256: u32, out: *mut u16) -> c_int;
        pub fn dc_gen_games_device(ctx: *mut dc_ctx, rules: u32, seed: u64, first_game: u64, n_games: u32,
                                   n_plies: u32, noise_per_256: u32, d_out: *mut u16) -> c_int;
        // state hash
        pub fn dc_keccak256(data: *const c_void, len: usize, out: *mut u8) -> c_int;
        pub fn dc_state_hash(ctx: *mut dc_ctx, start: *const dc_pos, history: *const c_char, names: *const c_char,
                             names_off: *const u32, moves: *const u16, n_games: u32, n_plies: u32,
                             hashes: *mut u8) -> c_int;
        pub fn dc_state_hash_device(ctx: *mut dc_ctx, start: *const dc_pos, history: *const c_char,
                                    d_names: *const c_char, d_names_off: *const u32, d_moves: *const u16,
                                    n_games: u32, n_plies: u32, d_hashes: *mut u8) -> c_int;
        // transaction signatures
        pub fn dc_verify_tx_batch(ctx: *mut dc_ctx, strings: *const c_char, str_off: *const u32,
                                  actions: *const u32, turns: *const i8, n: u32, verdicts: *mut u8) -> c_int;
        pub fn dc_verify_tx_batch_device(ctx: *mut dc_ctx, d_strings: *const c_char, d_str_off: *const u32,
                                         d_actions: *const u32, d_turns: *const i8, n: u32,
                                         d_verdicts: *mut u8) -> c_int;
        pub fn dc_sig_verdict_message(verdict: u8) -> *const c_char;
        // perft
        pub fn dc_perft(ctx: *mut dc_ctx, rules: u32, pos: *const dc_pos, depth: u32, divide: *mut u64,
                        root_moves: *mut u16, n_root: *mut u32, total: *mut u64) -> c_int;
        pub fn dc_perft_shard(ctx: *mut dc_ctx, rules: u32, pos: *const dc_pos, depth: u32, split_depth: u32,
                              shard: u32, n_shards: u32, divide: *mut u64, root_moves: *mut u16,
                              n_root: *mut u32, total: *mut u64) -> c_int;
        pub fn dc_perft_stats(ctx: *mut dc_ctx, rules: u32, pos: *const dc_pos, depth: u32, totals: *mut u64,
                              rows: *mut u64, root_moves: *mut u16, n_root: *mut u32) -> c_int;
        pub fn dc_perft_stats_shard(ctx: *mut dc_ctx, rules: u32, pos: *const dc_pos, depth: u32, split_depth: u32,
                                    shard: u32, n_shards: u32, totals: *mut u64, rows: *mut u64,
                                    root_moves: *mut u16, n_root: *mut u32) -> c_int;
        pub fn dc_perft_repeat_device(ctx: *mut dc_ctx, rules: u32, pos: *const dc_pos, depth: u32,
                                      split_depth: u32, shard: u32, n_shards: u32, n_runs: u32,
                                      d_out: *mut u64) -> c_int;
        pub fn dc_perft_batch(ctx: *mut dc_ctx, rules: u32, pos: *const dc_pos, n_pos: u32, depth: u32,
                              totals: *mut u64, divide: *mut u64, root_moves: *mut u16, root_pos: *mut u8,
                              n_root: *mut u32) -> c_int;
        pub fn dc_perft_batch_repeat_device(ctx: *mut dc_ctx, rules: u32, pos: *const dc_pos, n_pos: u32,
                                            depth: u32, split_depth: u32, n_runs: u32, d_out: *mut u64) -> c_int;
        pub fn dc_ctx_synchronize(ctx: *mut dc_ctx) -> c_int;
        // multi-GPU
        pub fn dc_multi_perft(devices: *const c_int, n_devices: c_int, rules: u32, pos: *const dc_pos, depth: u32,
                              divide: *mut u64, root_moves: *mut u16, n_root: *mut u32, total: *mut u64) -> c_int;
        pub fn dc_replay_shard_range(n_games: u64, shard: u32, n_shards: u32, first: *mut u64,
                                     count: *mut u64) -> c_int;
        pub fn dc_replay_scatter_shards(n_games: u64, n_shards: u32, n_plies: u32, gathered: *const u64,
                                        bitmap: *mut u64) -> c_int;
        pub fn dc_multi_replay(devices: *const c_int, n_devices: c_int, rules: u32, seed: u64, n_games: u64,
                               n_plies: u32, noise_per_256: u32, bitmap: *mut u64,
                               stats: *mut dc_replay_stats) -> c_int;
    }
}

/// A failed ABI call: the DC_E* status and its dc_strerror text.  Never a
/// rejected move -- that is a verdict (`Verdict`), not an error.
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct DcError {
    pub status: c_int,
    pub what: &'static str,
    pub text: String,
}

impl std::fmt::Display for DcError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "{}: {} ({})", self.what, self.text, self.status)
    }
}
impl std::error::Error for DcError {}

fn cstr(p: *const c_char) -> String {
    if p.is_null() {
        return String::new();
    }
    unsafe { CStr::from_ptr(p) }.to_string_lossy().into_owned()
}

fn check(status: c_int, what: &'static str) -> Result<(), DcError> {
    if status == sys::DC_SUCCESS {
        Ok(())
    } else {
        Err(DcError { status, what, text: cstr(unsafe { sys::dc_strerror(status) }) })
    }
}

/// The reference's rejection (core/src/chess.rs:82-125): Ok or the exact text
/// validate_move returns; OOR is the coordinate the reference would panic on.
#[derive(Clone, Debug, PartialEq, Eq)]
pub enum Verdict {
    Ok,
    Rejected(String),
    OutOfRange,
}

fn verdict(v: u8) -> Verdict {
    match v {
        sys::DC_V_OK => Verdict::Ok,
        sys::DC_V_OOR => Verdict::OutOfRange,
        _ => Verdict::Rejected(cstr(unsafe { sys::dc_verdict_message(v) })),
    }
}

/// One device context (one gfx950 GPU, one HIP stream).  Send but not Sync:
/// keep one per thread (e.g. a thread_local per tokio blocking worker).
pub struct Engine(*mut sys::dc_ctx);
unsafe impl Send for Engine {}

impl Engine {
    pub fn new(device: i32) -> Result<Self, DcError> {
        let mut c = std::ptr::null_mut();
        check(unsafe { sys::dc_ctx_create(device, &mut c) }, "dc_ctx_create")?;
        Ok(Engine(c))
    }

    pub fn raw(&self) -> *mut sys::dc_ctx {
        self.0
    }

    /// Opt-in resident validator for this context (dc_live_validator): calls of
    /// at most 64 moves skip the kernel launch while the lease lasts; 0 stops it.
    pub fn live_validator(&self, lease_us: u32) -> Result<(), DcError> {
        check(unsafe { sys::dc_live_validator(self.0, lease_us) }, "dc_live_validator")
    }

    /// validate_move (chess.rs:82) for one (from, to) pair: n = 1, the live consensus call.
    pub fn validate(&self, pos: &sys::dc_pos, from: (u32, u32), to: (u32, u32)) -> Result<Verdict, DcError> {
        let mv = unsafe { sys::dc_move_pack(from.0, from.1, to.0, to.1) };
        let mut v = 0u8;
        check(unsafe { sys::dc_validate_batch(self.0, sys::DC_RULES_REF, pos, &mv, 1, &mut v) },
              "dc_validate_batch")?;
        Ok(verdict(v))
    }

    /// A block's worth of checks at once (is_valid_tx over many transactions).
    pub fn validate_batch(&self, pos: &[sys::dc_pos], moves: &[u16]) -> Result<Vec<Verdict>, DcError> {
        if pos.len() != moves.len() || pos.len() > u32::MAX as usize {
            return Err(DcError { status: sys::DC_EINVAL, what: "validate_batch", text: "length mismatch".into() });
        }
        let mut v = vec![0u8; pos.len()];
        check(unsafe { sys::dc_validate_batch(self.0, sys::DC_RULES_REF, pos.as_ptr(), moves.as_ptr(),
                                              pos.len() as u32, v.as_mut_ptr()) }, "dc_validate_batch")?;
        Ok(v.into_iter().map(verdict).collect())
    }

    /// The legal moves and DC_ST_* status of every position (dc_legal_moves_batch):
    /// a sizing call, then a fill call.  Returns (offsets [n + 1], moves [total],
    /// status [n]); position i's moves are moves[offsets[i] .. offsets[i + 1]).
    pub fn legal_moves(&self, rules: u32, pos: &[sys::dc_pos]) -> Result<(Vec<u32>, Vec<u16>, Vec<u8>), DcError> {
        let n = u32::try_from(pos.len()).map_err(|_| DcError {
            status: sys::DC_EINVAL, what: "dc_legal_moves_batch", text: "more than u32::MAX positions".into() })?;
        let mut offsets = vec![0u32; pos.len() + 1];
        let mut status = vec![0u8; pos.len()];
        let mut total = 0u32;
        check(unsafe { sys::dc_legal_moves_batch(self.0, rules, pos.as_ptr(), n, offsets.as_mut_ptr(),
                                                 status.as_mut_ptr(), std::ptr::null_mut(), 0, &mut total) },
              "dc_legal_moves_batch")?;
        let mut moves = vec![0u16; total as usize];
        if total != 0 {
            check(unsafe { sys::dc_legal_moves_batch(self.0, rules, pos.as_ptr(), n, offsets.as_mut_ptr(),
                                                     status.as_mut_ptr(), moves.as_mut_ptr(), total, &mut total) },
                  "dc_legal_moves_batch")?;
        }
        Ok((offsets, moves, status))
    }

    /// apply_move (chess.rs:43-80) on the cells of a proto board: validates,
    /// makes the move on the GPU, updates `turn` and appends the history entry
    /// (update_history, chess.rs:127-184, via dc_history_append).  A rejected
    /// move leaves everything untouched and returns its verdict.  Cells of kind
    /// OTHER (6) never move (chess.rs:210), so the caller's kind strings for
    /// them stay valid.
    pub fn apply_move(&self, cells: &mut [i8; 64], turn: &mut u8, history: &mut String, from: (u32, u32),
                      to: (u32, u32)) -> Result<Verdict, DcError> {
        let mut pos = sys::dc_pos::default();
        check(unsafe { sys::dc_pos_from_cells(cells.as_ptr(), *turn, &mut pos) }, "dc_pos_from_cells")?;
        let mv = unsafe { sys::dc_move_pack(from.0, from.1, to.0, to.1) };
        let (mut v, mut info) = (0u8, 0u8);
        check(unsafe { sys::dc_apply_batch(self.0, sys::DC_RULES_REF, &mut pos, &mv, 1, &mut v, &mut info) },
              "dc_apply_batch")?;
        if v != sys::DC_V_OK {
            return Ok(verdict(v));
        }
        let h = history_append(history, &[mv], &[info])?;
        check(unsafe { sys::dc_pos_to_cells(&pos, cells.as_mut_ptr(), turn) }, "dc_pos_to_cells")?;
        *history = h;
        Ok(Verdict::Ok)
    }

    /// Resync: replay a game's committed moves in one call; returns the per-ply
    /// info bytes (0xFF = rejected) and the counters.
    pub fn replay_info(&self, moves: &[u16]) -> Result<(Vec<u8>, sys::dc_replay_stats), DcError> {
        // n_plies is a u32 at the ABI: a longer log is an error, never truncated
        let n_plies = u32::try_from(moves.len()).map_err(|_| DcError {
            status: sys::DC_EINVAL, what: "dc_replay_info", text: "move log longer than u32::MAX plies".into() })?;
        let mut info = vec![0u8; moves.len()];
        let mut st = sys::dc_replay_stats::default();
        check(unsafe { sys::dc_replay_info(self.0, sys::DC_RULES_REF, std::ptr::null(), moves.as_ptr(), 1,
                                           n_plies, std::ptr::null_mut(), std::ptr::null_mut(),
                                           info.as_mut_ptr(), &mut st) }, "dc_replay_info")?;
        Ok((info, st))
    }

    /// Adjudicates one game's move log under the standard rules before a vote
    /// (dc_replay_outcome, n_games = 1): where the game ended and how, and the
    /// counters of the plies up to there.  Plies at or past `end_ply` of a
    /// finished game belong to no game: the caller rejects them.
    pub fn replay_outcome(&self, start: Option<&sys::dc_pos>, start_halfmove: u32, moves: &[u16])
                          -> Result<(sys::dc_game_outcome, sys::dc_replay_stats), DcError> {
        let n_plies = u32::try_from(moves.len()).map_err(|_| DcError {
            status: sys::DC_EINVAL, what: "dc_replay_outcome", text: "move log longer than u32::MAX plies".into() })?;
        let mut out = sys::dc_game_outcome::default();
        let mut st = sys::dc_replay_stats::default();
        let sp = start.map_or(std::ptr::null(), |p| p as *const sys::dc_pos);
        check(unsafe { sys::dc_replay_outcome(self.0, sp, start_halfmove, moves.as_ptr(), 1, n_plies,
                                              &mut out as *mut sys::dc_game_outcome as *mut c_void,
                                              std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(),
                                              &mut st) }, "dc_replay_outcome")?;
        Ok((out, st))
    }

    /// A batch of games that each begin at their own position with their own
    /// half-move clock (dc_replay_outcome_starts): `moves` is ply-major
    /// [n_plies][n_games], n_games = starts.len() = start_halfmoves.len().
    /// Returns every game's outcome and the position it stopped in, which with
    /// the outcome's halfmove continues the game in a later call.
    pub fn replay_outcome_starts(&self, starts: &[sys::dc_pos], start_halfmoves: &[u16], moves: &[u16])
                                 -> Result<(Vec<sys::dc_game_outcome>, Vec<sys::dc_pos>), DcError> {
        let bad = |text: &str| DcError { status: sys::DC_EINVAL, what: "dc_replay_outcome_starts", text: text.into() };
        let n_games = u32::try_from(starts.len()).map_err(|_| bad("more than u32::MAX games"))?;
        if start_halfmoves.len() != starts.len() { return Err(bad("one clock per start")); }
        if n_games == 0 { return Ok((Vec::new(), Vec::new())); }
        if moves.len() % starts.len() != 0 { return Err(bad("moves is not [n_plies][n_games]")); }
        let n_plies = u32::try_from(moves.len() / starts.len()).map_err(|_| bad("more than u32::MAX plies"))?;
        let mut out = vec![sys::dc_game_outcome::default(); starts.len()];
        let mut finals = starts.to_vec();
        check(unsafe { sys::dc_replay_outcome_starts(self.0, starts.as_ptr(), start_halfmoves.as_ptr(),
                                                     moves.as_ptr(), n_games, n_plies,
                                                     out.as_mut_ptr() as *mut c_void, std::ptr::null_mut(),
                                                     std::ptr::null_mut(), std::ptr::null_mut(),
                                                     std::ptr::null_mut(), finals.as_mut_ptr()) },
              "dc_replay_outcome_starts")?;
        Ok((out, finals))
    }

    /// One game's move log under the standard rules as PGN movetext
    /// (dc_replay_san, n_games = 1, then dc_pgn_movetext): the resync path's
    /// move text, the FIDE counterpart of replay_info + history_append.  The
    /// first move is numbered `first_fullmove`; the side to move is the start
    /// position's (White for the start position).
    pub fn replay_pgn(&self, start: Option<&sys::dc_pos>, start_halfmove: u32, first_fullmove: u32, moves: &[u16])
                      -> Result<(sys::dc_game_outcome, String), DcError> {
        let n_plies = u32::try_from(moves.len()).map_err(|_| DcError {
            status: sys::DC_EINVAL, what: "dc_replay_san", text: "move log longer than u32::MAX plies".into() })?;
        let mut out = sys::dc_game_outcome::default();
        let mut san = vec![0xFFu8; moves.len().max(1)];
        let sp = start.map_or(std::ptr::null(), |p| p as *const sys::dc_pos);
        check(unsafe { sys::dc_replay_san(self.0, sp, start_halfmove, moves.as_ptr(), 1, n_plies,
                                          &mut out as *mut sys::dc_game_outcome as *mut c_void, san.as_mut_ptr(),
                                          std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(),
                                          std::ptr::null_mut()) }, "dc_replay_san")?;
        let stm = start.map_or(0, |p| p.stm);
        let text = pgn_movetext(moves, &san[..moves.len()], first_fullmove, stm, out.result)?;
        Ok((out, text))
    }

    /// One game's SAN tokens (parse_movetext's) as move words (dc_san_resolve,
    /// n_games = 1): (moves, the first ply with a flagged word or the number of
    /// plies, the DC_SR_* counters).  A token no single legal move fits gives
    /// DC_MOVE_NOMATCH / _AMBIGUOUS / _MALFORMED there and leaves the position.
    pub fn resolve_san(&self, start: Option<&sys::dc_pos>, tokens: &[u32])
                       -> Result<(Vec<u16>, u32, [u64; sys::DC_SR_COUNT]), DcError> {
        let n_plies = u32::try_from(tokens.len()).map_err(|_| DcError {
            status: sys::DC_EINVAL, what: "dc_san_resolve", text: "more than u32::MAX tokens".into() })?;
        let mut moves = vec![sys::DC_MOVE_NONE; tokens.len()];
        let mut first_bad = 0u32;
        let mut counts = [0u64; sys::DC_SR_COUNT];
        let sp = start.map_or(std::ptr::null(), |p| p as *const sys::dc_pos);
        check(unsafe { sys::dc_san_resolve(self.0, sp, tokens.as_ptr(), 1, n_plies, moves.as_mut_ptr(),
                                           &mut first_bad, counts.as_mut_ptr()) }, "dc_san_resolve")?;
        Ok((moves, first_bad, counts))
    }

    /// The published perft tables' columns for one position (dc_perft_stats_shard;
    /// split_depth 1, shard 0 of 1 is the whole tree).  Returns (totals, one row
    /// of DC_PS_COUNT counters per root move, the root moves).
    pub fn perft_stats(&self, rules: u32, pos: &sys::dc_pos, depth: u32, split_depth: u32, shard: u32, n_shards: u32)
                       -> Result<([u64; sys::DC_PS_COUNT], Vec<[u64; sys::DC_PS_COUNT]>, Vec<u16>), DcError> {
        let mut totals = [0u64; sys::DC_PS_COUNT];
        let mut rows = vec![[0u64; sys::DC_PS_COUNT]; 256];
        let mut root_moves = vec![0u16; 256];
        let mut n_root = 0u32;
        check(unsafe { sys::dc_perft_stats_shard(self.0, rules, pos, depth, split_depth, shard, n_shards,
                                                 totals.as_mut_ptr(), rows.as_mut_ptr() as *mut u64,
                                                 root_moves.as_mut_ptr(), &mut n_root) }, "dc_perft_stats_shard")?;
        let n = (n_root as usize).min(256);
        rows.truncate(n);
        root_moves.truncate(n);
        Ok((totals, rows, root_moves))
    }
}

impl Drop for Engine {
    fn drop(&mut self) {
        let _ = unsafe { sys::dc_ctx_destroy(self.0) };
    }
}

/// update_history over plies (dc_history_append, host only): no panic on any input.
pub fn history_append(history: &str, moves: &[u16], info: &[u8]) -> Result<String, DcError> {
    if moves.len() != info.len() {
        return Err(DcError { status: sys::DC_EINVAL, what: "history_append", text: "length mismatch".into() });
    }
    let h = CString::new(history)
        .map_err(|_| DcError { status: sys::DC_EINVAL, what: "history_append", text: "NUL in history".into() })?;
    let mut len = 0usize;
    check(unsafe { sys::dc_history_append(h.as_ptr(), moves.as_ptr(), info.as_ptr(), moves.len() as u32, 1,
                                          std::ptr::null_mut(), 0, &mut len) }, "dc_history_append")?;
    let mut out = vec![0u8; len + 1];
    check(unsafe { sys::dc_history_append(h.as_ptr(), moves.as_ptr(), info.as_ptr(), moves.len() as u32, 1,
                                          out.as_mut_ptr() as *mut c_char, out.len(), &mut len) },
          "dc_history_append")?;
    out.truncate(len);
    String::from_utf8(out)
        .map_err(|_| DcError { status: sys::DC_EINVAL, what: "history_append", text: "not UTF-8".into() })
}

/// (half-move clock, full-move number) of a FEN (dc_fen_clocks, host only).
pub fn fen_clocks(fen: &str) -> Result<(u32, u32), DcError> {
    let f = CString::new(fen)
        .map_err(|_| DcError { status: sys::DC_EINVAL, what: "fen_clocks", text: "NUL in FEN".into() })?;
    let (mut hm, mut fm) = (0u32, 0u32);
    check(unsafe { sys::dc_fen_clocks(f.as_ptr(), &mut hm, &mut fm) }, "dc_fen_clocks")?;
    Ok((hm, fm))
}

fn text_of(mut out: Vec<u8>, len: usize, what: &'static str) -> Result<String, DcError> {
    out.truncate(len);
    String::from_utf8(out).map_err(|_| DcError { status: sys::DC_EINVAL, what, text: "not UTF-8".into() })
}

/// The SAN token of one accepted move (dc_san_format, host only).
pub fn san_format(mv: u16, san: u8) -> Result<String, DcError> {
    let mut out = vec![0u8; 8];
    check(unsafe { sys::dc_san_format(mv, san, out.as_mut_ptr() as *mut c_char) }, "dc_san_format")?;
    let len = out.iter().position(|&c| c == 0).unwrap_or(7);
    text_of(out, len, "san_format")
}

/// One game's PGN movetext from its moves and SAN bytes (dc_pgn_movetext, host only).
pub fn pgn_movetext(moves: &[u16], san: &[u8], first_fullmove: u32, first_stm: u8, result: u8)
                    -> Result<String, DcError> {
    let n_plies = u32::try_from(moves.len()).ok().filter(|_| moves.len() == san.len()).ok_or_else(|| DcError {
        status: sys::DC_EINVAL, what: "pgn_movetext", text: "length mismatch".into() })?;
    let mut len = 0usize;
    check(unsafe { sys::dc_pgn_movetext(moves.as_ptr(), san.as_ptr(), n_plies, 1, first_fullmove, first_stm, result,
                                        std::ptr::null_mut(), 0, &mut len) }, "dc_pgn_movetext")?;
    let mut out = vec![0u8; len + 1];
    check(unsafe { sys::dc_pgn_movetext(moves.as_ptr(), san.as_ptr(), n_plies, 1, first_fullmove, first_stm, result,
                                        out.as_mut_ptr() as *mut c_char, out.len(), &mut len) }, "dc_pgn_movetext")?;
    text_of(out, len, "pgn_movetext")
}

/// One SAN token ("Nbd2", "exd8=Q+", "O-O") as its token word (dc_san_parse, host only).
pub fn san_parse(text: &str) -> Result<u32, DcError> {
    let mut token = 0u32;
    check(unsafe { sys::dc_san_parse(text.as_ptr() as *const c_char, text.len(), &mut token) }, "dc_san_parse")?;
    Ok(token)
}

/// One game's movetext read by dc_pgn_parse_movetext (host only).
#[derive(Clone, Debug, Default, PartialEq, Eq)]
pub struct Movetext {
    pub tokens: Vec<u32>,
    /// 0 "*" or none, 1 "1-0", 2 "0-1", DC_PGN_DRAW "1/2-1/2"
    pub result: u8,
    pub first_fullmove: u32,
    pub first_stm: u8,
    /// bytes read through the result token: the next game begins there
    pub consumed: usize,
}

/// Parses one game's movetext; on a word that is no SAN token the error's text
/// names the byte offset of that word.
pub fn parse_movetext(text: &str) -> Result<Movetext, DcError> {
    let p = text.as_ptr() as *const c_char;
    let mut m = Movetext::default();
    let mut n = 0u32;
    let st = unsafe { sys::dc_pgn_parse_movetext(p, text.len(), std::ptr::null_mut(), 1, 0, &mut n, &mut m.result,
                                                 &mut m.first_fullmove, &mut m.first_stm, &mut m.consumed) };
    if st != sys::DC_SUCCESS {
        return Err(DcError { status: st, what: "dc_pgn_parse_movetext",
                             text: format!("no SAN token at byte {}", m.consumed) });
    }
    m.tokens = vec![sys::DC_SAN_TOKEN_NONE; n as usize];
    if n > 0 {
        check(unsafe { sys::dc_pgn_parse_movetext(p, text.len(), m.tokens.as_mut_ptr(), 1, n, &mut n, &mut m.result,
                                                  &mut m.first_fullmove, &mut m.first_stm, &mut m.consumed) },
              "dc_pgn_parse_movetext")?;
    }
    Ok(m)
}

/// The FEN of a position (dc_pos_to_fen, host only).
pub fn pos_to_fen(pos: &sys::dc_pos, halfmove: u32, fullmove: u32) -> Result<String, DcError> {
    let mut len = 0usize;
    check(unsafe { sys::dc_pos_to_fen(pos, halfmove, fullmove, std::ptr::null_mut(), 0, &mut len) }, "dc_pos_to_fen")?;
    let mut out = vec![0u8; len + 1];
    check(unsafe { sys::dc_pos_to_fen(pos, halfmove, fullmove, out.as_mut_ptr() as *mut c_char, out.len(), &mut len) },
          "dc_pos_to_fen")?;
    text_of(out, len, "pos_to_fen")
}

/// keccak256 (alloy) of one byte string, on the host.
pub fn keccak256(data: &[u8]) -> Result<[u8; 32], DcError> {
    let mut out = [0u8; 32];
    check(unsafe { sys::dc_keccak256(data.as_ptr() as *const c_void, data.len(), out.as_mut_ptr()) },
          "dc_keccak256")?;
    Ok(out)
}
