#!/usr/bin/env python3
"""Prints the perft table of a position (dc_perft_stats): one line per depth,
the counters in the published tables' column order.

  tools/perft_stats.py startpos 5
  tools/perft_stats.py "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq -" 4 --divide
  tools/perft_stats.py startpos 6 --rules ref
  tools/perft_stats.py startpos 6 --min-depth 5 --time --perft

--time repeats each depth's call with profiling on and prints HIP-event times
per call: `call` = the sum over the call's kernels, `leaf` = k_leaf_stats alone;
--perft adds dc_perft's kernels at the same depth and at depth + 1 (counting the
replies to every leaf is the work of perft(depth + 1)'s last ply).
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-chess_amd"))

import dchess  # noqa: E402

# every timing name a perft or perft-statistics call can launch under
KERNELS = ("expand_top", "front", "expand_count", "scan", "expand_write", "level_moves", "count1", "count2", "dfs",
           "fold", "leaf_stats")


def kernel_ms(eng, fn, reps):
    """Mean HIP-event milliseconds per call of fn(), per timing name."""
    fn()  # buffers sized, code loaded
    eng.set_profiling(True)
    eng.reset_stats()
    for _ in range(reps):
        fn()
    ms = {k: eng.kernel_stats(k)["total_ms"] / reps for k in KERNELS}
    eng.set_profiling(False)
    eng.reset_stats()
    return ms


def move_name(m):
    sq = lambda s: "abcdefgh"[s & 7] + str((s >> 3) + 1)  # noqa: E731
    return sq(m & 63) + sq((m >> 6) & 63) + " nbrq"[(m >> 12) & 7].strip()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("position", help="a FEN, or `startpos`")
    ap.add_argument("depth", type=int)
    ap.add_argument("--min-depth", type=int, default=1)
    ap.add_argument("--rules", choices=("fide", "ref"), default="fide")
    ap.add_argument("--divide", action="store_true", help="also one line per root move at the last depth")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--perft", action="store_true", help="with --time: dc_perft at depth and depth + 1 beside it")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rules = dchess.RULES_FIDE if a.rules == "fide" else dchess.RULES_REF
    pos = dchess.startpos() if a.position == "startpos" else dchess.pos_from_fen(a.position)
    eng = dchess.Engine(0)
    head = "depth " + " ".join(f"{n:>13}" for n in dchess.PS_NAMES)
    if a.time:
        head += "     call_ms     leaf_ms" + ("  perft(d)_ms perft(d+1)_ms" if a.perft else "")
    print(head)
    for d in range(a.min_depth, a.depth + 1):
        tot, rows, rm = eng.perft_stats(pos, d, rules)
        line = f"{d:>5} " + " ".join(f"{int(v):>13}" for v in tot)
        if a.time:
            ms = kernel_ms(eng, lambda: eng.perft_stats(pos, d, rules), a.reps)
            line += f" {sum(ms.values()):>11.4f} {ms['leaf_stats']:>11.4f}"
            if a.perft:
                for dd in (d, d + 1):
                    line += f" {sum(kernel_ms(eng, lambda: eng.perft(pos, dd, rules), a.reps).values()):>12.4f}"
        print(line, flush=True)
    if a.divide:
        for m, r in zip(rm.tolist(), rows):
            print(f"{move_name(m):>5} " + " ".join(f"{int(v):>13}" for v in r))
    eng.close()


if __name__ == "__main__":
    main()
