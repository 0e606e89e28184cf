#!/usr/bin/env python3
"""Adjudicates seeded games and prints how they ended.

Generates `--games` games of `--plies` plies with dc_gen_games under the
standard rules (seed, noise as dc_gen_games), adjudicates them with
dc_replay_outcome and prints the result histogram, then the per-kernel time of
the adjudicating replay ("replay_outcome") beside the plain FIDE replay's
(k_replay_fide, timing name "replay") on the same moves.  Everything stays on
the device; only the counters come back.

    python tools/game_outcomes.py --seed 2024 --games 1000000 --plies 200 --noise 32
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-chess_amd"))

import dchess  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=2024)
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--plies", type=int, default=200)
    ap.add_argument("--noise", type=int, default=32, help="junk moves per 256 plies")
    ap.add_argument("--reps", type=int, default=3, help="timed repetitions of each replay")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    eng = dchess.Engine(a.device)
    n, plies = a.games, a.plies
    words = (n + 63) // 64
    d_moves = eng.alloc(max(2 * n * plies, 1))
    d_out = eng.alloc(max(8 * n, 1))
    d_bitmap = eng.alloc(max(8 * words * plies, 1))
    d_digests = eng.alloc(max(8 * n, 1))
    eng.gen_games_device(d_moves, a.seed, 0, n, plies, a.noise, dchess.RULES_FIDE)

    # one untimed pass of each (buffers grow, code objects load), then the timed ones
    counts, st = eng.replay_outcome_device(d_moves, n, plies, d_out, d_bitmap, d_digests)
    plain = eng.replay_device(d_moves, n, plies, d_bitmap, d_digests, rules=dchess.RULES_FIDE)
    eng.set_profiling(True)
    eng.reset_stats()
    for _ in range(a.reps):
        eng.replay_outcome_device(d_moves, n, plies, d_out, d_bitmap, d_digests)
        eng.replay_device(d_moves, n, plies, d_bitmap, d_digests, rules=dchess.RULES_FIDE)
    ko, kr = eng.kernel_stats("replay_outcome"), eng.kernel_stats("replay")
    eng.set_profiling(False)

    print(f"{n} games x {plies} plies, seed {a.seed}, noise {a.noise}/256")
    for k, name in enumerate(dchess.GO_NAMES):
        print(f"  {name:12s} {int(counts[k]):10d}  {100.0 * int(counts[k]) / max(n, 1):6.2f} %")
    print(f"  moves consumed {st['validated']} (accepted {st['accepted']}, rejected {st['rejected']}); "
          f"plain replay validates {plain['validated']}")
    ms_o, ms_r = ko["total_ms"] / max(a.reps, 1), kr["total_ms"] / max(a.reps, 1)
    print(f"  replay_outcome {ms_o:9.3f} ms per batch ({ko['launches'] // max(a.reps, 1)} launches)")
    print(f"  k_replay_fide  {ms_r:9.3f} ms per batch")
    print(json.dumps({"games": n, "plies": plies, "seed": a.seed, "noise": a.noise,
                      "counts": {name: int(counts[k]) for k, name in enumerate(dchess.GO_NAMES)},
                      "consumed": st["validated"], "replay_outcome_ms": round(ms_o, 3), "replay_fide_ms": round(ms_r, 3)}))
    eng.close()


if __name__ == "__main__":
    main()
