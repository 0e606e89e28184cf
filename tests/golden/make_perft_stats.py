"""Regenerates tests/golden/perft_stats.json, the expected values of dc_perft_stats.

Run:  python tests/golden/make_perft_stats.py   (about a minute on 8 cores)

Every value comes from the oracle: moves from fastcpu (gen_moves, make), each
leaf move classified by the mailbox attack walk of tests/cpp/perft_stats_oracle.cpp,
which this script compiles (the binary stays out of git).  Before anything is
written the totals are checked against PINS below -- the published perft tables
wherever those carry the column.
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
sys.path.insert(0, HERE)
import oracle_lib as O  # noqa: E402
from make_golden import FIDE_SUITE  # noqa: E402

NAMES = ("nodes", "captures", "ep", "castles", "promotions", "checks", "discovered", "double", "checkmates",
         "stalemates", "king_captures")

# (position, depth): nodes / captures / e.p. / castles / promotions / checks / discovered / double / mates
PINS = {
    ("startpos", 3): (8902, 34, 0, 0, 0, 12, 0, 0, 0),
    ("startpos", 4): (197281, 1576, 0, 0, 0, 469, 0, 0, 8),
    ("startpos", 5): (4865609, 82719, 258, 0, 0, 27351, 6, 0, 347),
    ("kiwipete", 1): (48, 8, 0, 2, 0, 0, 0, 0, 0),
    ("kiwipete", 2): (2039, 351, 1, 91, 0, 3, 0, 0, 0),
    ("kiwipete", 3): (97862, 17102, 45, 3162, 0, 993, 0, 0, 1),
    ("kiwipete", 4): (4085603, 757163, 1929, 128013, 15172, 25523, 42, 6, 43),
    ("pos3", 3): (2812, 209, 2, 0, 0, 267, 3, 0, 0),
    ("pos3", 4): (43238, 3348, 123, 0, 0, 1680, 106, 0, 17),
    ("pos3", 5): (674624, 52051, 1165, 0, 0, 52950, 1292, 3, 0),
    ("pos4", 2): (264, 87, 0, 6, 48, 10, 0, 0, 0),
    ("pos4", 3): (9467, 1021, 4, 0, 120, 38, 2, 0, 22),
    ("pos4", 4): (422333, 131393, 0, 7795, 60032, 15492, 19, 0, 5),
    ("pos5", 3): (62379, 8517, 0, 1081, 5068, 1201, 0, 0, 44),
    ("pos5", 4): (2103487, 296153, 0, 0, 0, 158486, 10877, 1770, 240),
    ("pos6", 3): (89890, 9470, 0, 0, 0, 1783, 0, 0, 0),
    ("pos6", 4): (3894594, 440388, 0, 0, 0, 68985, 62, 20, 0),
}
SUITE_DEPTH = {"startpos": 5, "kiwipete": 4, "pos3": 5, "pos4": 4, "pos5": 4, "pos6": 4}
SUITE_ROWS = {("kiwipete", 3), ("pos4", 3)}  # per-root rows kept for these

# small positions that reach every rare branch within depth 3 (rows at depths 1 to 3)
SMALL = [
    "7k/5Q2/8/8/8/8/8/K7 w - - 0 1",
    "5k2/8/8/8/8/8/8/4K2R w K - 0 1",
    "8/8/8/R2pP2k/8/8/8/4K3 w - d6 0 1",
    "4k3/8/4N3/8/8/8/8/4RK2 w - - 0 1",
    "4k3/P7/8/8/8/8/8/4K3 w - - 0 1",
    "r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1",
    "n1n5/PPPk4/8/8/8/8/4Kppp/5N1N b - - 0 1",
]
# FEN -> depth -> {counter: value}
SMALL_PINS = {
    SMALL[0]: {1: {"nodes": 26, "checks": 7, "stalemates": 4}},
    SMALL[1]: {1: {"castles": 1, "checks": 3, "discovered": 0}},
    SMALL[2]: {1: {"ep": 1, "checks": 1, "discovered": 1}},
    SMALL[3]: {1: {"nodes": 20, "checks": 8, "discovered": 6, "double": 2}},
    SMALL[4]: {1: {"promotions": 4, "checks": 2}, 3: {"promotions": 100}},
    SMALL[5]: {2: {"castles": 42}, 3: {"nodes": 13744, "castles": 324, "checkmates": 10}},
    SMALL[6]: {1: {"nodes": 24, "captures": 11, "promotions": 12, "checks": 3}, 3: {"promotions": 3224}},
}
# REF (position, depth): nodes / captures / king captures
REF_PINS = {
    ("startpos", 4): (197742, 1579, 0),
    ("startpos", 5): (4896998, 83678, 461),
    ("kiwipete", 3): (87218, 15682, 5),
    ("kiwipete", 4): (3570807, 677272, 398),
}
N_RANDOM = 8  # of oracle_golden.json's perft_ref random_positions


def build_oracle():
    out_dir = os.path.join(TESTS, "cpp", "build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "perft_stats_oracle")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(TESTS, "cpp", "perft_stats_oracle.cpp"),
                           os.path.join(REPO, "oracle", "fastcpu.cpp"), "-o", exe])
    return exe


class Oracle:
    def __init__(self):
        self.proc = subprocess.Popen([build_oracle()], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def stats(self, pos, depth, rules):
        """-> (totals[11], root moves, rows[n_root][11])"""
        req = [int(rules), int(depth), pos.stm, pos.castle, pos.ep] + [int(c) for c in pos.cells]
        self.proc.stdin.write(" ".join(map(str, req)) + "\n")
        self.proc.stdin.flush()
        f = [int(x) for x in self.proc.stdout.readline().split()]
        n = f[0]
        assert len(f) == 1 + 12 * n, (len(f), n)
        moves = [f[1 + 12 * i] for i in range(n)]
        rows = [f[2 + 12 * i:13 + 12 * i] for i in range(n)]
        totals = [sum(r[k] for r in rows) for k in range(11)]
        return totals, moves, rows

    def close(self):
        self.proc.stdin.close()
        self.proc.wait()


def entry(totals, moves=None, rows=None):
    e = {"totals": totals}
    if rows is not None:
        e["moves"], e["rows"] = moves, rows
    return e


def main():
    orc = Oracle()
    out = {"names": list(NAMES)}
    # ------------------------------------------------------- FIDE: the suite
    fide = {}
    for name, (fen, _) in FIDE_SUITE.items():
        p = O.Pos.from_fen(fen)
        per = {}
        for d in range(1, SUITE_DEPTH[name] + 1):
            tot, mv, rows = orc.stats(p, d, O.FIDE)
            if (name, d) in PINS:
                assert tuple(tot[:9]) == PINS[(name, d)], (name, d, tot)
            assert tot[10] == 0
            per[str(d)] = entry(tot, mv, rows) if (name, d) in SUITE_ROWS else entry(tot)
            print("FIDE", name, d, tot)
        fide[name] = {"fen": fen, "depths": per}
    assert all(k[0] in fide and str(k[1]) in fide[k[0]]["depths"] for k in PINS)
    out["fide_suite"] = fide
    # --------------------------------------------- FIDE: the small positions
    small = []
    for fen in SMALL:
        p = O.Pos.from_fen(fen)
        per = {}
        for d in (1, 2, 3):
            tot, mv, rows = orc.stats(p, d, O.FIDE)
            for k, v in SMALL_PINS[fen].get(d, {}).items():
                assert tot[NAMES.index(k)] == v, (fen, d, k, tot)
            per[str(d)] = entry(tot, mv, rows)
            print("FIDE", fen, d, tot)
        small.append({"fen": fen, "depths": per})
    out["fide_small"] = small
    # ------------------------------------------------------------------ REF
    og = json.load(open(os.path.join(HERE, "oracle_golden.json")))
    ref = {}
    for name, depths in (("startpos", (3, 4, 5)), ("kiwipete", (3, 4))):
        p = O.Pos.from_fen(FIDE_SUITE[name][0])
        p.castle, p.ep = 0, -1  # the reference has neither
        per = {}
        for d in depths:
            tot, mv, rows = orc.stats(p, d, O.REF)
            if (name, d) in REF_PINS:
                assert (tot[0], tot[1], tot[10]) == REF_PINS[(name, d)], (name, d, tot)
            assert not any(tot[2:10])
            per[str(d)] = entry(tot, mv, rows) if (name, d) == ("startpos", 3) else entry(tot)
            print("REF", name, d, tot)
        ref[name] = {"fen": FIDE_SUITE[name][0], "depths": per}
    out["ref_suite"] = ref
    rnd = []
    for i, e in enumerate(og["perft_ref"]["random_positions"][:N_RANDOM]):
        p = O.Pos(np.array(e["cells"], np.int8), e["stm"])
        per = {}
        for d in (1, 2, 3):
            tot, mv, rows = orc.stats(p, d, O.REF)
            assert tot[0] == e["perft"][str(d)], (i, d, tot)
            per[str(d)] = entry(tot, mv, rows)
        rnd.append({"index": i, "depths": per})
    out["ref_random"] = rnd
    orc.close()
    with open(os.path.join(HERE, "perft_stats.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote perft_stats.json")


if __name__ == "__main__":
    main()
