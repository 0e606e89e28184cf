"""The launch sequence of every perft and perft-statistics path, pinned.

With profiling on, a context counts the launches under each timing name
(dchess.h: dc_ctx_kernel_stats) and replays no captured graph, so one call
shows the plain enqueue path's sequence: how often the top kernel, the level
kernels (expand_count, scan, expand_write), the fused stage (level_moves,
count2), count1, K4 (dfs), the one-launch front end (front, fold) and
leaf_stats ran.  A call that takes the exact rerun adds its launches to the
speculative run's.  Both are deterministic.

EXPECTED was recorded from the library as it stood before the level chain of
dc_api_perft.hip and the launch dispatch of dc_perft.hip were restructured
(`python tests/test_gpu_perft_sequence.py` prints the table from whatever
library DCHESS_LIB names): a change of the host side that alters a path's
launches fails here, whatever the totals say.  The totals are checked against
the goldens the other modules use.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dchess
import oracle_lib as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OG = json.load(open(os.path.join(HERE, "golden", "oracle_golden.json")))
PS = json.load(open(os.path.join(HERE, "golden", "perft_stats.json")))
REF, FIDE = dchess.RULES_REF, dchess.RULES_FIDE
RULES = {"ref": REF, "fide": FIDE}

NAMES = ("expand_top", "expand_count", "scan", "expand_write", "level_moves", "count2", "count1", "dfs", "front",
         "fold", "leaf_stats")
KNOBS = ("DCHESS_PERFT_K4", "DCHESS_PERFT_WIDE_MAX", "DCHESS_PERFT_WIDE_LEVEL_MAX")

# the sparse positions of test_gpu_dfs.py (their totals: fastcpu, in the test)
ROOK, KNIGHT_B, KINGS, KINGS_B, KINGS_10 = ("4k3/8/8/8/8/8/8/R3K3 w - - 0 1", "7k/8/8/8/3N4/8/8/K7 b - - 0 1",
                                            "7k/8/8/8/8/8/8/K7 w - - 0 1", "8/8/2k5/8/8/5K2/8/8 b - - 0 1",
                                            "k7/8/8/8/8/8/8/7K w - - 0 1")


def suite_fen(name):
    return OG["perft_fide"][name]["fen"]


def suite_total(name, depth, rules):
    if rules == FIDE:
        return OG["perft_fide"][name]["perft"][str(depth)]
    return OG["perft_ref"]["suite"][name]["perft"][str(depth)]


# A case: (id, kind, rules, position(s), depth, (split, n_shards), environment, level cap).
# kind "perft": the shards' totals sum to the golden; "batch": per position;
# "stats": the shards' counters sum to the golden's.
def _cases():
    out = []
    # 1: no final stage; 2: count1; 3-5: the top kernel reaches the final stage's level; 6, 7: front (7: + fold)
    for d in range(1, 8):
        out.append((f"ref-startpos-d{d}", "perft", "ref", "startpos", d, (1, 1), {}, 0))
    out += [
        ("ref-d5-split2-of3", "perft", "ref", "startpos", 5, (2, 3), {}, 0),  # shard_words, S == T
        ("ref-d5-split4-of5", "perft", "ref", "startpos", 5, (4, 5), {}, 0),  # S == F: no fused stage, gathered
        ("ref-d6-split3-of2", "perft", "ref", "startpos", 6, (3, 2), {}, 0),  # the front end's strided shard
        ("ref-d7-split5-of3", "perft", "ref", "startpos", 7, (5, 3), {}, 0),  # the legacy chain below a shard cut
        ("fide-kiwipete-d3", "perft", "fide", "kiwipete", 3, (1, 1), {}, 0),
        ("fide-kiwipete-d4", "perft", "fide", "kiwipete", 4, (1, 1), {}, 0),
        ("fide-kiwipete-d5", "perft", "fide", "kiwipete", 5, (1, 1), {}, 0),  # the short top
        ("fide-kiwipete-d5-split3-of3", "perft", "fide", "kiwipete", 5, (3, 3), {}, 0),
        ("batch-ref-d4", "batch", "ref", ("kiwipete", "pos4"), 4, (1, 1), {}, 0),
        ("batch-fide-d4", "batch", "fide", ("kiwipete", "pos4"), 4, (1, 1), {}, 0),
        # depth 8: 64-bit move words below ply 5, or K4 (L = 1); depth 9: the sliced stage, or K4 (L = 2); 10: L = 3
        ("wide-d8", "perft", "ref", ROOK, 8, (1, 1), {}, 0),
        ("sliced-d9", "perft", "ref", KINGS, 9, (1, 1), {}, 0),
        ("k4-d8", "perft", "ref", ROOK, 8, (1, 1), {"DCHESS_PERFT_K4": "1"}, 0),
        ("k4-d8-black", "perft", "ref", KNIGHT_B, 8, (1, 1), {"DCHESS_PERFT_K4": "1"}, 0),
        ("k4-d9", "perft", "ref", KINGS_B, 9, (1, 1), {"DCHESS_PERFT_K4": "1"}, 0),
        ("k4-d10", "perft", "ref", KINGS_10, 10, (1, 1), {}, 0),
        # the exact rerun's fallbacks to K4: too many words, too large a sliced level
        ("wide-max-d8", "perft", "ref", ROOK, 8, (1, 1), {"DCHESS_PERFT_WIDE_MAX": "1000"}, 0),
        ("wide-level-max-d9", "perft", "ref", KINGS, 9, (1, 1), {"DCHESS_PERFT_WIDE_LEVEL_MAX": "100000"}, 0),
    ]
    for r in ("ref", "fide"):
        # (the REF fixture starts at depth 3: depths 1 and 2 are checked against perft's totals)
        for d in (1, 2, 4):
            out.append((f"stats-{r}-d{d}", "stats", r, "kiwipete", d, (1, 1), {}, 0))
    out += [
        ("stats-ref-d5", "stats", "ref", "startpos", 5, (1, 1), {}, 0),  # a level below the top under REF
        ("stats-fide-d4-split2-of3", "stats", "fide", "kiwipete", 4, (2, 3), {}, 0),
        ("stats-fide-d5-cap", "stats", "fide", "startpos", 5, (1, 1), {}, 10000),  # ply 4 past the cap: exact rerun
    ]
    return out


CASES = _cases()

# id: launches per NAMES entry (recorded from the parent commit's library; see the module docstring)
EXPECTED = {
    "ref-startpos-d1": (1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    "ref-startpos-d2": (1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0),
    "ref-startpos-d3": (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0),
    "ref-startpos-d4": (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0),
    "ref-startpos-d5": (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0),
    "ref-startpos-d6": (0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0),
    "ref-startpos-d7": (0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0),
    "ref-d5-split2-of3": (3, 3, 3, 0, 3, 3, 0, 0, 0, 0, 0),
    "ref-d5-split4-of5": (5, 0, 0, 0, 0, 5, 0, 0, 0, 0, 0),
    "ref-d6-split3-of2": (0, 0, 0, 0, 0, 2, 0, 0, 2, 0, 0),
    "ref-d7-split5-of3": (3, 3, 6, 6, 0, 3, 0, 0, 0, 0, 0),
    "fide-kiwipete-d3": (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0),
    "fide-kiwipete-d4": (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0),
    "fide-kiwipete-d5": (1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0),
    "fide-kiwipete-d5-split3-of3": (3, 3, 3, 3, 0, 3, 0, 0, 0, 0, 0),
    "batch-ref-d4": (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0),
    "batch-fide-d4": (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0),
    "wide-d8": (1, 1, 3, 2, 1, 1, 0, 0, 0, 0, 0),
    "sliced-d9": (1, 1, 4, 3, 228, 228, 0, 0, 0, 0, 0),
    "k4-d8": (1, 1, 2, 2, 0, 0, 0, 1, 0, 0, 0),
    "k4-d8-black": (1, 1, 2, 2, 0, 0, 0, 1, 0, 0, 0),
    "k4-d9": (1, 1, 2, 2, 0, 0, 0, 1, 0, 0, 0),
    "k4-d10": (1, 1, 2, 2, 0, 0, 0, 1, 0, 0, 0),
    "wide-max-d8": (2, 6, 8, 6, 1, 1, 0, 1, 0, 0, 0),
    "wide-level-max-d9": (2, 6, 9, 7, 1, 1, 0, 1, 0, 0, 0),
    "stats-ref-d1": (1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1),
    "stats-ref-d2": (1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1),
    "stats-ref-d4": (1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1),
    "stats-fide-d1": (1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1),
    "stats-fide-d2": (1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1),
    "stats-fide-d4": (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1),
    "stats-ref-d5": (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1),
    "stats-fide-d4-split2-of3": (3, 3, 3, 3, 0, 0, 0, 0, 0, 0, 3),
    "stats-fide-d5-cap": (2, 4, 4, 4, 0, 0, 0, 0, 0, 0, 2),
}


def _pos(p):
    return dchess.pos_from_fen(suite_fen(p) if " " not in p else p)


def collect(case):
    """Runs the case on a fresh context with profiling on.  Returns (launch
    counts in NAMES order, what the call computed)."""
    _, kind, rules, position, depth, (split, n_shards), env, cap = case
    rules = RULES[rules]
    saved = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    eng = dchess.Engine(0)
    try:
        L = dchess.lib()
        if cap:
            L.dc_test_perft_stats_level_cap.argtypes = [C.c_void_p, C.c_uint64]
            L.dc_test_perft_stats_last_exact.argtypes = [C.c_void_p]
            assert L.dc_test_perft_stats_level_cap(eng.ctx, cap) == dchess.SUCCESS
        eng.set_profiling(True)
        eng.reset_stats()
        if kind == "batch":
            got = eng.perft_batch([_pos(p) for p in position], depth, rules)[0].tolist()
        elif kind == "perft":
            p = _pos(position)
            got = sum(eng.perft_shard(p, depth, split, s, n_shards, rules)[0] for s in range(n_shards))
        else:
            p = _pos(position)
            got = np.zeros(dchess.PS_COUNT, np.uint64)
            for s in range(n_shards):
                got += eng.perft_stats(p, depth, rules, split_depth=split, shard=s, n_shards=n_shards)[0]
            got = got.tolist()
            if cap:
                assert L.dc_test_perft_stats_last_exact(eng.ctx) == 1
        counts = tuple(int(eng.kernel_stats(n)["launches"]) for n in NAMES)
    finally:
        eng.close()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return counts, got


_fast = {}


def golden(case):
    _, kind, rules, position, depth, _, _, _ = case
    r = RULES[rules]
    if kind == "batch":
        return [suite_total(p, depth, r) for p in position]
    if kind == "stats":
        key = "fide_suite" if r == FIDE else "ref_suite"
        ent = PS[key][position]["depths"].get(str(depth))
        return ent["totals"] if ent else None
    if " " not in position:
        return OG["perft_ref"]["startpos"][str(depth)]["total"] if (r, position) == (REF, "startpos") else \
            suite_total(position, depth, r)
    if (position, depth) not in _fast:  # a sparse position: fastcpu, once per position and depth
        _fast[position, depth] = O.fast_perft(O.Pos.from_fen(position), depth, O.REF,
                                              threads=min(16, os.cpu_count() or 1))[0]
    return _fast[position, depth]


def test_table_covers_the_cases():
    assert sorted(EXPECTED) == sorted(c[0] for c in CASES)
    assert all(len(v) == len(NAMES) for v in EXPECTED.values())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_launch_sequence(case):
    counts, got = collect(case)
    print(case[0], dict(zip(NAMES, counts)), got)
    want = golden(case)
    if want is None:  # perft statistics below the fixture's depths: NODES is perft's total
        assert got[dchess.PS_NODES] == suite_total(case[3], case[4], RULES[case[2]])
    else:
        assert got == want
    assert dict(zip(NAMES, counts)) == dict(zip(NAMES, EXPECTED[case[0]]))


if __name__ == "__main__":
    for c in CASES:  # (with the package's directory in PYTHONPATH)
        print(f'    "{c[0]}": {collect(c)[0]},', flush=True)
