"""CPU tests of the perft statistics entry points (dc_perft_stats*): the library
exports them, a NULL context is an argument error before any device is touched,
the Python constants are the header's, the leaf kernel is built without scratch
memory, and the committed fixture holds the published tables' values."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import dchess
from test_spill_free import LLVM, kernel_scratch

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "dchess.h")
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_perft_stats as G  # noqa: E402  (the pinned tables; nothing runs on import)

FX = json.load(open(os.path.join(HERE, "golden", "perft_stats.json")))


def test_library_exports_perft_stats():
    L = dchess.lib()
    names = dchess.exported_symbols()
    for n in ("dc_perft_stats", "dc_perft_stats_shard"):
        assert n in names, n
        assert hasattr(L, n), n


def test_null_context_is_einval():
    tot = (C.c_uint64 * dchess.PS_COUNT)()
    nr = C.c_uint32()
    pos = np.array([dchess.startpos()], dchess.POS_DTYPE)
    p = C.c_void_p(pos.ctypes.data)
    L = dchess.lib()
    assert L.dc_perft_stats(None, dchess.RULES_FIDE, p, 1, C.cast(tot, C.c_void_p), None, None,
                            C.byref(nr)) == dchess.EINVAL
    assert L.dc_perft_stats_shard(None, dchess.RULES_FIDE, p, 1, 1, 0, 1, C.cast(tot, C.c_void_p), None, None,
                                  C.byref(nr)) == dchess.EINVAL


def test_counter_constants_match_header():
    hdr = open(HEADER).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+DC_PS_(\w+)\s+(\d+)\b", hdr)}
    assert vals.pop("COUNT") == dchess.PS_COUNT == 11
    assert vals == {n: getattr(dchess, "PS_" + n) for n in
                    ("NODES", "CAPTURES", "EP", "CASTLES", "PROMOTIONS", "CHECKS", "DISCOVERED", "DOUBLE",
                     "CHECKMATES", "STALEMATES", "KING_CAPTURES")}
    assert sorted(vals.values()) == list(range(11))
    assert len(dchess.PS_NAMES) == dchess.PS_COUNT and tuple(FX["names"]) == dchess.PS_NAMES


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm llvm tools")
def test_leaf_stats_kernel_uses_no_scratch():
    ks = {n: s for n, s in kernel_scratch().items() if "k_leaf_stats" in n}
    assert len(ks) == 4, sorted(ks)  # REF and FIDE, either side to move
    assert not {n: s for n, s in ks.items() if s != 0}, ks


def test_fixture_holds_the_published_tables():
    for (name, d), want in G.PINS.items():
        tot = FX["fide_suite"][name]["depths"][str(d)]["totals"]
        assert tuple(tot[:9]) == want, (name, d, tot)
        assert tot[dchess.PS_KING_CAPTURES] == 0
    for (name, d), (nodes, cap, kcap) in G.REF_PINS.items():
        tot = FX["ref_suite"][name]["depths"][str(d)]["totals"]
        assert (tot[dchess.PS_NODES], tot[dchess.PS_CAPTURES], tot[dchess.PS_KING_CAPTURES]) == (nodes, cap, kcap)
        assert not any(tot[dchess.PS_EP:dchess.PS_KING_CAPTURES])
    small = {e["fen"]: e["depths"] for e in FX["fide_small"]}
    assert list(small) == G.SMALL
    for fen, per in G.SMALL_PINS.items():
        for d, pins in per.items():
            tot = small[fen][str(d)]["totals"]
            for k, v in pins.items():
                assert tot[dchess.PS_NAMES.index(k)] == v, (fen, d, k, tot)
    # every entry with rows: the totals are the rows' column sums
    for grp in (list(FX["fide_suite"].values()) + FX["fide_small"] + list(FX["ref_suite"].values()) + FX["ref_random"]):
        for e in grp["depths"].values():
            if "rows" in e:
                assert [sum(r[k] for r in e["rows"]) for k in range(11)] == e["totals"]
                assert len(e["moves"]) == len(e["rows"])
