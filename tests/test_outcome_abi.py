"""CPU tests of the game-adjudication entry points (dc_replay_outcome*,
dc_fen_clocks): the library exports them, a NULL context is an argument error
before any device is touched, the Python constants and the record layout are
the header's, the FEN clocks parse on the host, and the adjudication kernel is
built without scratch memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dchess
from test_spill_free import LLVM, kernel_scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dchess.h")


def test_library_exports_outcome_symbols():
    L = dchess.lib()
    names = dchess.exported_symbols()
    for n in ("dc_replay_outcome", "dc_replay_outcome_device", "dc_fen_clocks"):
        assert n in names, n
        assert hasattr(L, n), n


def test_null_context_is_einval():
    out = np.zeros(1, dchess.OUTCOME_DTYPE)
    mv = np.zeros(1, np.uint16)
    for fn in (dchess.lib().dc_replay_outcome, dchess.lib().dc_replay_outcome_device):
        assert fn(None, None, 0, dchess._ptr(mv), 1, 1, dchess._ptr(out), None, None, None, None) == dchess.EINVAL


def test_result_constants_match_header():
    hdr = open(HEADER).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+DC_GO_(\w+)\s+(\d+)\b", hdr)}
    assert vals == {"ONGOING": dchess.GO_ONGOING, "WHITE_WINS": dchess.GO_WHITE_WINS,
                    "BLACK_WINS": dchess.GO_BLACK_WINS, "STALEMATE": dchess.GO_STALEMATE, "DEAD": dchess.GO_DEAD,
                    "FIVEFOLD": dchess.GO_FIVEFOLD, "SEVENTYFIVE": dchess.GO_SEVENTYFIVE, "COUNT": dchess.GO_COUNT}
    assert [vals[k] for k in ("ONGOING", "WHITE_WINS", "BLACK_WINS", "STALEMATE", "DEAD", "FIVEFOLD", "SEVENTYFIVE",
                              "COUNT")] == list(range(8))
    assert len(dchess.GO_NAMES) == dchess.GO_COUNT


def test_outcome_record_is_8_bytes():
    """sizeof(dc_game_outcome) == 8 with the fields where OUTCOME_DTYPE reads
    them, asked of a compiler on the header itself."""
    d = dchess.OUTCOME_DTYPE
    assert d.itemsize == 8
    assert [d.fields[k][1] for k in ("result", "repeats", "halfmove", "end_ply")] == [0, 1, 2, 4]
    src = ('#include <stddef.h>\n#include "dchess.h"\n'
           "static_assert(sizeof(dc_game_outcome) == 8, \"size\");\n"
           "static_assert(offsetof(dc_game_outcome, result) == 0 && offsetof(dc_game_outcome, repeats) == 1 &&\n"
           "              offsetof(dc_game_outcome, halfmove) == 2 && offsetof(dc_game_outcome, end_ply) == 4, \"layout\");\n")
    # g++: the compiler the build itself uses for the host programs
    r = subprocess.run(["g++", "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", os.path.dirname(HEADER), "-"],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


def test_fen_clocks():
    assert dchess.fen_clocks("rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1") == (0, 1)
    assert dchess.fen_clocks("r3k2r/8/8/8/8/8/8/R3K2R b KQkq e3 37 112") == (37, 112)
    assert dchess.fen_clocks("8/8/8/8/k3p2Q/8/3P4/3K4 w - - 149 300") == (149, 300)
    # absent fields: 0 and 1
    assert dchess.fen_clocks("4k3/3p4/8/4P3/8/8/8/4K3 b") == (0, 1)
    assert dchess.fen_clocks("4k3/3p4/8/4P3/8/8/8/4K3 b - -") == (0, 1)
    assert dchess.fen_clocks("4k3/3p4/8/4P3/8/8/8/4K3 b - - 12") == (12, 1)
    hm = C.c_uint32()
    assert dchess.lib().dc_fen_clocks(b"4k3/8/8/8/8/8/8/4K3 w - - 7 9", C.byref(hm), None) == dchess.SUCCESS
    assert hm.value == 7
    assert dchess.lib().dc_fen_clocks(None, C.byref(hm), None) == dchess.EINVAL
    for bad in ("4k3/8/8/8/8/8/8/4K3 w - - x 1", "4k3/8/8/8/8/8/8/4K3 w - - 3 1x", "4k3/8/8/8/8/8/8/4K3 w - - -1 1",
                "4k3/8/8/8/8/8/8/4K3 w - - 99999999999 1"):
        with pytest.raises(dchess.DChessError):
            dchess.fen_clocks(bad)


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm llvm tools")
def test_outcome_kernels_use_no_scratch():
    ks = {n: s for n, s in kernel_scratch().items() if "k_replay_outcome" in n or "k_outcome_reduce" in n}
    assert len(ks) == 2, sorted(ks)
    assert not {n: s for n, s in ks.items() if s != 0}, ks
