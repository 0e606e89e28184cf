"""CPU tests of the legal-move list entry points (dc_legal_moves_batch*): the
library exports them, a NULL context is an argument error before any device is
touched, the Python constants are the header's, and every kernel of the list
path is built without scratch memory."""
import ctypes as C
import os
import re

import pytest

import dchess
from test_spill_free import LLVM, kernel_scratch

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dchess.h")


def test_library_exports_legal_moves():
    L = dchess.lib()
    names = dchess.exported_symbols()
    for n in ("dc_legal_moves_batch", "dc_legal_moves_batch_device"):
        assert n in names, n
        assert hasattr(L, n), n


def test_null_context_is_einval():
    off = (C.c_uint32 * 2)()
    tot = C.c_uint32()
    for fn in (dchess.lib().dc_legal_moves_batch, dchess.lib().dc_legal_moves_batch_device):
        assert fn(None, dchess.RULES_REF, None, 0, C.cast(off, C.c_void_p), None, None, 0, C.byref(tot)) == dchess.EINVAL


def test_status_constants_match_header():
    hdr = open(HEADER).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+DC_ST_(\w+)\s+(\d+)u", hdr)}
    assert vals == {"CHECK": dchess.ST_CHECK, "NO_MOVES": dchess.ST_NO_MOVES, "DEAD": dchess.ST_DEAD}
    assert (dchess.ST_CHECK, dchess.ST_NO_MOVES, dchess.ST_DEAD) == (1, 2, 4)


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm llvm tools")
def test_legal_kernels_use_no_scratch():
    ks = {n: s for n, s in kernel_scratch().items() if "k_legal_" in n}
    assert len(ks) >= 4, sorted(ks)
    assert not {n: s for n, s in ks.items() if s != 0}, ks
