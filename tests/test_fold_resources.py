"""k_front_fold and k_copy_result fit on a CU beside the other context's heavy
kernels (CPU test, reads the built library's gfx950 code-object notes as
tests/test_spill_free.py does).  The fold ships with its
tag histogram in LDS (the form without LDS measured slower), so it is held to
what k_front leaves; the result copy has no LDS and is held to k_count3c too.

bench.py's headline runs two contexts so that one run's latency-bound kernels
execute while the other holds the VALUs.  A fold wave does that only if it
fits into what k_front<0,1,true> (one 1,024-thread block a CU: four waves per
SIMD at 120 registers, 155,888 B of LDS) or k_count3c<0,4592,4,u32,true> (four
256-thread blocks a CU: four waves per SIMD at 112 registers, 4 x 40,952 B of
LDS) leave free: 32 registers per SIMD, and no LDS beside k_count3c."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import dchess

LLVM = "/opt/rocm/lib/llvm/bin"
FRONT_LDS_LEFT = 7952  # what one k_front<0,1,true> block leaves of a CU's LDS after allocation rounding
SIMD_REGS = 512      # unified VGPR + AGPR file per lane of a SIMD
CU_LDS = 163840      # bytes
REG_GRANULE = 8
FIELDS = ("vgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size")

# mangled-name fragments
FOLD = "12k_front_foldENS_"  # (no template parameter since its form without LDS was removed)
COPY = "13k_copy_result"
FRONT = "7k_frontILi0ELi1ELb1E"
COUNT = "9k_count3cILi0ELj4592ELi4EjLb1E"


def kernel_notes():
    """{kernel name: {field: value}} over every gfx950 code object of the library."""
    tmp = tempfile.mkdtemp()
    try:
        lib = os.path.join(tmp, "lib.so")
        shutil.copy(dchess.LIB_PATH, lib)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", lib], cwd=tmp, check=True,
                       capture_output=True)
        out = {}
        for f in os.listdir(tmp):
            if not f.endswith("gfx950"):
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, f)],
                                   check=True, capture_output=True, text=True).stdout
            cur, indent = None, None
            for line in notes.splitlines():
                m = re.match(r"(\s*)(- )?\.(\w+):\s*(\S*)", line)
                if not m:
                    continue
                col = len(m.group(1)) + (2 if m.group(2) else 0)
                if m.group(2) and (indent is None or col <= indent) and m.group(3) in ("agpr_count", "args"):
                    cur, indent = {}, col  # a new kernel's map (its keys are sorted: .agpr_count or .args first)
                if cur is None or col != indent:
                    continue
                if m.group(3) == "name":
                    out[m.group(4)] = cur
                elif m.group(3) in FIELDS:
                    cur[m.group(3)] = int(m.group(4))
        return out
    finally:
        shutil.rmtree(tmp)


def _one(ks, frag):
    hit = [v for n, v in ks.items() if frag in n]
    assert len(hit) == 1, (frag, [n for n in ks if frag in n])
    assert all(f in hit[0] for f in FIELDS), hit[0]
    return hit[0]


def _regs(k):
    r = k["vgpr_count"] + k["agpr_count"]
    return (r + REG_GRANULE - 1) // REG_GRANULE * REG_GRANULE


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="no ROCm llvm tools")
def test_fold_and_copy_fit_beside_the_heavy_kernels():
    ks = kernel_notes()
    assert len(ks) >= 40, sorted(ks)
    front, count = _one(ks, FRONT), _one(ks, COUNT)
    for frag, lds_bound in ((FOLD, FRONT_LDS_LEFT), (COPY, 0)):
        k = _one(ks, frag)
        assert k["vgpr_count"] <= 32 and k["agpr_count"] == 0, (frag, k)
        assert k["private_segment_fixed_size"] == 0, (frag, k)
        assert k["group_segment_fixed_size"] <= lds_bound, (frag, k)
        # beside k_front: four of its waves and one of ours on a SIMD, both blocks' LDS on the CU
        assert 4 * _regs(front) + _regs(k) <= SIMD_REGS, (frag, k, front)
        assert front["group_segment_fixed_size"] + k["group_segment_fixed_size"] <= CU_LDS
        if lds_bound == 0:
            # beside k_count3c: four blocks of it a CU, one wave of each per SIMD
            assert 4 * _regs(count) + _regs(k) <= SIMD_REGS, (frag, k, count)
            assert 4 * count["group_segment_fixed_size"] + k["group_segment_fixed_size"] <= CU_LDS
