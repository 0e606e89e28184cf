#!/usr/bin/env python3
"""Measures dc_legal_moves_batch_device (the legal-move list section).

Input: the 615 FIDE test positions (tests/test_gpu_legal_moves.py fide_set)
tiled to --n positions, uploaded once.  After warm-up it times

  - the _device call end to end (a host clock around the call, which returns
    after a stream synchronise);
  - the "legal_count" and "legal_emit" kernels (dc_ctx_kernel_stats) in a
    separate profiling-on pass;
  - host-form calls of n = 1 and n = 64 positions, in microseconds per call;
  - what a caller needs for the same answer without the list call:
    dc_validate_batch over all 4,096 (from, to) pairs of 4,096 positions.

Prints one JSON line (the figures under variants.shipped: an earlier staged
emit was timed beside the shipped one).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "distributed-chess_amd"), os.path.join(REPO, "tests")]

import dchess  # noqa: E402

FIDE = dchess.RULES_FIDE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs-positions", type=int, default=4096)
    ap.add_argument("--small-calls", type=int, default=2000)
    a = ap.parse_args()

    import test_gpu_legal_moves as T
    base = T.fide_set().pos
    eng = dchess.Engine(0)
    variants = ["shipped"]

    n = a.n
    pos = base[np.arange(n) % len(base)]
    d_pos = eng.alloc(pos.nbytes)
    d_pos.upload(pos)
    d_off, d_st = eng.alloc(4 * (n + 1)), eng.alloc(n)
    total = eng.legal_moves_device(d_pos, n, d_off, d_st, None, 0, FIDE)
    d_mv = eng.alloc(2 * max(total, 1))
    out = {"n": n, "moves": total, "lib": os.path.basename(dchess.LIB_PATH), "variants": {}}

    # ---- end to end
    wall = {v: [] for v in variants}
    for r in range(a.warmup + a.reps):
        for v in variants:
            t0 = time.perf_counter()
            eng.legal_moves_device(d_pos, n, d_off, d_st, d_mv, total, FIDE)
            dt = time.perf_counter() - t0
            if r >= a.warmup:
                wall[v].append(dt)
    # ---- kernel times, profiling on
    eng.set_profiling(True)
    for v in variants:
        eng.reset_stats()
        for _ in range(a.reps):
            eng.legal_moves_device(d_pos, n, d_off, d_st, d_mv, total, FIDE)
        cnt, emit = eng.kernel_stats("legal_count"), eng.kernel_stats("legal_emit")
        scan = eng.kernel_stats("legal_scan")
        w = float(np.median(wall[v]))
        cms, ems = cnt["total_ms"] / cnt["launches"], emit["total_ms"] / emit["launches"]
        out["variants"][v] = {
            "call_ms_median": w * 1e3, "call_ms_min": min(wall[v]) * 1e3, "call_ms_max": max(wall[v]) * 1e3,
            "positions_per_s": n / w, "moves_per_s": total / w,
            "legal_count_ms": cms, "legal_scan_ms": scan["total_ms"] / scan["launches"], "legal_emit_ms": ems,
            "emit_over_count": ems / cms,
            "emit_write_GBps": (2 * total + 4 * n) / (ems * 1e-3) / 1e9,
        }
    eng.set_profiling(False)
    eng.reset_stats()

    # ---- small host-form calls (one launch, pinned I/O)
    L = dchess.lib()
    small = {}
    for k in (1, 64):
        p = np.ascontiguousarray(base[:k])
        off, st, mv = np.zeros(k + 1, np.uint32), np.zeros(k, np.uint8), np.zeros(256 * k, np.uint16)
        tot = C.c_uint32()
        args = (eng.ctx, FIDE, dchess._ptr(p), k, dchess._ptr(off), dchess._ptr(st), dchess._ptr(mv), len(mv),
                C.byref(tot))
        for v in variants:
            for _ in range(200):
                assert L.dc_legal_moves_batch(*args) == 0
            t0 = time.perf_counter()
            for _ in range(a.small_calls):
                L.dc_legal_moves_batch(*args)
            small[f"n{k}_{v}_us"] = (time.perf_counter() - t0) / a.small_calls * 1e6
    out["host_form_us_per_call"] = small

    # ---- the same answer without the list call: every (from, to) pair validated
    m = a.pairs_positions
    pp = np.repeat(base[np.arange(m) % len(base)], 4096)
    words = np.tile(np.arange(4096, dtype=np.uint16), m)
    eng.validate_batch(pp[:4096 * 64], words[:4096 * 64], FIDE)  # warm-up
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        ver = eng.validate_batch(pp, words, FIDE)
        ts.append(time.perf_counter() - t0)
    eng.set_profiling(True)
    eng.reset_stats()
    eng.validate_batch(pp, words, FIDE)
    vk = eng.kernel_stats("validate")
    eng.set_profiling(False)
    ok = int((ver == dchess.V_OK).sum())
    best = min(out["variants"].values(), key=lambda d: d["call_ms_median"])
    out["all_pairs"] = {
        "positions": m, "verdicts": len(words), "accepted": ok,
        "host_call_ms": min(ts) * 1e3, "validate_kernel_ms": vk["total_ms"] / max(vk["launches"], 1),
        "us_per_position_host_call": min(ts) / m * 1e6,
        "us_per_position_kernel": vk["total_ms"] / max(vk["launches"], 1) / m * 1e3,
        "list_us_per_position_call": best["call_ms_median"] / n * 1e3,
        "list_us_per_position_kernels": (best["legal_count_ms"] + best["legal_scan_ms"] + best["legal_emit_ms"]) / n * 1e3,
    }
    out["all_pairs"]["ratio_kernels"] = (out["all_pairs"]["us_per_position_kernel"]
                                         / out["all_pairs"]["list_us_per_position_kernels"])
    out["all_pairs"]["ratio_calls"] = (out["all_pairs"]["us_per_position_host_call"]
                                       / out["all_pairs"]["list_us_per_position_call"])
    for d in (d_pos, d_off, d_st, d_mv):
        d.free()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
