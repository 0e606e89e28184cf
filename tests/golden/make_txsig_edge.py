#!/usr/bin/env python3
"""Generates tests/golden/txsig_edge.json: signatures crafted so that the
verifier's u1 G + u2 Q runs where honestly signed transactions never take it.

A verifier sees only (u1, u2) = (z/s, r/s) and Q, so for any chosen (u1, u2)
and a real message hash z there is a valid signature: r = z u2 / u1 (retry the
message until r is an x coordinate), R = (r, y), s = r / u2,
Q = (R - u1 G) / u2 (tests/secp_model.py craft).  Oracle only (oracle/txsig.py
and the big-integer models of tests/secp_model.py), seeded; every property a
class claims is asserted here, so a class that cannot be built fails the run.

Classes:
  sweep        u1 with byte j in all 32 rows, j = 1..255: every G-table entry
  sweep_twin   every eighth of them with the lowest bit of r flipped (verdict 5)
  sparse_u1    u1 = 2^(8k), k = 0..31, and n - 1
  u2_fixed     u2 = 1, 2, n-1, n-2, lambda, ..., (n +- 1)/2
  u2_split     u2 = k1 + lambda k2: four sign pairs x magnitudes up to 2^128
  xr_ge_n      R = (n + t, y): valid only by ecdsa_verify's second comparison
  xr_ge_n_twin the same with s + 1 (verdict 5 after both comparisons)
  r_boundary   r = p - n (r + n = p: no second comparison) and p - n - 1
  r_inf        Q = d G, r = -z/d: u1 G + u2 Q is the point at infinity
  arm_double   Q = G, u2 = 1, low byte of u1 = 1: the first table addition doubles
  arm_inf      the accumulator passes through infinity after table row i
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import secp_model as M  # noqa: E402
from secp_model import N, P, T  # noqa: E402

OUT = os.path.join(HERE, "txsig_edge.json")


def main(seed=0xED6E51):
    rng = random.Random(seed)
    txs = []

    def names(i):
        return "white-%d" % (i % 7), "black-%d" % (i % 5)

    def emit(cls, white, black, act, r, s, pk, want, u1=None, u2=None):
        sig = T.sig_hex(r, s)
        v = T.check_tx(white, black, tuple(act), sig, pk)
        assert v == want, (cls, v, want)
        z = int.from_bytes(T.message_hash(white, black, tuple(act)), "big") % N
        si = M.inv_n(s)
        if u1 is not None:
            assert (z * si % N, r * si % N) == (u1, u2), cls
        txs.append({"class": cls, "white": white, "black": black, "action": list(act), "sig": sig, "pk": pk,
                    "turn": -1, "verdict": v, "u1": "%064x" % (z * si % N), "u2": "%064x" % (r * si % N)})

    def valid(cls, u1, u2, form="c"):
        i = len(txs)
        w, b = names(i)
        act, r, s, q = M.craft(u1, u2, w, b, [rng.randrange(8) for _ in range(4)], odd=bool(i & 1))
        emit(cls, w, b, act, r, s, M.pk_hex(q, form), 0, u1, u2)
        return w, b, act, r, s, q

    # ---- table sweep: byte j in every row (the top byte lowered where that is >= n)
    ones = sum(1 << (8 * i) for i in range(32))
    sweep = []
    for j in range(1, 256):
        u1 = j * ones
        if u1 >= N:
            u1 -= 1 << 248
        sweep.append(u1)
    sweep.append(0xFF << 248 | ones >> 8)  # top byte 0xFF
    assert all(0 < u < N for u in sweep) and sweep[-1] >> 248 == 0xFF
    seen = set()
    for k, u1 in enumerate(sweep):
        w, b, act, r, s, q = valid("sweep", u1, rng.randrange(1, N), "u" if k % 16 == 5 else "c")
        seen |= M.u1_rows(u1)
        if k % 8 == 0:
            emit("sweep_twin", w, b, act, r ^ 1, s, txs[-1]["pk"], 5)
    assert seen == {(i, j) for i in range(32) for j in range(1, 256)}, len(seen)

    # ---- sparse u1
    for u1 in [1 << (8 * k) for k in range(32)] + [N - 1]:
        valid("sparse_u1", u1, rng.randrange(1, N))

    # ---- u2 shapes
    for u2 in M.u2_fixed():
        valid("u2_fixed", rng.randrange(1, N), u2)
    split_list = M.u2_split(rng)
    for u2 in split_list:
        valid("u2_split", rng.randrange(1, N), u2)
    shapes = [M.split_shape(u2) for u2 in split_list]
    assert {(a[0], b[0]) for a, b in shapes} == {(x, y) for x in (False, True) for y in (False, True)}
    for h in (0, 1):
        assert {d for sh in shapes for d in sh[h][1]} == set(range(-4, 5)), h
        assert any(sh[h][1][M.Q_WINDOWS - 1] for sh in shapes), h
    for u2 in M.u2_fixed() + split_list:
        assert all(abs(M.signed(k)) < 2 ** 128 for k in M.split(u2))

    # ---- x(R) >= n: r = t, R = (n + t, y)
    ts = [t for t in range(1, 40) if M.lift_x(N + t, False)][:3]
    assert len(ts) == 3 and all(t + N < P for t in ts)
    for k, t in enumerate(ts):
        i = len(txs)
        w, b = names(i)
        act = [rng.randrange(8) for _ in range(4)]
        z = int.from_bytes(T.message_hash(w, b, tuple(act)), "big") % N
        s = rng.randrange(1, N - 1)
        R = M.lift_x(N + t, bool(k & 1))
        q = M.key_for(R, t, s, z)
        pk = M.pk_hex(q, "c")
        emit("xr_ge_n", w, b, act, t, s, pk, 0)
        u1, u2 = int(txs[-1]["u1"], 16), int(txs[-1]["u2"], 16)
        assert T._add(T.mul(u1, T.G), T.mul(u2, q)) == R and R[0] >= N  # accepted by the second comparison alone
        emit("xr_ge_n_twin", w, b, act, t, s + 1, pk, 5)
    # ---- r at the edge of the second comparison (r + n < p <=> r < p - n)
    for r in (P - N, P - N - 1):
        i = len(txs)
        w, b = names(i)
        emit("r_boundary", w, b, [rng.randrange(8) for _ in range(4)], r, rng.randrange(1, N),
             T.pubkey_hex(rng.randrange(1, N)), 5)

    # ---- R at infinity: Q = d G, r = -z/d, any s; the last with u1 < 2^192
    for form, short in (("c", False), ("u", False), ("h", False), ("c", True)):
        i = len(txs)
        w, b = names(i)
        act = [rng.randrange(8) for _ in range(4)]
        z = int.from_bytes(T.message_hash(w, b, tuple(act)), "big") % N
        d = rng.randrange(1, N)
        r = -z * M.inv_n(d) % N
        u1 = rng.randrange(2 ** 184, 2 ** 192)
        s = z * M.inv_n(u1) % N if short else rng.randrange(1, N)
        q = T.mul(d, T.G)
        emit("r_inf", w, b, act, r, s, M.pk_hex(q, form), 5, u1 if short else None, -u1 * M.inv_n(d) % N)
        u1, u2 = int(txs[-1]["u1"], 16), int(txs[-1]["u2"], 16)
        assert T._add(T.mul(u1, T.G), T.mul(u2, q)) is None
        assert not short or u1 >> 192 == 0

    # ---- through gej_add_ge's special arms with an invalid result
    def through(cls, d, u1, u2):
        i = len(txs)
        w, b = names(i)
        act = [rng.randrange(8) for _ in range(4)]
        z = int.from_bytes(T.message_hash(w, b, tuple(act)), "big") % N
        s = z * M.inv_n(u1) % N
        emit(cls, w, b, act, u2 * s % N, s, M.pk_hex(T.mul(d, T.G), "c"), 5, u1, u2)

    u1 = rng.randrange(1, N) >> 8 << 8 | 1
    through("arm_double", 1, u1, 1)  # u2 Q = G, then row 0 adds gtab[1] = G
    for row in (0, 13, 30):
        u1 = rng.randrange(N >> 1, N)
        low = u1 % (1 << (8 * (row + 1)))
        assert low and (u1 >> (8 * (row + 1))) & 255
        d = rng.randrange(1, N)
        u2 = -low * M.inv_n(d) % N  # u2 Q = -(the rows 0..row of u1) G
        assert T._add(T.mul(u2, T.mul(d, T.G)), T.mul(low, T.G)) is None
        through("arm_inf", d, u1, u2)

    out = {"generator": "tests/golden/make_txsig_edge.py", "seed": seed, "txs": txs}
    json.dump(out, open(OUT, "w"), separators=(",", ":"))
    assert os.path.getsize(OUT) <= os.path.getsize(os.path.join(HERE, "txsig_batch.json"))
    classes = {}
    for t in txs:
        classes.setdefault(t["class"], [0, 0])[t["verdict"] != 0] += 1
    print(len(txs), os.path.getsize(OUT), classes)


if __name__ == "__main__":
    main()
