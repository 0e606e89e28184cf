"""The secp256k1 arithmetic below dc_verify_tx_batch, one operation per lane
(csrc/dc_test_secp.hip, dc_test_secp_op), against Python big integers and
oracle/txsig.py.  Exact comparisons only.

On the device mul_wide, sqr_wide, fe_reduce and sc_fold are Comba loops over two
inline-asm helpers; the host build (build/test_secp) compiles their C branch.
Every operand list below therefore runs twice: on the CPU through build/test_secp
(test_host_list) and, under the gpu mark, through the device hook (test_gpu_list).
The lists are built to reach what random operands do not:

  - fe_reduce's second carry w and fe_canon's subtraction: products = v mod p
    with one factor near p and 2^33 <= v < 2^60 (w = 1) or v < 2^32 + 977 (canon);
  - sc_reduce's fourth fold (h3 = 1) and sc_canon's subtraction: products
    = v mod n with C <= v < 2^134 resp. v < C, C = 2^256 - n;
  - every slot of the device-built G table;
  - ecdsa_verify through gej_add_ge's doubling, infinity and a.inf arms with a
    *valid* result (known discrete logs and a chosen z), R at infinity,
    x(R) >= n, z = 0;
  - ecmult at the GLV / Booth edges test_host_point_mul checks on the host.

test_stage_coverage asserts, from the operand lists alone, how often each
stage condition is reached, and prints the counts (pytest -s).
"""
import ctypes as C
import functools
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import secp_model as M  # noqa: E402
from secp_model import N, P, T  # noqa: E402
from test_txsig import secp_bin  # noqa: E402,F401  (the build/test_secp line driver)

OPS = {"fe_mul": 0, "fe_sqr": 1, "fe_add": 2, "fe_sub": 3, "fe_inv": 4, "fe_sqrt": 5, "sc_mul": 6, "sc_inv": 7,
       "sc_add": 8, "split": 9, "ecmult": 10, "verify": 11, "gtab": 12}
FE_EDGE = [P - 1, P - 2, 0, 1, 2, 2 ** 255, 2 ** 32 + 977]
SC_EDGE = [N - 1, N - 2, 0, 1, 2, 2 ** 255, M.C_N, M.C_N - 1, 2 ** 128]
LIMB = [0xFFFFFFFF << (32 * i) for i in range(8)]


# ---------------------------------------------------------------- operand lists
# Each returns (op, operands, expected): operands are tuples of integers (at most
# five), expected (result0, result1, flag) as dc_test_secp_op writes them.
def _near(rng, m):
    return m - 1 - rng.randrange(2 ** 64)


def _fe_stage_pairs(rng, count):
    """(a, b) with a near p and a b = v mod p: half with 2^33 <= v < 2^60 (the
    second carry w), half with v < 2^32 + 977 (the canon subtraction)."""
    out = []
    for k in range(count):
        a = _near(rng, P)
        v = rng.randrange(2 ** 33, 2 ** 60) if k & 1 else rng.randrange(M.K_P)
        out.append((a, v * M.inv_p(a) % P))
    return out


@functools.lru_cache(None)
def fe_mul_list():
    rng = random.Random(101)
    ops = _fe_stage_pairs(rng, 2000)
    ops += [(a, b) for a in LIMB for b in LIMB]
    ops += [(a, b) for a in FE_EDGE for b in FE_EDGE]
    ops += [(rng.randrange(P), rng.randrange(P)) for _ in range(500)]
    return "fe_mul", ops, [(a * b % P, 0, 0) for a, b in ops]


@functools.lru_cache(None)
def fe_sqr_list():
    rng = random.Random(102)
    ops = []
    v = 0
    while len(ops) < 400:  # roots of small residues: a^2 = v mod p, v < 2^32 + 977 (canon)
        v += 1
        y = pow(v, (P + 1) // 4, P)
        if y * y % P == v:
            ops += [(y,), (P - y,)]
    while len(ops) < 800:  # and of 2^33 <= v < 2^60 (w)
        v = rng.randrange(2 ** 33, 2 ** 60)
        y = pow(v, (P + 1) // 4, P)
        if y * y % P == v:
            ops += [(y,), (P - y,)]
    ops += [(a,) for a in LIMB + FE_EDGE]
    ops += [(rng.randrange(P),) for _ in range(500)]
    return "fe_sqr", ops, [(a * a % P, 0, 0) for a, in ops]


def _add_edges(m, rng):
    """(a, b) below m with a + b = m - 1, m, m + 1, around 2^256 and 2m - 2."""
    out = []
    for a in (1, 2, m // 2, m - 2, rng.randrange(1, m - 2), rng.randrange(1, m - 2)):
        for total in (m - 1, m, m + 1):
            b = total - a
            if 0 <= b < m:
                out.append((a, b))
    k = M.M256 - m
    for total in (M.M256 - 1, M.M256, M.M256 + 1, M.M256 + k, M.M256 + k - 1, M.M256 + k + 1, 2 * m - 2, 2 * m - 3):
        for a in (m - 1, m - 2, m - rng.randrange(1, k)):
            b = total - a
            if 0 <= b < m:
                out.append((a, b))
    return out + [(0, 0), (0, m - 1), (m - 1, 0), (m - 1, m - 1), (m - 1, 1)]


@functools.lru_cache(None)
def fe_add_list():
    rng = random.Random(103)
    ops = _add_edges(P, rng) + [(a, b) for a in FE_EDGE for b in FE_EDGE]
    ops += [(rng.randrange(P), rng.randrange(P)) for _ in range(200)]
    assert any(a + b >= M.M256 for a, b in ops) and {a + b - P for a, b in ops} >= {-1, 0, 1}
    return "fe_add", ops, [((a + b) % P, 0, 0) for a, b in ops]


@functools.lru_cache(None)
def fe_sub_list():
    rng = random.Random(104)
    xs = FE_EDGE + [rng.randrange(P) for _ in range(12)]
    ops = [(a, b) for a in xs for b in xs] + [(0, x) for x in xs] + [(x, x) for x in xs]
    ops += [(a, a + 1) for a in xs if a + 1 < P] + [(a + 1, a) for a in xs if a + 1 < P]
    # borrows that run the whole chain, and differences just under 2^32 + 977
    ops += [(0, 1), (1 << 224, 1), (0, M.K_P), (M.K_P - 1, M.K_P), (5, M.K_P + 5), (1 << 32, (1 << 32) + 977)]
    assert any(a < b for a, b in ops) and any(a > b for a, b in ops)
    return "fe_sub", ops, [((a - b) % P, 0, 0) for a, b in ops]


@functools.lru_cache(None)
def fe_inv_list():
    rng = random.Random(105)
    ops = [(a,) for a in FE_EDGE + LIMB + [rng.randrange(P) for _ in range(200)]]
    return "fe_inv", ops, [(pow(a, P - 2, P), 0, 0) for a, in ops]


@functools.lru_cache(None)
def fe_sqrt_list():
    rng = random.Random(106)
    xs = list(FE_EDGE) + [3, 5, 7]
    for _ in range(150):
        a = rng.randrange(1, P)
        xs += [a * a % P, (P - a * a) % P]  # a residue and (p = 3 mod 4) a non-residue
    exp = []
    for a in xs:
        r = pow(a, (P + 1) // 4, P)
        exp.append((r, 0, int(r * r % P == a)))
    assert sum(e[2] for e in exp) >= 150 and sum(not e[2] for e in exp) >= 150 and 0 in xs
    return "fe_sqrt", [(a,) for a in xs], exp


def _sc_stage_pairs(rng):
    """(a, b), a near n: 1000 with a b = v mod n, v < C (the canon subtraction),
    and, filtered by the model from v in [C, 2^134), 100 whose fourth fold is
    not the identity (h3 = 1)."""
    out = []
    for _ in range(1000):
        a = _near(rng, N)
        out.append((a, rng.randrange(M.C_N) * M.inv_n(a) % N))
    got = 0
    for _ in range(200000):
        a = _near(rng, N)
        b = rng.randrange(M.C_N, 2 ** 134) * M.inv_n(a) % N
        if M.sc_reduce_stages(a * b)[3]:
            out.append((a, b))
            got += 1
            if got == 100:
                break
    assert got == 100
    return out


@functools.lru_cache(None)
def sc_mul_list():
    rng = random.Random(107)
    ops = _sc_stage_pairs(rng)
    ops += [(N - 1, N - 1)] + [(a, b) for a in SC_EDGE for b in SC_EDGE] + [(a, b) for a in LIMB[:7] for b in LIMB[:7]]
    ops += [(rng.randrange(N), rng.randrange(N)) for _ in range(500)]
    return "sc_mul", ops, [(a * b % N, 0, 0) for a, b in ops]


@functools.lru_cache(None)
def sc_inv_list():
    rng = random.Random(108)
    ops = [(a,) for a in SC_EDGE + [M.LAMBDA, (N + 1) // 2] + [rng.randrange(N) for _ in range(100)]]
    return "sc_inv", ops, [(pow(a, N - 2, N), 0, 0) for a, in ops]


@functools.lru_cache(None)
def sc_add_list():
    rng = random.Random(109)
    ops = _add_edges(N, rng) + [(a, b) for a in SC_EDGE for b in SC_EDGE]
    ops += [(rng.randrange(N), rng.randrange(N)) for _ in range(200)]
    assert any(a + b >= M.M256 for a, b in ops) and {a + b - N for a, b in ops} >= {-1, 0, 1}
    return "sc_add", ops, [((a + b) % N, 0, 0) for a, b in ops]


def _u2_list():
    return M.u2_fixed() + M.u2_split(random.Random(110))


@functools.lru_cache(None)
def split_list():
    rng = random.Random(111)
    ks = _u2_list() + [0, N // 2] + [rng.randrange(N) for _ in range(2000)]
    exp = []
    for k in ks:
        k1, k2 = M.split(k)
        assert (k1 + M.LAMBDA * k2) % N == k and abs(M.signed(k1)) < 2 ** 128 and abs(M.signed(k2)) < 2 ** 128
        exp.append((k1, k2, 0))
    return "split", [(k,) for k in ks], exp


@functools.lru_cache(None)
def gtab_list():
    pts = M.gtab_points()
    assert len(pts) == 8192 and pts[1] == T.G and pts[256 * 31 + 255] == T.mul(255 << 248, T.G)
    rng = random.Random(114)
    for k in (0, 1, N - 1, rng.randrange(N), rng.randrange(N)):  # the table walk the other lists' expectations use
        assert M.mulg(k) == T.mul(k, T.G)
    return "gtab", [(k,) for k in range(8192)], [(pt[0], pt[1], 0) if pt else (0, 0, 0) for pt in pts]


def g_row_arms(start, u1):
    """gej_add_ge's arms along ecmult's G-table loop, entered with the
    accumulator `start` (= u2 Q): the rows that double, that end at infinity,
    and that start from infinity."""
    pts, acc, arms = M.gtab_points(), start, []
    for i in range(32):
        b = (u1 >> (8 * i)) & 255
        if not b:
            continue
        g = pts[256 * i + b]
        if acc is None:
            arms.append(("a.inf", i))
        elif acc == g:
            arms.append(("double", i))
        elif acc == M.neg(g):
            arms.append(("inf", i))
        acc = T._add(acc, g)
    return acc, arms


@functools.lru_cache(None)
def verify_cases():
    """[(label, z, r, s, Q, arms, oracle verdict)]: signatures with known discrete logs and a
    chosen z (d, u1, u2 -> R = (u1 + u2 d) G, r = x(R) mod n, s = r / u2,
    z = u1 s), each followed by a twin whose r is one more."""
    rng = random.Random(112)
    out = []

    def known(label, d, u1, u2):
        d, u1, u2 = d % N, u1 % N, u2 % N
        R = M.mulg((u1 + u2 * d) % N)
        r = R[0] % N
        s = r * M.inv_n(u2) % N
        z = u1 * s % N
        q = M.mulg(d)
        end, arms = g_row_arms(M.mulg(u2 * d % N), u1)
        assert end == R
        out.append((label, z, r, s, q, arms))
        out.append((label + " twin", z, (r + 1) % N, s, q, arms))

    for row in (0, 13, 31):  # u2 = 1: the accumulator equals the table entry of row `row`
        u1 = rng.randrange(N >> 1, N - (1 << 250))
        b = (u1 >> (8 * row)) & 255
        assert b
        known("double@%d" % row, (b << (8 * row)) - u1 % (1 << (8 * row)), u1, 1)
    for row in (0, 13, 30):  # u2 = 1: infinity after row `row`, then on from infinity
        u1 = rng.randrange(N >> 1, N)
        assert (u1 >> (8 * (row + 1))) & 255
        known("inf@%d" % row, -(u1 % (1 << (8 * (row + 1)))), u1, 1)
    for row in (5,):  # the same with a GLV-split u2
        u1, u2 = rng.randrange(N >> 1, N), rng.randrange(1, N)
        known("inf@%d u2" % row, -(u1 % (1 << (8 * (row + 1)))) * M.inv_n(u2), u1, u2)
    known("z=0", rng.randrange(1, N), 0, rng.randrange(1, N))
    known("z=0 u2=1", rng.randrange(1, N), 0, 1)
    for _ in range(3):
        known("plain", rng.randrange(1, N), rng.randrange(1, N), rng.randrange(1, N))
    # R at infinity: Q = d G, r = -z / d, any s
    for _ in range(2):
        d, z, s = rng.randrange(1, N), rng.randrange(1, N), rng.randrange(1, N)
        out.append(("R inf", z, -z * M.inv_n(d) % N, s, M.mulg(d), None))
    # x(R) >= n: R = (n + t, y), r = t
    for t in [t for t in range(1, 40) if M.lift_x(N + t, False)][:2]:
        z, s = rng.randrange(1, N), rng.randrange(1, N - 1)
        q = M.key_for(M.lift_x(N + t, bool(t & 1)), t, s, z)
        out.append(("x>=n", z, t, s, q, None))
        out.append(("x>=n twin", z, t, s + 1, q, None))
    q = M.mulg(rng.randrange(1, N))
    out.append(("r=0", rng.randrange(N), 0, rng.randrange(1, N), q, None))
    out.append(("s=0", rng.randrange(N), rng.randrange(1, N), 0, q, None))
    out.append(("r=p-n", rng.randrange(N), P - N, rng.randrange(1, N), q, None))
    return [c + (T.verify_raw(*c[1:5]),) for c in out]  # the oracle's verdict, once


@functools.lru_cache(None)
def verify_list():
    cases = verify_cases()
    ops = [(z, r, s, q[0], q[1]) for _, z, r, s, q, _, _ in cases]
    return "verify", ops, [(0, 0, int(c[6])) for c in cases]


@functools.lru_cache(None)
def ecmult_list():
    """(u1, u2, Q = d G): expected (u1 + u2 d) G."""
    rng = random.Random(113)
    d = rng.randrange(1, N)
    cases = [(0, k, d) for k in _u2_list()]                                   # the Q part alone
    cases += [(k, 0, d) for k in (1, 255, 256, N - 1, 0xFF << 248, rng.randrange(N))]  # the G part alone
    cases += [(0, 0, d)]                                                      # both zero: infinity
    for _ in range(3):                                                        # u1 G = -u2 Q: infinity
        u2, d2 = rng.randrange(1, N), rng.randrange(1, N)
        cases.append((-u2 * d2 % N, u2, d2))
    cases += [(rng.randrange(N), rng.randrange(N), rng.randrange(1, N)) for _ in range(12)]
    ops, exp = [], []
    qs = {}
    for u1, u2, dd in cases:
        q = qs.setdefault(dd, M.mulg(dd))
        pt = M.mulg((u1 + u2 * dd) % N)
        ops.append((u1, u2, q[0], q[1]))
        exp.append((pt[0], pt[1], 0) if pt else (0, 0, 1))
    assert sum(e[2] for e in exp) == 4
    return "ecmult", ops, exp


LISTS = {f.__name__[:-5]: f for f in (fe_mul_list, fe_sqr_list, fe_add_list, fe_sub_list, fe_inv_list, fe_sqrt_list,
                                      sc_mul_list, sc_inv_list, sc_add_list, split_list, gtab_list, verify_list,
                                      ecmult_list)}


# ------------------------------------------------------------- coverage (CPU)
def test_stage_coverage():
    """Which reduction stages the operand lists reach, from the big-integer
    models of fe_reduce and sc_reduce (secp_model.py).

    fe_reduce: top (34 bits, always taken), the second carry w, the canon
    subtraction.  sc_reduce: h1, h2, h3 = the high parts its second, third and
    fourth sc_fold multiply by C, and the canon subtraction.  h3 = 1 and canon
    exclude each other (h3 = 1 leaves d = c - n < 2^134 < n).  h2 <= 8: after
    the first fold a < 2^256 + 2^385, so h1 < 2^130 and b < 2^256 + 2^259;
    the lists reach h2 in {0, 1, 2}."""
    _, ops, _ = fe_mul_list()
    st = [M.fe_reduce_stages(a * b) for a, b in ops]
    fe_mul = {"lanes": len(ops), "w": sum(s[2] for s in st), "canon": sum(s[3] for s in st),
              "top_max_bits": max(s[1] for s in st).bit_length()}
    _, ops, _ = fe_sqr_list()
    st = [M.fe_reduce_stages(a * a) for a, in ops]
    fe_sqr = {"lanes": len(ops), "w": sum(s[2] for s in st), "canon": sum(s[3] for s in st)}
    _, ops, _ = sc_mul_list()
    st = [M.sc_reduce_stages(a * b) for a, b in ops]
    sc_mul = {"lanes": len(ops), "h1_max_bits": max(s[1] for s in st).bit_length(),
              "h2": sorted({s[2] for s in st}), "h3": sum(s[3] for s in st), "canon": sum(s[4] for s in st)}
    print("stage coverage:", {"fe_mul": fe_mul, "fe_sqr": fe_sqr, "sc_mul": sc_mul})
    assert fe_mul["w"] >= 100 and fe_mul["canon"] >= 100
    assert fe_sqr["w"] >= 100 and fe_sqr["canon"] >= 100
    assert sc_mul["h3"] >= 100 and sc_mul["canon"] >= 100 and sc_mul["h2"] == [0, 1, 2]
    assert sc_mul["h1_max_bits"] <= 130
    # random operands reach none of them: the constructions are what does
    rng = random.Random(1)
    st = [M.fe_reduce_stages(rng.randrange(P) * rng.randrange(P)) for _ in range(2000)]
    assert not any(s[2] or s[3] for s in st)


def test_verify_cases_reach_the_arms():
    """The chosen-z signatures take the arms they are named for (traced on the
    affine oracle along the G-table rows), the valid ones verify in the oracle
    and their twins do not."""
    seen = set()
    for label, z, r, s, q, arms, ok in verify_cases():
        if arms is not None:
            assert ok == (not label.endswith("twin")), label
            seen |= set(arms)
            if label.startswith("double@"):
                assert ("double", int(label.split("@")[1].split()[0])) in arms, (label, arms)
            if label.startswith("inf@"):
                row = int(label.split("@")[1].split()[0])
                assert ("inf", row) in arms and any(a == "a.inf" and i > row for a, i in arms), (label, arms)
        elif label in ("R inf", "x>=n twin", "r=0", "s=0", "r=p-n"):
            assert not ok, label
        else:
            assert ok, label
    assert {("double", 0), ("double", 13), ("double", 31), ("inf", 0), ("inf", 13), ("inf", 30)} <= seen
    # z = 0 is really there
    assert sum(z == 0 for _, z, *_ in verify_cases()) == 4


def test_split_list_shapes():
    """The split list shows all four sign pairs, every Booth digit -4..4 in both
    halves and a non-zero top window (w = 42) in each."""
    shapes = [M.split_shape(k) for k in _u2_list()]
    assert {(a[0], b[0]) for a, b in shapes} == {(x, y) for x in (False, True) for y in (False, True)}
    for h in (0, 1):
        assert {d for sh in shapes for d in sh[h][1]} == set(range(-4, 5))
        assert any(sh[h][1][42] for sh in shapes)


# ------------------------------------------------------------------ host (CPU)
def _h(x):
    return "%064x" % x


def host_run(ask, op, ops):
    """One build/test_secp line per record -> (result0, result1, flag); None
    where the host command does not print that word."""
    out = []
    for rec in ops:
        if op == "gtab":
            a = ask("gtab %d" % rec[0])
        else:
            a = ask(op + " " + " ".join(_h(x) for x in rec))
        w = a.split()
        if op == "verify":
            out.append((0, 0, int(a)))
        elif a == "inf":
            out.append((0, 0, 1))
        elif len(w) == 2:
            out.append((int(w[0], 16), int(w[1], 16), 0))
        else:
            out.append((int(a, 16), 0, None))
    return out


def _mismatches(got, exp, ops):
    return [(i, ["%x" % x for x in ops[i]], g, e) for i, (g, e) in enumerate(zip(got, exp))
            if g[:2] != e[:2] or (g[2] is not None and g[2] != e[2])][:3]


@pytest.mark.parametrize("name", sorted(LISTS))
def test_host_list(secp_bin, name):  # noqa: F811
    op, ops, exp = LISTS[name]()
    got = host_run(secp_bin, op, ops)  # (gtab: the host binary's own table, the same gtab_entry code)
    assert len(got) == len(exp)
    assert not _mismatches(got, exp, ops)


# --------------------------------------------------------------------- device
def _limbs(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), np.uint32)


def device_run(engine, op, ops):
    import dchess
    L = dchess.lib()
    L.dc_test_secp_op.restype = C.c_int
    L.dc_test_secp_op.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    n = len(ops)
    inp = np.zeros((n, 5, 8), np.uint32)
    for i, rec in enumerate(ops):
        for k, x in enumerate(rec):
            inp[i, k] = _limbs(x)
    out = np.full((n, 17), 0xA5A5A5A5, np.uint32)
    rc = L.dc_test_secp_op(engine.ctx, OPS[op], inp.ctypes.data, n, out.ctypes.data)
    assert rc == 0, rc
    raw = out[:, :16].tobytes()
    return [(int.from_bytes(raw[64 * i:64 * i + 32], "little"), int.from_bytes(raw[64 * i + 32:64 * i + 64], "little"),
             int(out[i, 16])) for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LISTS))
def test_gpu_list(engine, name):
    op, ops, exp = LISTS[name]()
    got = device_run(engine, op, ops)
    assert not _mismatches(got, exp, ops)


@pytest.mark.gpu
def test_gpu_probe_rejects_bad_input(engine):
    """The hook's own guards: a table index just past the end and a key off the
    curve are flagged, not computed."""
    got = device_run(engine, "gtab", [(8192,), (8193,), (1,)])
    assert [g[2] for g in got] == [0xFFFFFFFF, 0xFFFFFFFF, 0] and got[2][:2] == T.G
    got = device_run(engine, "ecmult", [(1, 1, T.GX, T.GY + 1)])
    assert got[0] == (0, 0, 0xFFFFFFFF)
