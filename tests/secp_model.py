"""Big-integer models of what csrc/dc_secp.h does below a verdict, shared by
tests/test_txsig.py, tests/test_secp_device.py and the fixture generator
tests/golden/make_txsig_edge.py (test infrastructure only):

  - the GLV split (sc_split_lambda), its sign + magnitude form (sc_signed128)
    and the radix-8 Booth digits ecmult takes from each half;
  - the stages of fe_reduce and sc_reduce, so an operand list can say which of
    their rare carries and conditional subtractions it reaches;
  - crafted ECDSA signatures: for a chosen (u1, u2) = (z/s, r/s) and a message
    hash z a verifier cannot tell the signature from an honest one.
"""
import functools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import txsig as T  # noqa: E402

P, N = T.P, T.N
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
# the short lattice basis (a1, b1), (a2, b2): a_i + b_i lambda = 0 mod n
A1, B1 = 0x3086D221A7D46BCDE86C90E49284EB15, -0xE4437ED6010E88286F547FA90ABFE4C3
A2, B2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8, A1
G1 = (2 ** 384 * B2 + N // 2) // N
G2 = (2 ** 384 * -B1 + N // 2) // N
M256 = 2 ** 256
K_P = 2 ** 32 + 977  # 2^256 mod p
C_N = M256 - N       # 2^256 mod n (129 bits)

Q_WINDOW = 3                               # dc_secp.h kQWindow
Q_WINDOWS = (129 + Q_WINDOW - 1) // Q_WINDOW  # 43


def inv_n(x):
    return pow(x, N - 2, N)


def inv_p(x):
    return pow(x, P - 2, P)


# ------------------------------------------------------------------ GLV split
def split(k):
    """sc_split_lambda: (r1, r2) mod n with k = r1 + lambda r2 and |r_i| < 2^128."""
    c1 = (k * G1 + 2 ** 383) >> 384
    c2 = (k * G2 + 2 ** 383) >> 384
    r2 = (c1 * -B1 + c2 * -B2) % N
    r1 = (k - r2 * LAMBDA) % N
    return r1, r2


def signed(r):
    """sc_signed128: r mod n as a signed integer of magnitude < 2^128."""
    return r if r < N - r else r - N


def booth_digits(m, w=Q_WINDOW):
    """booth_digit<W>(m, 0 .. NW-1) of the 128-bit magnitude m."""
    out = []
    for i in range((129 + w - 1) // w):
        lo = (m >> (w * i)) & ((1 << w) - 1)
        below = (m >> (w * i - 1)) & 1 if i else 0
        out.append(lo + below - ((lo >> (w - 1)) << w))
    assert sum(d * (1 << (w * i)) for i, d in enumerate(out)) == m
    return out


def split_shape(k):
    """What ecmult sees of u2 = k: ((sign1, digits1), (sign2, digits2))."""
    return tuple((s < 0, booth_digits(abs(s))) for s in map(signed, split(k)))


def u2_fixed():
    return [1, 2, N - 1, N - 2, LAMBDA, LAMBDA + 1, N - LAMBDA, LAMBDA * LAMBDA % N, 2 ** 127, 2 ** 128 - 1, 2 ** 128,
            2 ** 128 + 1, (N + 1) // 2, (N - 1) // 2]


def largest_split(rng, tries=4000):
    """Per sign pair, the scalar whose split has the largest max(|k1|, |k2|) among
    `tries` random scalars and the corners of the split's fundamental cell."""
    best = {}
    cands = [rng.randrange(1, N) for _ in range(tries)]
    for e1 in (-1, 1):  # half-sums of the basis vectors: the cell's corners, nudged inside
        for e2 in (-1, 1):
            for nudge in (0, 1, -1, 5, -5):
                x = (e1 * A1 + e2 * A2) // 2 + nudge
                y = (e1 * B1 + e2 * B2) // 2 + nudge
                cands.append((x + LAMBDA * y) % N)
    for k in cands:
        if k == 0:
            continue
        s1, s2 = map(signed, split(k))
        key = (s1 < 0, s2 < 0)
        m = max(abs(s1), abs(s2))
        if s1 and s2 and m > best.get(key, (0, 0))[0]:
            best[key] = (m, k)
    return {key: k for key, (m, k) in best.items()}


def u2_split(rng):
    """u2 = k1 + lambda k2 for the four sign pairs and the magnitudes of the edge
    classes: 1, 4 (K), sum 4 8^w, the bit pattern (011 100)* whose Booth digits
    alternate -4, +4, 2^32 - 1, 2^32, 2^96 - 1, and the largest a search finds."""
    mags = [1, 4, sum(4 * 8 ** w for w in range(42)), sum(0b011100 * 64 ** i for i in range(21)),
            2 ** 32 - 1, 2 ** 32, 2 ** 96 - 1]
    big = largest_split(rng)
    out = []
    for n1 in (False, True):
        for n2 in (False, True):
            for m in mags:
                out.append(((-m if n1 else m) + LAMBDA * (-m if n2 else m)) % N)
            out.append(big[(n1, n2)])
    return out


# ------------------------------------------------------- reduction stage models
def fe_reduce_stages(t):
    """fe_reduce on the 512-bit t: (result, top, w, canon) -- the 34-bit `top`
    of the first fold, the second carry w, and whether fe_canon subtracts p."""
    lo, hi = t % M256, t >> 256
    s1 = lo + K_P * hi
    s, top = s1 % M256, s1 >> 256
    assert top < 2 ** 34
    s2 = s + top * K_P
    s, w = s2 % M256, s2 >> 256
    assert w <= 1 and (w == 0 or s < 2 ** 67)
    s += w * K_P
    assert s < M256
    canon = s >= P
    if canon:
        s -= P
    assert s == t % P
    return s, top, w, canon


def sc_reduce_stages(t):
    """sc_reduce on the 512-bit t: (result, h1, h2, h3, canon) -- the high parts
    the second, third and fourth sc_fold multiply by C, and whether sc_canon
    subtracts n."""
    a = t % M256 + (t >> 256) * C_N
    assert a < 2 ** (13 * 32)
    h1 = a >> 256
    b = a % M256 + h1 * C_N
    assert b < 2 ** (9 * 32)
    h2 = b >> 256
    c = b % M256 + h2 * C_N
    assert c < 2 ** (9 * 32)
    h3 = c >> 256
    d = c % M256 + h3 * C_N
    assert d < M256 and h3 <= 1
    canon = d >= N
    if canon:
        d -= N
    assert d == t % N
    return d, h1, h2, h3, canon


# ------------------------------------------------------------ crafted signatures
def lift_x(x, odd):
    """The curve point (x, y) with y of the given parity, or None."""
    if x >= P:
        return None
    y2 = (x * x * x + 7) % P
    y = pow(y2, (P + 1) // 4, P)
    if y * y % P != y2:
        return None
    return (x, P - y if (y & 1) != odd else y)


def neg(pt):
    return None if pt is None else (pt[0], (P - pt[1]) % P)


def key_for(R, r, s, z):
    """The public key Q for which (r, s) verifies z with u1 G + u2 Q = R."""
    si = inv_n(s)
    u1, u2 = z * si % N, r * si % N
    return T.mul(inv_n(u2), T._add(R, neg(T.mul(u1, T.G))))


def pk_hex(q, form):
    """form: 'c' compressed, 'u' uncompressed (0x04), 'h' hybrid (0x06 / 0x07)."""
    x, y = q
    if form == "c":
        return "%02x%064x" % (2 + (y & 1), x)
    return "%02x%064x%064x" % (4 if form == "u" else 6 + (y & 1), x, y)


def craft(u1, u2, white, black, action, odd=False):
    """A valid signature whose verification computes u1 G + u2 Q: walks the
    action's last coordinate until r = z u2 / u1 is an x coordinate.  Returns
    (action, r, s, Q)."""
    assert 0 < u1 < N and 0 < u2 < N
    act = list(action)
    while True:
        z = int.from_bytes(T.message_hash(white, black, tuple(act)), "big") % N
        r = z * u2 % N * inv_n(u1) % N
        R = lift_x(r, odd) if r else None
        if R is not None and z:
            s = r * inv_n(u2) % N
            q = key_for(R, r, s, z)
            if q is not None:
                assert z * inv_n(s) % N == u1 and r * inv_n(s) % N == u2
                return tuple(act), r, s, q
        act[3] += 1


def u1_rows(u1):
    """The (row, byte) G-table entries ecmult reads for u1."""
    return {(i, (u1 >> (8 * i)) & 255) for i in range(32)} - {(i, 0) for i in range(32)}


@functools.lru_cache(None)
def gtab_points():
    """The G table of dc_secp.h: slot 256 i + j = j 2^(8 i) G (None for j = 0),
    built by 8160 affine additions of the oracle."""
    out = []
    base = T.G
    for i in range(32):
        acc = None
        out.append(None)
        for j in range(1, 256):
            acc = T._add(acc, base)
            out.append(acc)
        base = T._add(acc, base)  # 256 * base
    return out


def mulg(k):
    """k G as 32 table additions (test_secp_device.py pins it to the oracle's mul)."""
    pts, acc = gtab_points(), None
    for i in range(32):
        b = (k >> (8 * i)) & 255
        if b:
            acc = T._add(acc, pts[256 * i + b])
    return acc
