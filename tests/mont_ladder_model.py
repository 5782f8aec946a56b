"""
Plain-integer model of the Montgomery-form x-only ladder of k_varbase_mont (jubjub_amd/csrc/jj_mont.h): the map from Jubjub's
twisted Edwards form to the birationally equivalent Montgomery curve B y^2 = x^3 + A x^2 + x, the RFC 7748 ladder (xDBLADD,
one conditional swap per bit), the projective Okeya-Sakurai y-recovery (Costello-Smith, "Montgomery curves and their
arithmetic", Algorithm 5) scaled by u instead of divided by y1, the map back to Edwards and the masks of the exceptional inputs.
Step for step the order of operations of the device code, over exact integers mod q; tests/test_mont_ladder_cpu.py holds it
to the oracle.
"""
from oracle import jubjub_ref as J

Q = J.Q
D = J.EDWARDS_D
# a = -1:  A = 2(a + d)/(a - d),  B = 4/(a - d),  a24 = (A - 2)/4
MONT_A = 2 * (-1 + D) * pow(-1 - D, -1, Q) % Q
MONT_B = 4 * pow(-1 - D, -1, Q) % Q
A24 = (MONT_A - 2) * pow(4, -1, Q) % Q
assert MONT_A == 40962 and MONT_B == (-40964) % Q and A24 == 10240
NBITS = 252          # bits 251..0 of the scalar, as the reference's ladder (it skips the top four)


def to_x1(p):
    """affine x1 = (1 + v)/(1 - v) of an Edwards point; a zero denominator (v = 1: the identity) is replaced by 1 and flagged"""
    u, v = p
    den = (1 - v) % Q
    flag = den == 0
    return (1 + v) * pow(den if not flag else 1, -1, Q) % Q, flag


def xdbladd(x1, x2, z2, x3, z3):
    """RFC 7748 section 5: (x2:z2) <- 2 (x2:z2), (x3:z3) <- (x2:z2) + (x3:z3), difference x1"""
    a, b = (x2 + z2) % Q, (x2 - z2) % Q
    aa, bb = a * a % Q, b * b % Q
    e = (aa - bb) % Q
    c, d = (x3 + z3) % Q, (x3 - z3) % Q
    da, cb = d * a % Q, c * b % Q
    x3n = (da + cb) ** 2 % Q
    z3n = x1 * (da - cb) ** 2 % Q
    x2n = aa * bb % Q
    z2n = e * (aa + A24 * e) % Q
    return x2n, z2n, x3n, z3n


def ladder(x1, k):
    """(X_k : Z_k), (X_{k+1} : Z_{k+1}) for the bits 251..0 of k, from (1 : 0) and (x1 : 1)"""
    x2, z2, x3, z3 = 1, 0, x1, 1
    prev = 0
    for i in range(NBITS - 1, -1, -1):
        b = (k >> i) & 1
        if b ^ prev:
            x2, z2, x3, z3 = x3, z3, x2, z2
        prev = b
        x2, z2, x3, z3 = xdbladd(x1, x2, z2, x3, z3)
    if prev:
        x2, z2, x3, z3 = x3, z3, x2, z2
    return x2, z2, x3, z3


def recover(u, x1, xq, zq, xp, zp):
    """Okeya-Sakurai y-recovery of Q = (xq : zq) from P = (x1, y1) and Q + P = (xp : zp), every coordinate scaled by u with
    y1 = x1 / u (no division), then Montgomery (X : Y : Z) -> Edwards (X (X + Z) : Y (X - Z) : Y (X + Z))"""
    v1 = x1 * zq % Q
    v2 = (xq + v1) % Q
    v3 = (xq - v1) ** 2 * xp % Q
    t = 2 * MONT_A * zq % Q
    v2 = (v2 + t) * (x1 * xq + zq) % Q
    v2 = (v2 - t * zq) * zp % Q
    Y = u * (v2 - v3) % Q
    w = 2 * MONT_B * x1 % Q * zq % Q * zp % Q
    X, Z = w * xq % Q, w * zq % Q
    return X * (X + Z) % Q, Y * (X - Z) % Q, Y * (X + Z) % Q


def varbase(p, k):
    """k P as a projective Edwards (U : V : Z), exceptional inputs by the device's masks"""
    u, v = p
    x1, ident = to_x1(p)
    xq, zq, xp, zp = ladder(x1, k)
    U, V, Z = recover(u, x1, xq, zq, xp, zp)
    odd = (k >> 0) & 1
    # order of the device's selects: the later one wins
    if zp == 0:                      # (k + 1) P = O: k P = -P
        U, V, Z = -u % Q, v, 1
    if xq == 0 and zq != 0:          # k P = (0, 0): Edwards (0, -1)
        U, V, Z = 0, Q - 1, 1
    if zq == 0:                      # k P = O
        U, V, Z = 0, 1, 1
    if x1 == 0:                      # P = (0, -1): identity for even k, P for odd
        U, V, Z = (0, Q - 1, 1) if odd else (0, 1, 1)
    if ident:                        # P = O
        U, V, Z = 0, 1, 1
    return U, V, Z


def affine(p):
    U, V, Z = p
    zi = pow(Z, -1, Q)
    return U * zi % Q, V * zi % Q
