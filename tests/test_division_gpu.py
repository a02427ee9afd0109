"""The shared-denominator division of the pair sweeps (csrc/sph_device.h: recip_prepare + div_shared) on the GPU, exhaustively where that is
possible: div_shared forms RN(a/d) with ONE residual correction, which Markstein's theorem allows when y = recip_prepare(d).y is RN(1/d).
Whether it is depends on what v_rcp_f32 returns, so this file measures it instead of assuming it:

(a) recip_prepare over all 2^23 significands of every binade the sweeps divide in; E = the denominators with y != RN(1/d);
(b) every d of E, and the all-ones significand of every binade in any case, under all 2^23 numerator significands of a binade in both signs:
    one correction == two corrections == numpy's a/d;
(c) all 2^23 significands as ordinary denominators, 68 numerators each: one correction == numpy's a/d;
(d) +-0 over a floored divisor stays 0.
numpy's f32 `/` is the IEEE divide of the host and is the reference throughout (the same one the oracle's divisions use).

Scaling numerator or denominator by a power of two scales every intermediate of the sequence exactly (nothing here comes near the denormal
range or overflow), so once (a) has shown y = RN(1/d) for a significand in every binade, (b) and (c) need one numerator binade per denominator,
and (c) one denominator binade."""
import math

import numpy as np
import pytest

from cfd_taichi_amd import _native as nat
from harness import bits

pytestmark = pytest.mark.gpu

M = 1 << 23                      # significands per binade
ALL_ONES = M - 1
H = 0.1                          # support radius of every scene (4 * particle_radius); a pair passes the 1e-5 gate with 1e-5 h < r <= h
SCALE = 32                       # the staged sweeps carry r (and so h * r) times 2^32 (Consts::h_s, grad_w_scaled)
NUM_SHIFT = 8                    # numerators sit 2^8 above their denominator ((b), (c)); any shift gives the same significands (see above)


def binades():
    """Exponents e (d in [2^e, 2^(e+1))) of the divisors the sweeps meet: both ends and the middle of h * r and of the same times 2^32, and
    the two binades around rho^2 ~ 1e6 (densities within ~ +-20 % of rho_0 = 1000) of the pressure solvers."""
    lo, hi = math.floor(math.log2(1e-5 * H * H)), math.floor(math.log2(H * H))
    hr = [lo, (lo + hi) // 2, hi]
    return hr + [e + SCALE for e in hr] + [math.floor(math.log2(1e6)), math.floor(math.log2(1e6)) + 1]


def binade(e, mant=None):
    """The floats 2^e * (1 + m / 2^23) for the significands `mant` (all of them by default), built from their bits."""
    mant = np.arange(M, dtype=np.uint32) if mant is None else np.asarray(mant, dtype=np.uint32)
    return (np.uint32((e + 127) << 23) | mant).view(np.float32)


def same_quotients(got, ref, what, a, d):
    bad = np.flatnonzero(bits(got) != bits(ref))
    print("%s: %d of %d differ" % (what, len(bad), got.size))
    assert len(bad) == 0, "%s differs at %d of %d; first: a=%r (0x%08x) d=%r (0x%08x): %r vs %r" % (
        what, len(bad), got.size, a[bad[0]], bits(a)[bad[0]], d[bad[0]], bits(d)[bad[0]], got[bad[0]], ref[bad[0]])


@pytest.fixture(scope="module")
def exceptional():
    """(a): {binade: significands whose refined reciprocal is not RN(1/d)}, measured once for the module."""
    E = {}
    ones = np.ones(M, dtype=np.float32)
    for e in binades():
        d = binade(e)
        y = nat.selftest_math(nat.MATH_RECIP, ones, d)
        E[e] = np.flatnonzero(bits(y) != bits(np.float32(1.0) / d))
        print("binade 2^%d: recip_prepare(d).y != RN(1/d) for %d significands: %s" % (e, len(E[e]), ["0x%06x" % m for m in E[e][:40]]))
    return E


def test_reciprocal_is_correctly_rounded_outside_a_small_set(exceptional):
    """(a) The Newton step cannot reach RN(1/d) for the all-ones significand, whatever v_rcp_f32 returns within its 1 ulp; from a v_rcp_f32
    that is 1 ulp high it also misses 32 more.  Anything beyond those 33 per binade means the reciprocal is not what the one-step quotient
    was argued from, and (b) could not run every numerator against every such d in a test's time."""
    for e, m in exceptional.items():
        assert len(m) <= 33, "binade 2^%d: %d exceptional significands" % (e, len(m))


def test_exceptional_denominators_all_numerators(exceptional):
    """(b) For every d of E and for the all-ones significand of every binade: all 2^23 numerator significands, both signs."""
    am = binade(0)
    for e, m in exceptional.items():
        for mant in sorted(set(m.tolist()) | {ALL_ONES}):
            d1 = binade(e, [mant])[0]
            a = np.concatenate([am, -am]) * np.float32(2.0 ** (e + NUM_SHIFT))
            d = np.full_like(a, d1)
            one, two = nat.selftest_math(nat.MATH_DIV_SHARED, a, d), nat.selftest_math(nat.MATH_DIV_SHARED_TWO_STEP, a, d)
            what = "d = 2^%d * 1.[0x%06x]" % (e, mant)
            same_quotients(one, two, what + ": one correction vs two", a, d)
            same_quotients(one, a / d, what + ": one correction vs a/d", a, d)


SLICES = 16


@pytest.mark.parametrize("part", range(SLICES))
def test_ordinary_denominators(part, exceptional):
    """(c) Every significand as a denominator (1/16 of them per case) with 64 numerators:
    - 32 random ones of either sign;
    - for k = 1..8 the float next to d * RN(k/d) and its two neighbours;
    - 8 whose quotient lies right beside a rounding boundary, the inputs a division sequence gets wrong first: with D the 24-bit integer
      significand of d (odd) and X = r / D mod 2^25 for r = +-1, +-3, +-5, +-7, the integer A = (D X - r) / 2^25 is a float's significand and
      A 2^25 / D = X - r/D: X is odd, so the quotient's significand is a float's plus half an ulp minus r/(2 D) ulp, |r/(2 D)| < 2^-21.
      (Where D is even or X < 2^24 there is no such A for that r; a random numerator takes the place.)"""
    e = binades()[1]
    mant = np.arange(part * (M // SLICES), (part + 1) * (M // SLICES), dtype=np.uint32)
    d1 = binade(e, mant)
    d64 = d1.astype(np.float64)
    rng = np.random.default_rng(1000 + part)

    def random_numerators():
        sign = rng.integers(0, 2, len(mant), dtype=np.uint32) << np.uint32(31)
        return ((bits(binade(e + NUM_SHIFT, rng.integers(0, M, len(mant), dtype=np.uint32)))) | sign).view(np.float32)

    cols = [random_numerators() for _ in range(32)]
    for k in range(1, 9):
        q = (np.float32(k * 2.0 ** (e + NUM_SHIFT)) / d1).astype(np.float32)
        a0 = (d64 * q.astype(np.float64)).astype(np.float32)          # the product is exact in f64 (24 x 24 bits)
        cols += [a0, (bits(a0) - np.uint32(1)).view(np.float32), (bits(a0) + np.uint32(1)).view(np.float32)]
    D = (mant | np.uint32(M)).astype(np.uint64)
    inv = D.copy()                                                    # 1/D mod 2^32 for odd D (Newton: each pass doubles the valid low bits)
    for _ in range(5):
        inv = (inv * ((np.uint64(2) - D * inv) & np.uint64(0xffffffff))) & np.uint64(0xffffffff)
    hard = 0
    for r in (1, -1, 3, -3, 5, -5, 7, -7):
        X = (inv * np.uint64(abs(r))) & np.uint64((1 << 25) - 1)
        if r < 0:
            X = (np.uint64(1 << 25) - X) & np.uint64((1 << 25) - 1)
        P = (D * X).astype(np.int64) - r
        ok = ((D & np.uint64(1)) == 1) & (X >= np.uint64(1 << 24)) & ((P & ((1 << 25) - 1)) == 0)
        A = (P >> 25).astype(np.float32) * np.float32(2.0 ** (e + NUM_SHIFT - 23))
        hard += int(ok.sum())
        cols.append(np.where(ok, A, random_numerators()).astype(np.float32))
    print("numerators beside a rounding boundary: %d of %d (denominator, r) combinations" % (hard, 8 * len(mant)))
    assert hard > 1.5 * len(mant)                                     # about a quarter of the combinations have one: D odd and X in the upper half
    a = np.stack(cols).ravel()
    d = np.tile(d1, len(cols))
    assert len(cols) == 64 and np.all(np.isfinite(a)) and np.all(np.abs(a) >= 2.0 ** (e + NUM_SHIFT - 2))
    keep = np.tile(~np.isin(mant, exceptional[e]), len(cols))       # the exceptional d have all their numerators in (b); none are left out
    a, d = a[keep], d[keep]
    same_quotients(nat.selftest_math(nat.MATH_DIV_SHARED, a, d), a / d, "ordinary denominators %d/%d, %d quotients" % (part + 1, SLICES, a.size), a, d)


def test_zero_numerators_over_a_floored_divisor():
    """(d) A pair the 1e-5 gate closes has s = 0 and numerators +-0; its divisor (0 for coincident particles) is raised to kDenFloor = 1e-30 and
    the quotient must be a zero: the sweeps add it to sums that start at +0, where either zero changes nothing."""
    d = np.float32([0.0, 1e-45, 1e-38, 9.99e-31, 1e-30, 1.0001e-30, 1e-20, 1e-7, 0.01, 4.0e7])
    for zero in (np.float32(0.0), np.float32(-0.0)):
        a = np.full_like(d, zero)
        got = nat.selftest_math(nat.MATH_DIV_SHARED_FLOORED, a, d)
        print("%r / max(d, 1e-30): bits %s" % (zero, ["0x%08x" % b for b in bits(got)]))
        assert np.all((bits(got) & np.uint32(0x7fffffff)) == 0)
        assert np.array_equal(bits(nat.selftest_math(nat.MATH_DIV_SHARED, a, np.maximum(d, np.float32(1e-30)))), bits(got))
    # and above the floor the max is the identity: the floored op is the plain one
    a = np.float32([1.0, -3.0, 0.5]); d = np.float32([1e-7, 2e-4, 0.01])
    assert np.array_equal(bits(nat.selftest_math(nat.MATH_DIV_SHARED_FLOORED, a, d)), bits(a / d))
