"""Integer models of the device's arithmetic shortcuts (CPU only).

* `roll61w` (dg_correcting.hip): the correcting build's rolling step on a
  weakly reduced fingerprint (residue + 0..2 M, high dword <= 2^29) in dword
  arithmetic with explicit carries, and `fp61_canon`'s single-dword fix-up.
  Modelled bit for bit with Python integers and checked against
  (fp * 263 + nb + in) mod M over random, boundary and chained inputs.
* `mod_q_small` (dg_devutil.h): x mod q in FP64 with 1/q rounded DOWN, so the
  quotient estimate is exact or one short and a single fix-up suffices.
  Python floats are IEEE doubles; y = xh (2^32 mod q) + xl and the final
  fma are exact here (< 2^53), so only the product y * inv rounds, as on the
  device.
* `mod_q` (dg_devutil.h) and `checkpoint_slot` (dg_correcting.hip): the
  64-bit Barrett reductions that take over from q = 2^23 and |F| = 2^23,
  checked against % and // (below, with `slot_of`'s truncation to a dword).
"""
import math
import random
import struct
from fractions import Fraction

M = (1 << 61) - 1
BASE = 263
MASK29 = (1 << 29) - 1
U32 = 0xFFFFFFFF


def roll61w(fp, nb, inb):
    lo, hi = fp & U32, fp >> 32
    assert hi <= (1 << 29)
    P = lo * BASE + nb                       # one 32x32+64 multiply-add
    Q = hi * BASE
    s = ((Q >> 29) & U32) + inb
    tl = ((P & U32) + s) & U32
    carry = 1 if tl < s else 0
    th = ((P >> 32) + (Q & MASK29) + carry) & U32
    f = th >> 29
    rl = (tl + f) & U32
    rh = (th & MASK29) + (1 if rl < f else 0)
    return (rh << 32) | rl


def fp61_canon(r):
    ge = r >= M
    lo = ((r & U32) + (1 if ge else 0)) & U32
    hi = 0 if ge else r >> 32
    return (hi << 32) | lo


def test_roll61w_matches_the_residue():
    rng = random.Random(61)
    edge_fp = [0, 1, M - 1, M, M + 1, M + 2, (1 << 61) - (1 << 40), (MASK29 << 32) | U32]
    edge_nb = [0, 1, M - 1, M - 263, 1 << 60]
    for _ in range(40000):
        fp = rng.choice(edge_fp) if rng.random() < 0.2 else rng.randrange(M + 3)
        nb = rng.choice(edge_nb) if rng.random() < 0.2 else rng.randrange(M)
        inb = rng.randrange(256)
        r = roll61w(fp, nb, inb)
        assert r <= M + 2 and (r >> 32) <= (1 << 29)
        assert fp61_canon(r) == (fp * BASE + nb + inb) % M
    for _ in range(300):   # chains never leave the weak range
        fp = rng.randrange(M)
        ref = fp
        for _ in range(64):
            nb, inb = rng.randrange(M), rng.randrange(256)
            fp = roll61w(fp, nb, inb)
            ref = (ref * BASE + nb + inb) % M
            assert fp61_canon(fp) == ref


def _inv_down(q):
    inv = 1.0 / q
    if Fraction(inv) * q > 1:
        inv = struct.unpack("<d", struct.pack("<q", struct.unpack("<q", struct.pack("<d", inv))[0] - 1))[0]
    return inv


def _mod_q_small(x, q, inv):
    k1 = (1 << 32) % q
    y = float(x >> 32) * float(k1) + float(x & U32)
    assert y == (x >> 32) * k1 + (x & U32)   # exact
    u = int(y - math.floor(y * inv) * q)
    assert 0 <= u < 2 * q                    # one fix-up is enough
    return min(u, (u - q) & U32)


def test_mod_q_small_one_fixup():
    rng = random.Random(23)
    for q in (3, 4099, 16411, 33457, 65537, 524309, 1048573, 8388593):
        inv = _inv_down(q)
        k1 = (1 << 32) % q
        ymax = MASK29 * k1 + U32
        for _ in range(4000):
            x = rng.randrange(M)
            assert _mod_q_small(x, q, inv) == x % q
        for _ in range(2000):   # y just below, at and above a multiple of q
            k = rng.randrange(1, ymax // q)
            for y in (k * q - 1, k * q, k * q + 1):
                if 0 <= y <= ymax:
                    u = int(y - math.floor(float(y) * inv) * q)
                    assert 0 <= u < 2 * q


# ── the Barrett paths: mod_q (dg_devutil.h) and checkpoint_slot (dg_correcting.hip) ──
#
# From q = 2^23 on slot_of is (uint32_t)mod_q(fp, q, magic), and from
# |F| = 2^23 on the correcting kernels test a checkpoint with checkpoint_slot.
# Both estimate a quotient by the high half of a 64 x 64 multiply with
# magic = floor((2^64 - 1) / d), which is the quotient or short by at most
# two, and fix up by conditional subtracts.

U64 = (1 << 64) - 1
K_SENTINEL = 0xFFFFFFFF   # dg_layout.h: "no slot"

BIG_Q = (1 << 23, 8388617, 33554467, (1 << 31) + 11, 4294967291)
CKPT_M = (1, 2, 3, 9, 16, 17, 2047)


def umul64hi(a, b):
    assert 0 <= a <= U64 and 0 <= b <= U64
    return (a * b) >> 64


def mod_q(x, q, magic):
    qh = umul64hi(x, magic)
    r = (x - qh * q) & U64
    if r >= q:
        r -= q
    if r >= q:
        r -= q
    return r


def slot_of_big(x, q):
    """slot_of's branch for q >= 2^23: the Barrett residue truncated to a dword"""
    return mod_q(x, q, U64 // q) & U32


def checkpoint_slot(fp, f_size, m, q, k):
    """(passes, slot): f = fp mod |F| passes iff f mod m == k and f / m < q"""
    f = mod_q(fp, f_size, U64 // f_size)
    if m == 1:
        i, r = f, 0
    else:
        i = umul64hi(f, U64 // m)
        r = (f - i * m) & U64
        if r >= m:
            r -= m
            i += 1
        if r >= m:
            r -= m
            i += 1
    return (r == k and i < q), i & U32, i


def _xs(rng, q, n):
    """random fingerprints and the neighbours of multiples of q, the largest included"""
    xs = [0, 1, M - 1, q - 1, q, q + 1]
    xs += [rng.randrange(M) for _ in range(n)]
    kmax = (M - 1) // q
    for k in [1, 2, kmax - 1, kmax] + [rng.randrange(1, kmax + 1) for _ in range(n // 4)]:
        xs += [x for x in (k * q - 1, k * q, k * q + 1) if 0 <= x < M]
    return xs


def _big_qs(rng, n):
    return list(BIG_Q) + [rng.randrange(1 << 23, 1 << 32) for _ in range(n)]


def test_mod_q_barrett_matches_the_residue():
    rng = random.Random(64)
    for q in _big_qs(rng, 60):
        magic = U64 // q
        for x in _xs(rng, q, 400):
            # the estimate is short by at most two: two subtracts suffice
            assert 0 <= x // q - umul64hi(x, magic) <= 2
            assert mod_q(x, q, magic) == x % q


def test_slot_of_truncation_is_lossless():
    """encode_geometry rejects q >= 2^32 - 1, so every residue fits a dword
    and none equals kSentinel (nor kSentinel - 1, the other 'no slot' mark of
    the window chain, unless q is the largest accepted value's neighbour)."""
    rng = random.Random(32)
    for q in _big_qs(rng, 20) + [K_SENTINEL - 1]:
        assert q < K_SENTINEL
        for x in _xs(rng, q, 200):
            r = mod_q(x, q, U64 // q)
            assert r < (1 << 32) and slot_of_big(x, q) == r == x % q
            assert slot_of_big(x, q) != K_SENTINEL
    # the largest residue of the largest accepted q
    q = K_SENTINEL - 1
    assert slot_of_big(q - 1 + q * 5, q) == q - 1 == K_SENTINEL - 2


def test_checkpoint_slot_matches_divmod():
    rng = random.Random(17)
    for f_size in _big_qs(rng, 25):
        ms = list(CKPT_M) + [rng.randrange(1, 5000) for _ in range(4)] + [rng.randrange(1, f_size) for _ in range(2)]
        for m in ms:
            cap = (f_size + m - 1) // m               # the smallest table that holds every f / m
            for q in (cap, max(1, cap // 2)):      # (--max-table can cut the table below that)
                for x in _xs(rng, f_size, 40):
                    f = x % f_size
                    for k in {f % m, rng.randrange(m)}:
                        ok, slot, i = checkpoint_slot(x, f_size, m, q, k)
                        assert i == f // m and slot == i   # slot fits a dword
                        assert ok == (f % m == k and f // m < q)
                # f at multiples of m: where a short quotient estimate would show
                for j in [0, 1, (f_size - 1) // m] + [rng.randrange(0, (f_size - 1) // m + 1) for _ in range(20)]:
                    for f in (j * m - 1, j * m, j * m + 1):
                        if 0 <= f < f_size:
                            ok, slot, i = checkpoint_slot(f, f_size, m, q, f % m)
                            assert (ok, slot) == (f // m < q, f // m)
