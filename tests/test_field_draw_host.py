"""The Pose2 draw on its 21-bit fields (box_muller_field of rome.jl_amd/csrc/rome_device_math.hpp), CPU side: what the device function
relies on is enumerated over all 2^21 fields in float32 NumPy, with every multiply-add a single-rounded fma, and the model itself is
tied to the project's oracle (ro.box_muller = ro_box_muller) bit for bit.  No tolerance anywhere: equality of bit patterns.

  * h = -ln u1 of every radius field is positive and normal (>= 2^-96, sqrt32_rn_normal's range): box_muller's `h > 0` select never takes
    the zero, so box_muller_field has none;
  * the words box_muller_field builds are the ones the draw is defined by: (f << 11) | 0x400 for the radius (its `+ 1` folded into the one
    conversion of (f << 11) | 0x401), wb << 2 for the angle (as the signed 19-bit field plus one half), pair C's fields on top of one
    funnel shift.

The single-rounded fma: a·b is exact in float64 (48 bits), the sum with c is rounded to odd in float64 (TwoSum gives the sign of what was
lost) and then to float32; with 53 >= 2·24 + 2 bits that is the correctly rounded float32 fma."""
import numpy as np

import oracle as ro

F32, U32, I32 = np.float32, np.uint32, np.int32
NF = 1 << 21
FIELDS = np.arange(NF, dtype=np.uint64)


def fma32(a, b, c):
    a, b, c = (np.asarray(v, dtype=F32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.uint64) & np.uint64(1)) == 0
    up = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, up, s).astype(F32)


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(U32)


def h_of_x(x):
    """box_muller_h_of_x / ro_box_muller's radius argument"""
    xb = bits(x)
    ke = (159 - (xb >> 23).astype(np.int64)).astype(F32)
    t = ((xb & U32(0x007FFFFF)) | U32(0x3F800000)).view(F32) - F32(1.5)
    p = np.full(t.shape, float.fromhex("0x1.4fab76p-7"), dtype=F32)
    for c in ("-0x1.1d4ffp-6", "0x1.a972ep-6", "-0x1.90d3ap-5", "0x1.94a6a8p-4", "-0x1.c72898p-3", "0x1.555544p-1", "0x1.9f324cp-2"):
        p = fma32(p, t, F32(float.fromhex(c)))
    return fma32(ke, F32(float.fromhex("0x1.62e43p-1")), -p)


def model_box_muller(wa, wb):
    """ro_box_muller in float32 NumPy (uint32 arrays in, float64 pairs out)"""
    wa, wb = np.asarray(wa, dtype=U32), np.asarray(wb, dtype=U32)
    h = h_of_x(wa.astype(F32) + F32(1.0))
    rr = np.where(h > 0, np.sqrt(np.maximum(h, F32(0))), F32(0)).astype(F32)
    a = (wb << U32(2)).view(I32).astype(F32) * F32(float.fromhex("0x1.921fb6p-32"))
    z = a * a
    sp = fma32(z, F32(-1.9515295891e-4), F32(8.3321608736e-3))
    sp = fma32(z, sp, F32(-1.6666654611e-1))
    sn = fma32(z * a, sp, a)
    cp = fma32(z, F32(2.443315711809948e-5), F32(-1.388731625493765e-3))
    cp = fma32(z, cp, F32(4.166664568298827e-2))
    cs = fma32(z * z, cp, fma32(z, F32(-0.5), F32(1.0)))
    m0, m1 = rr * (cs - sn), rr * (cs + sn)
    n0 = np.where(wb & U32(0x80000000), -m0, m0).astype(np.float64)
    n1 = np.where(wb & U32(0x40000000), -m1, m1).astype(np.float64)
    return n0, n1


def field_word(f):
    return ((f << np.uint64(11)) | np.uint64(0x400)).astype(U32)


def test_the_model_is_the_oracle_bit_for_bit():
    """every 61st field (and both ends) as radius and as angle field, and general 32-bit words, through ro_box_muller"""
    rng = np.random.default_rng(21)
    f = np.unique(np.concatenate([np.arange(0, NF, 61), [0, 1, NF - 2, NF - 1]])).astype(np.uint64)
    other = rng.integers(0, NF, len(f)).astype(np.uint64)
    gen = rng.integers(0, 1 << 32, (2, 4096)).astype(U32)
    for wa, wb in ((field_word(f), field_word(other)), (field_word(other), field_word(f)), (gen[0], gen[1]),
                   (np.array([0xFFFFFFFF, 0], dtype=U32), np.array([123, 0x20000000], dtype=U32))):
        n0, n1 = model_box_muller(wa, wb)
        want = np.array([ro.box_muller(int(a), int(b)) for a, b in zip(wa, wb)])
        assert np.array_equal(n0.view(np.uint64), want[:, 0].copy().view(np.uint64))
        assert np.array_equal(n1.view(np.uint64), want[:, 1].copy().view(np.uint64))


def test_the_radius_argument_of_every_field_is_positive_and_normal():
    h = h_of_x(field_word(FIELDS).astype(F32) + F32(1.0))
    assert (h > 0).all() and (h >= F32(2.0 ** -96)).all() and np.isfinite(h).all()
    assert h.min() == F32(2.0 ** -24) and int(np.argmin(h)) == NF - 1, "the smallest h is 2^-24, at the last field"
    assert 15.2 < h.max() < 15.3 and int(np.argmax(h)) == 0


def test_the_words_box_muller_field_builds_are_the_words_of_the_draw():
    rng = np.random.default_rng(22)
    low = rng.integers(0, 1 << 11, NF).astype(np.uint64)                        # what lies under the field in the Philox word: ignored
    w = ((FIELDS << np.uint64(11)) | low).astype(U32)
    want = field_word(FIELDS)
    # radius: (w & 0xFFFFF800) | 0x401 is the word of the draw plus one, and its conversion is float(word) + 1
    built = (w & U32(0xFFFFF800)) | U32(0x401)
    assert np.array_equal(built, want + U32(1))
    assert np.array_equal(bits(built.astype(F32)), bits(want.astype(F32) + F32(1.0)))
    # angle: int32(w << 2) >> 13 is the signed low 19 bits; sf·2^13 + 2^12 is the word of the draw shifted by two, and
    # (float(sf) + 0.5)·(π/4)·2^-18 is float(int32(wb << 2))·(π/4)·2^-31
    sf = (w << U32(2)).view(I32) >> I32(13)
    wb2 = (want << U32(2)).view(I32)
    assert np.array_equal(sf.astype(np.int64) * 8192 + 4096, wb2.astype(np.int64))
    a_new = (sf.astype(F32) + F32(0.5)) * F32(float.fromhex("0x1.921fb6p-19"))
    a_old = wb2.astype(F32) * F32(float.fromhex("0x1.921fb6p-32"))
    assert np.array_equal(bits(a_new), bits(a_old))
    # the signs: bits 31 / 30 of the word are bits 31 / 30 of w
    assert np.array_equal(w >> U32(30), want >> U32(30))
    # pair C: field = the low 11 bits of hi, then bits 10..1 of lo; field_word_c = alignbit(hi, lo << 21, 11) = (hi << 21) | ((lo << 21) >> 11)
    hi = ((rng.integers(0, 1 << 21, NF).astype(np.uint64) << np.uint64(11)) | (FIELDS >> np.uint64(10))).astype(U32)
    lo = ((rng.integers(0, 1 << 21, NF).astype(np.uint64) << np.uint64(11)) | ((FIELDS & np.uint64(0x3FF)) << np.uint64(1))
          | rng.integers(0, 2, NF).astype(np.uint64)).astype(U32)
    wc = (hi << U32(21)) | ((lo << U32(21)) >> U32(11))
    defined = (hi << U32(21)) | ((lo & U32(0x7FE)) << U32(10)) | U32(0x400)        # ro_rng_normals' rc / ac
    assert np.array_equal(defined, want)
    assert np.array_equal((wc & U32(0xFFFFF800)) | U32(0x400), want)
