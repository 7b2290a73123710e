"""The argument the lo-half split of the matrix-core GP loop rests on
(csrc/kf_gp_mfma.h gpm_exp_split), as a NumPy model: hi is m truncated to f16
(round toward zero), so m - hi is a suffix of m's significand and the f32
subtraction is exact.  The rounded f16 result of the single-rounding FMA
fma(hi, -1, m) is therefore the f16 rounding of that f32 difference, which is
what the default split computes in two steps."""
import numpy as np

E_MIN, E_MAX = -40, 14          # the loop keeps m <= 2^14
PER_BINADE = 4096


def rtz_f16(m):
    """float32 m >= 0 (below the f16 overflow) truncated to float16: the
    nearest-even conversion, stepped down where it rounded up."""
    m = np.asarray(m, dtype=np.float32)
    h = m.astype(np.float16)
    up = h.astype(np.float32) > m
    down = (h.view(np.uint16) - np.uint16(1)).view(np.float16)      # positive f16: the next value toward zero
    return np.where(up, down, h).astype(np.float16)


def split_model(m):
    """(hi, lo) float16 of float32 m: hi = rtz(m), lo = rne(m - hi) from the exact float64 difference."""
    m = np.asarray(m, dtype=np.float32)
    hi = rtz_f16(m)
    d64 = m.astype(np.float64) - hi.astype(np.float64)
    # float64 -> float16 directly would be one rounding; numpy rounds to nearest even
    return hi, d64.astype(np.float16)


def binade_values(e, rng, n=PER_BINADE):
    """float32 values in [2^e, 2^(e+1)): random significands, all ones, every single bit, the ends."""
    frac = rng.integers(0, 1 << 23, n, dtype=np.uint32)
    special = np.array([0, (1 << 23) - 1] + [1 << b for b in range(23)] +
                       [((1 << 23) - 1) ^ (1 << b) for b in range(23)] +
                       [((1 << 23) - 1) >> b << b for b in range(23)], dtype=np.uint32)
    frac = np.concatenate([frac, special])
    bits = (np.uint32(e + 127) << np.uint32(23)) | frac
    return bits.view(np.float32)


def boundary_values():
    """0 and the f16 subnormal / underflow boundaries with their float32 neighbours."""
    out = [np.float32(0.0)]
    for e in (-14, -24, -25):
        v = np.float32(2.0 ** e)
        out += [v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(1)),
                np.nextafter(np.nextafter(v, np.float32(0)), np.float32(0)),
                np.nextafter(np.nextafter(v, np.float32(1)), np.float32(1))]
    out += [np.float32(2.0 ** -24 * 1.5), np.float32(2.0 ** -23), np.float32(2.0 ** -149), np.float32(2.0 ** 14)]
    return np.array(out, dtype=np.float32)


def all_values(seed=0):
    rng = np.random.default_rng(seed)
    return np.concatenate([binade_values(e, rng) for e in range(E_MIN, E_MAX)] + [boundary_values()])


def test_hi_is_truncation():
    m = all_values()
    hi = rtz_f16(m).astype(np.float64)
    assert np.all(hi <= m) and np.all(hi >= 0)
    # no f16 value lies strictly between hi and m
    nxt = (rtz_f16(m).view(np.uint16) + np.uint16(1)).view(np.float16).astype(np.float64)
    assert np.all(nxt > m.astype(np.float64))


def test_f32_residual_is_exact():
    m = all_values()
    assert m.size > (E_MAX - E_MIN) * 4000
    hi = rtz_f16(m)
    d32 = m - hi.astype(np.float32)                                 # float32 arithmetic
    assert d32.dtype == np.float32
    d64 = m.astype(np.float64) - hi.astype(np.float64)              # exact: both are float32 values
    assert np.array_equal(d32.astype(np.float64), d64)
    # so rounding the float32 residual to f16 is the single rounding of the exact one
    lo_two_step = d32.astype(np.float16)
    lo_one_step = d64.astype(np.float16)
    assert np.array_equal(lo_two_step.view(np.uint16), lo_one_step.view(np.uint16))
    assert np.array_equal(split_model(m)[1].view(np.uint16), lo_two_step.view(np.uint16))


def test_residual_below_one_f16_step_and_22_bits_kept():
    m = all_values()
    hi, lo = split_model(m)
    m64, hi64, lo64 = m.astype(np.float64), hi.astype(np.float64), lo.astype(np.float64)
    normal = m64 >= 2.0 ** -14
    # hi + lo carries m to 2^-22 relative where hi is a normal f16 and lo does not underflow
    big = m64 >= 2.0 ** -3
    assert np.all(np.abs(hi64 + lo64 - m64)[big] <= m64[big] * 2.0 ** -21)
    # the residual is below one step of hi's binade (normal) or of the subnormal grid
    step = np.where(normal, 2.0 ** (np.floor(np.log2(np.maximum(m64, 2.0 ** -14))) - 10), 2.0 ** -24)
    assert np.all(m64 - hi64 < step)
    # underflow: below the smallest subnormal hi is exactly 0 and lo carries what f16 can
    tiny = m64 < 2.0 ** -24
    assert np.all(hi64[tiny] == 0)
