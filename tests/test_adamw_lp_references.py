"""CPU: the rounding and the hash of the bf16-moment AdamW step (tests/adamw_lp_refs.py, restated from include/mode_hip.h) have the properties the
feature rests on - one-ulp error, exactness, Inf / NaN handling, unbiasedness - and let a second moment decay where round-to-nearest holds it."""
import numpy as np

import adamw_lp_refs as R


def _finite_samples():
    rng = np.random.default_rng(3)
    u = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)
    u = u[(u & R.EXP) != R.EXP]                                             # finite: normals, denormals, zeros of both signs
    edge = np.array([0x00000000, 0x80000000, 0x00000001, 0x0000FFFF, 0x00010000, 0x007FFFFF, 0x00800000, 0x3F800000, 0x3F80FFFF, 0x3F7FFFFF,
                     0x7F7F0000, 0x7F7F0001, 0x7F7FFFFF, 0x7F7EFFFF, 0xFF7FFFFF, 0xFF7F0000, 0xBF800001], dtype=np.uint32)
    return np.concatenate([edge, u])


def test_result_is_the_truncation_or_one_ulp_above_it():
    u = _finite_samples()
    rng = np.random.default_rng(4)
    for r16 in (np.zeros(u.size, np.uint32), np.full(u.size, 0xFFFF, np.uint32), rng.integers(0, 1 << 16, u.size).astype(np.uint32)):
        got = R.sr_bf16(u, r16).astype(np.int64)
        trunc = (u >> np.uint32(16)).astype(np.int64)
        assert np.all((got == trunc) | (got == trunc + 1))
        low = (u & np.uint32(0xFFFF)).astype(np.int64)
        up = low + r16.astype(np.int64) >= 1 << 16                          # the definition: up iff the discarded bits plus the random field carry
        at_max = (trunc & 0x7FFF) == R.BF16_MAX_BITS                        # ... except at the largest finite magnitude, which is truncated
        assert np.array_equal(got == trunc + 1, up & ~at_max)
    assert np.array_equal(R.sr_bf16(u, np.zeros(u.size, np.uint32)), (u >> np.uint32(16)).astype(np.uint16))


def test_bf16_representable_values_are_unchanged_for_every_random_field():
    b = np.arange(1 << 16, dtype=np.uint32)
    b = b[(b & 0x7F80) != 0x7F80]                                           # every finite bf16 value
    u = b << np.uint32(16)
    for r16 in (0, 1, 0x8000, 0xFFFF):
        assert np.array_equal(R.sr_bf16(u, np.full(u.size, r16, np.uint32)), b.astype(np.uint16))


def test_inf_and_nan_pass_through_and_the_largest_finite_value_never_becomes_inf():
    r_all = np.arange(1 << 16, dtype=np.uint32)
    for inf in (0x7F800000, 0xFF800000):
        assert np.all(R.sr_bf16(np.full(r_all.size, inf, np.uint32), r_all) == inf >> 16)
    for nan in (0x7FC00000, 0xFFC00001, 0x7F800001, 0x7F80FFFF, 0xFFFFFFFF, 0x7FBF0000):
        got = R.sr_bf16(np.full(r_all.size, nan, np.uint32), r_all)
        assert np.all(got == ((nan >> 16) | 0x40))
        assert np.all(np.isnan(R.expand(got)))                              # also a payload that lives in the discarded bits only stays a NaN
    for big in (0x7F7FFFFF, 0x7F7F0001, 0x7F7F0000, 0xFF7FFFFF):
        got = R.sr_bf16(np.full(r_all.size, big, np.uint32), r_all)
        assert np.all(got == big >> 16) and np.all(np.isfinite(R.expand(got)))
    just_below = R.sr_bf16(np.full(r_all.size, 0x7F7EFFFF, np.uint32), r_all)                # one bf16 ulp below the maximum still rounds up to it
    assert set(just_below.tolist()) == {0x7F7E, 0x7F7F}


def test_negative_values_mirror_positive_ones():
    u = _finite_samples() & np.uint32(0x7FFFFFFF)
    r16 = np.random.default_rng(5).integers(0, 1 << 16, u.size).astype(np.uint32)
    pos, neg = R.sr_bf16(u, r16), R.sr_bf16(u | np.uint32(0x80000000), r16)
    assert np.array_equal(neg, pos | np.uint16(0x8000))


def test_the_mean_over_all_random_fields_is_the_input_exactly():
    r_all = np.arange(1 << 16, dtype=np.uint32)
    # (values whose bf16 neighbours are both finite; fp64 holds every sum exactly: 2^16 terms of <= 8 significant bits at one or two adjacent exponents)
    for x in (np.float32(1.0) + np.float32(2.0 ** -10), np.float32(-3.1415927), np.float32(1e-3), np.float32(0.999) * np.float32(7.25e-5),
              np.float32(1e-41), np.float32(-2.5e38), np.float32(3.38e38)):
        u = R.f32_bits(np.array([x]))[0]
        vals = R.expand(R.sr_bf16(np.full(r_all.size, u, np.uint32), r_all)).astype(np.float64)
        assert vals.sum() / 65536.0 == float(x), (x, vals.sum() / 65536.0)
        assert len(set(vals.tolist())) == 2


def _lowbias32_int(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def _round_hash_int(seed, step, e):
    """Second formulation, python integers, straight from the header's three lines."""
    key = _lowbias32_int((seed & 0xFFFFFFFF) ^ ((0x9E3779B9 * (step + 1)) & 0xFFFFFFFF))
    return _lowbias32_int(_lowbias32_int((e & 0xFFFFFFFF) ^ key) + (e >> 32) * 0x9E3779B9)


def test_hash_matches_a_second_formulation_and_separates_steps_and_seeds():
    assert _lowbias32_int(1) == int(R.lowbias32(np.array([1]))[0]) and _lowbias32_int(0) == 0
    idx = np.array([0, 1, 2, 3, 4, 1023, 65539, (1 << 31) - 1, 1 << 31, (1 << 32) - 4, 1 << 32, (1 << 32) + 5, (5 << 32) + 77, (1 << 40) + 12], dtype=np.uint64)
    for seed, step in ((0, 1), (0, 2), (1, 1), (0xDEADBEEF, 1000), (0xFFFFFFFF, 7)):
        got = R.round_hash(seed, step, idx)
        assert [int(x) for x in got] == [_round_hash_int(seed, step, int(e)) for e in idx], (seed, step)
    n = 65536
    a, b, c = R.round_hash(0, 1, np.arange(n)), R.round_hash(0, 2, np.arange(n)), R.round_hash(1, 1, np.arange(n))
    assert np.mean(a == b) < 1e-3 and np.mean(a == c) < 1e-3
    assert np.array_equal(a, R.round_hash(0, 1, np.arange(n)))
    assert not np.array_equal(R.round_hash(0, 1, np.arange(8)), R.round_hash(0, 1, np.arange(8) + (1 << 32)))   # the high word of the index counts
    # both 16-bit fields are uniform enough to be unbiased in the mean: n = 65536 draws of mean 32767.5, sigma 18918 / sqrt(n) = 74; 6 sigma
    for field in (a & np.uint32(0xFFFF), a >> np.uint32(16)):
        assert abs(float(field.astype(np.float64).mean()) - 32767.5) < 6 * 18918.0 / np.sqrt(n)


def test_second_moment_decays_under_stochastic_rounding_and_not_under_round_to_nearest():
    beta2, steps, n = 0.999, 200, 65536
    b0, v0, out = R.decay_case(n, beta2, steps, 0)
    held = R.decay_reference(b0, beta2, steps, 0, stochastic=False)
    assert np.array_equal(held, b0)                                          # one step moves v by 0.1 % < half a bf16 ulp: every element keeps its bits
    got = R.expand(out).astype(np.float64)
    ratio = got / v0.astype(np.float64)
    want = 0.999 ** steps
    err = ratio.mean() / want - 1.0
    print(f"mean v_200 / v_0 = {ratio.mean():.6f} (exact {want:.6f}, relative error {err:+.2e}); per-element spread {ratio.std():.4f}")
    assert abs(err) < 1e-3                                                   # ~8 sigma of the mean: spread 0.025 / sqrt(65536) ~ 1e-4
