"""CPU: the numpy replay of mode_val_noise_levels / mode_level_error (tests/level_refs.py) checked against what it restates - plain sums within the
bound the refs file derives, the action-error replay level by level, the window x level cross over K draws -, the level tables of
validation.level_table, and the means validation.LevelResult derives from hand-made sums."""
import math

import numpy as np
import pytest
import torch

import level_refs as LR
import val_refs as V
from mode_diffusion_policy_amd import validation
from mode_diffusion_policy_amd.gc_sampling import get_sigmas_exponential


def _case(B, W, A, K, seed):
    rng = np.random.default_rng(seed)
    pred, target = rng.standard_normal((B, W, A)).astype(np.float32), rng.standard_normal((B, W, A)).astype(np.float32)
    mask = (rng.random((B, W)) < 0.7).astype(np.float32) * rng.random((B, W)).astype(np.float32)
    weight = rng.random(B).astype(np.float32)
    level = rng.integers(0, K, B).astype(np.int32)
    return pred, target, mask, weight, level


@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("B,W,A", [(1, 1, 1), (3, 4, 3), (64, 10, 7), (65, 10, 7), (130, 2, 5), (300, 10, 7)])
def test_ordered_level_error_agrees_with_a_plain_sum_within_the_derived_bound(B, W, A, K):
    pred, target, mask, weight, level = _case(B, W, A, K, 7 * B + K)
    assert np.finfo(np.longdouble).nmant >= 63, "the plain reference needs an extended-precision accumulator"
    bound = LR.sum_bound(B)
    assert bound == LR.roundings(B) * LR.U / (1 - LR.roundings(B) * LR.U) and LR.roundings(B) == math.ceil(B / 64) + 6
    for kw in (dict(), dict(mask=mask), dict(weight=weight), dict(mask=mask, weight=weight)):
        got, want = LR.level_error(pred, target, level, K, **kw), LR.level_error_plain(pred, target, level, K, **kw)
        for g, w_, name in zip(got, want, ("sq", "cnt")):
            assert g.shape == w_.shape and np.all(np.abs(g.astype(np.longdouble) - w_) <= bound * w_), (kw.keys(), name)
        # level k's slice is the action-error replay with the level folded into the weight, bit for bit
        for k in range(K):
            sq, _, cnt = V.action_error(pred, target, kw.get("mask"), LR.folded_weight(level, k, kw.get("weight")), None)
            assert np.array_equal(got[0][k].view(np.uint64), sq.view(np.uint64)) and np.array_equal(got[1][k].view(np.uint64), cnt.view(np.uint64))
    counts = np.bincount(level, minlength=K)
    assert np.array_equal(LR.level_error(pred, target, level, K)[1], np.repeat(counts[:, None], W, 1).astype(np.float64))
    first = LR.level_error(pred, target, level, K, mask=mask)
    both = LR.level_error(target, pred, level, K, weight=weight, into=first)
    for b_, f_, s_ in zip(both, first, LR.level_error(target, pred, level, K, weight=weight)):
        assert np.array_equal(b_, f_ + s_)


def test_level_error_ignores_other_levels_and_what_is_masked_out():
    B, W, A, K = 70, 4, 3, 3
    pred, target, mask, weight, level = _case(B, W, A, K, 5)
    mask[::3] = [0.0, -1.0, np.nan, 1.0]
    weight[1::5] = np.nan
    level[::7] = np.resize(np.array([-1, K, 2 ** 31 - 1, -2 ** 31], np.int32), level[::7].shape)      # out of range: counts nowhere
    ref = LR.level_error(pred, target, level, K, mask=mask, weight=weight)
    c = V._terms(pred, target, mask, weight, None)[0]
    dead = (c == 0) | ((level < 0) | (level >= K))[:, None]
    dirty = pred.copy()
    dirty[dead] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(int(dead.sum())) % 3][:, None]
    assert dead.sum() > B and not np.isfinite(dirty).all()
    got = LR.level_error(dirty, target, level, K, mask=mask, weight=weight)
    for g, r in zip(got, ref):
        assert np.isfinite(g).all() and np.array_equal(g.view(np.uint64), r.view(np.uint64))
    inside = np.where((level >= 0) & (level < K), level, 0)
    keep = ((level >= 0) & (level < K)).astype(np.float32)
    want = LR.level_error(pred, target, inside, K, mask=mask, weight=weight * keep)                   # the same as weighting those rows 0
    assert all(np.array_equal(g, w_) for g, w_ in zip(ref, want))
    empty = LR.level_error(dirty, target, np.full(B, 1, np.int32), K, mask=mask, weight=weight)
    for arr in empty:
        assert np.array_equal(arr[[0, 2]].view(np.uint64), np.zeros_like(arr[[0, 2]]).view(np.uint64))  # an empty level is +0.0


@pytest.mark.parametrize("K", [1, 3, 16])
def test_k_draws_cover_the_window_level_cross_exactly_once(K):
    windows = np.arange(300)
    # draws 0 .. K - 1, and K consecutive draws whose window + draw stays below 2^32 from a large base: the full cross, each pair once
    for draw0 in (0, 2 ** 32 - 300 - K):
        seen = {}
        for draw in range(draw0, draw0 + K):
            lv = LR.levels_of(windows.astype(np.int32), draw, K)
            assert lv.dtype == np.int32 and lv.min() >= 0 and lv.max() < K
            for g, k in zip(windows.tolist(), lv.tolist()):
                seen[(g, k)] = seen.get((g, k), 0) + 1
        assert len(seen) == len(windows) * K and set(seen.values()) == {1}, (K, draw0)
    # window + draw past 2^32: the sum wraps before the modulus (K = 3 does not divide 2^32, so the wrap shows in the level)
    lv = LR.levels_of(windows.astype(np.int32), 2 ** 32 - 2, K)
    assert lv.tolist() == [((g + 2 ** 32 - 2) % 2 ** 32) % K for g in windows.tolist()]
    assert LR.levels_of(np.array([5], np.int32), 2 ** 32 - 2, 3).tolist() == [(5 + 2 ** 32 - 2 - 2 ** 32) % 3]
    assert LR.levels_of(np.array([-1], np.int32), 1, 16).tolist() == [0]          # a window read as uint32


def test_noise_levels_is_unfused_fp32_and_a_function_of_the_row():
    rng = np.random.default_rng(0)
    B, W, A, K = 9, 4, 3, 3
    actions, noise = rng.standard_normal((B, W, A)).astype(np.float32), rng.standard_normal((B, W, A)).astype(np.float32)
    window = rng.integers(0, 500, B).astype(np.int32)
    sigmas = np.array([0.013, 0.7, 61.0], np.float32)
    level, sigma, x = LR.noise_levels(actions, noise, window, sigmas, 4)
    assert level.dtype == np.int32 and sigma.dtype == x.dtype == np.float32 and np.array_equal(sigma, sigmas[level])
    fused = (actions.astype(np.float64) + noise.astype(np.float64) * sigma.astype(np.float64)[:, None, None]).astype(np.float32)
    assert np.abs(x - fused).max() <= 2.0 ** -23 * np.abs(fused).max() and not np.array_equal(x, fused)      # two roundings, not one
    perm = rng.permutation(B)[:5]
    l2, s2, x2 = LR.noise_levels(actions[perm], noise[perm], window[perm], sigmas, 4)
    assert np.array_equal(l2, level[perm]) and np.array_equal(s2, sigma[perm]) and np.array_equal(x2, x[perm])


@pytest.mark.parametrize("K,smin,smax,sd", [(16, 0.001, 80.0, 0.5), (1, 0.001, 80.0, 0.5), (7, 0.02, 3.0, 1.0), (256, 0.001, 80.0, 0.5)])
def test_density_levels_are_the_quantiles_of_the_training_density(K, smin, smax, sd):
    t = validation.level_table("density", num_levels=K, sigma_min=smin, sigma_max=smax, sigma_data=sd)
    assert t.dtype == torch.float64 and t.shape == (K,) and t.device.type == "cpu"
    s = t.numpy()
    assert (np.diff(s) > 0).all() and s[0] >= smin and s[-1] <= smax
    cdf = lambda x: 1.0 / (1.0 + np.exp(-(np.log(x) - math.log(sd)) / 0.5))
    lo, hi = cdf(np.float64(smin)), cdf(np.float64(smax))
    u = (np.arange(K) + 0.5) / K
    assert np.abs((cdf(s) - lo) / (hi - lo) - u).max() <= 1e-12
    s32 = t.to(torch.float32).numpy()
    assert (np.diff(s32) > 0).all() and s32[0] >= np.float32(smin) and s32[-1] <= np.float32(smax)


def test_schedule_and_explicit_levels():
    for n, smin, smax in ((10, 0.001, 80.0), (1, 0.001, 80.0), (4, 0.01, 2.0)):
        t = validation.level_table("schedule", sigma_min=smin, sigma_max=smax, num_sampling_steps=n)
        assert torch.equal(t, get_sigmas_exponential(n, smin, smax)[:-1]) and t.shape == (n,)
    assert validation.level_table([0.05, 0.5, 5, 50]).to(torch.float32).tolist() == torch.tensor([0.05, 0.5, 5, 50]).tolist()
    assert torch.equal(validation.level_table(torch.tensor([3.0, 0.25])), torch.tensor([3.0, 0.25]))          # as given, no sorting
    assert validation.level_table(np.array([1, 2])).tolist() == [1.0, 2.0]
    for bad in ([], [0.0, 1.0], [-1.0], [float("nan")], [float("inf")], [1e-50], [[1.0, 2.0]], [0.5] * 257, "quantiles", None, [True, False]):
        with pytest.raises(ValueError):
            validation.level_table(bad)
    for kw in (dict(num_levels=0), dict(num_levels=257), dict(num_levels=2.0), dict(sigma_min=0.0), dict(sigma_min=2.0, sigma_max=1.0)):
        with pytest.raises(ValueError):
            validation.level_table("density", **kw)
    for kw in (dict(num_sampling_steps=0), dict(num_sampling_steps=257)):
        with pytest.raises(ValueError):
            validation.level_table("schedule", **kw)


def test_constructor_refusals_need_no_device():
    class Den:
        sigma_data = 0.5
    with pytest.raises(ValueError, match="WindowSweep"):
        validation.LevelValidator(Den(), object(), lambda b: b)


def test_level_result_derives_each_mean_exactly_and_skips_empty_levels():
    K, W, A, sd = 3, 2, 2, 0.5
    sq = torch.tensor([[[1.0, 3.0], [4.0, 8.0]], [[0.0, 0.0], [0.0, 0.0]], [[2.0, 2.0], [0.0, 0.0]]], dtype=torch.float64)
    cnt = torch.tensor([[2.0, 2.0], [0.0, 0.0], [4.0, 0.0]], dtype=torch.float64)
    sigmas = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float32)
    res = validation.LevelResult.from_sums(sq.reshape(K, W * A), cnt, sigmas, sd)
    assert res["sq"].shape == (K, W, A) and torch.equal(res["cnt"], cnt) and torch.equal(res["sigmas"], sigmas)
    assert res["count_per_level"].tolist() == [4.0, 0.0, 4.0]
    assert res["mse_per_level"].tolist() == [16.0 / 8, 0.0, 4.0 / 8]
    assert res["mse_per_level_step"].tolist() == [[4.0 / 4, 12.0 / 4], [0.0, 0.0], [4.0 / 8, 0.0]]            # a step without a count is 0 too
    assert res["mse_per_level_dim"].tolist() == [[5.0 / 4, 11.0 / 4], [0.0, 0.0], [2.0 / 4, 2.0 / 4]]
    lam = [(s * s + sd * sd) / (s * sd) ** 2 for s in (0.5, 1.0, 2.0)]                                        # 8, 5, 4.25: exact in fp64
    assert lam == [8.0, 5.0, 4.25]
    assert res["loss_per_level"].tolist() == [8.0 * 2.0, 0.0, 4.25 * 0.5]
    assert float(res["loss"]) == (16.0 + 2.125) / 2                                                           # the empty level is not averaged in
    # raw units: unit[a]^2 per dimension on the mse entries only; a constant dimension (unit 0) contributes nothing
    unit = torch.tensor([2.0, 0.0], dtype=torch.float64)
    raw = validation.LevelResult.from_sums(sq.reshape(K, W * A), cnt, sigmas, sd, unit=unit)
    assert raw["mse_per_level"].tolist() == [4.0 * 5.0 / 8, 0.0, 4.0 * 2.0 / 8]
    assert raw["mse_per_level_dim"].tolist() == [[4.0 * 5.0 / 4, 0.0], [0.0, 0.0], [4.0 * 2.0 / 4, 0.0]]
    assert raw["mse_per_level_step"].tolist() == [[4.0 * 1.0 / 4, 4.0 * 4.0 / 4], [0.0, 0.0], [4.0 * 2.0 / 8, 0.0]]
    assert torch.equal(raw["loss_per_level"], res["loss_per_level"]) and torch.equal(raw["loss"], res["loss"]) and torch.equal(raw["sq"], res["sq"])
    # nothing at all: every mean is 0; sums of two passes add
    zero = validation.LevelResult.from_sums(torch.zeros(K, W * A, dtype=torch.float64), torch.zeros(K, W, dtype=torch.float64), sigmas, sd)
    assert float(zero["loss"]) == 0 and all(float(zero[k].abs().sum()) == 0 for k in ("mse_per_level", "mse_per_level_step", "mse_per_level_dim", "loss_per_level"))
    two = validation.LevelResult.from_sums(2 * sq, 2 * cnt, sigmas, sd)
    assert torch.equal(two["loss_per_level"], res["loss_per_level"]) and two["count_per_level"].tolist() == [8.0, 0.0, 8.0]
