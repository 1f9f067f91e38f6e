"""GPU: validation.LevelValidator on the tiny c1e4 denoiser and the four-episode test store (33 windows; B = 8: five batches, the last one padded;
K = 3 levels) - predict() is the denoiser on the hand-built noised input, run() accumulates exactly what the ordered replay (tests/level_refs.py)
gives for the same predictions, K draws are the full window x level cross, the sums do not depend on the sweep's batch size beyond summation order,
loss_per_level is GCDenoiser.loss at that level, the EMA swap / training flags / guidance_scale are put back, repeated passes hold no device memory,
and a hindsight sweep runs unchanged.

Measured gaps of the objective check (fp32, one MI355X) are printed by the test; its allowance is FP32_LOSS relative plus 2 * 2^-23 * rms(D) /
rms(D - a): D is an fp32 number of the size of the action while D - a is what the loss sees, so one rounding of D (and one of the generic path's own
F * c_out form) moves the level's loss by that ratio, which grows like 1 / c_out towards small sigma."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import data_refs as R  # noqa: E402
import level_refs as LR  # noqa: E402
import tolerances as T  # noqa: E402
import val_refs as V  # noqa: E402
import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import data, rollout  # noqa: E402
from mode_diffusion_policy_amd.optim import ArenaEMA  # noqa: E402

W, A, SEED, K = 10, 7, 5, 3
SIGMAS = [0.02, 0.6, 30.0]
LENGTHS = R.episode_lengths(W)                                                   # 1, 9, 10, 13: 33 windows
REAL_STEPS = sum(min(W, L - p) for L in LENGTHS for p in range(L))


def setup(dtype, B=8, levels=SIGMAS, step_goals=False, sweep_kw=None, **kw):
    den, m, st, sweep, embed = V.held_out_setup(dtype, W, A, B, SEED, step_goals, sweep_kw)
    return den, m, st, sweep, embed, M.LevelValidator(den, sweep, embed, levels=levels, **kw)


def host(b, *keys):
    return [b[k].cpu().numpy() for k in keys]


def replay(val, draws):
    """The ordered replay applied to the predict() outputs of every batch in order -> ((sq, cnt), calls)."""
    acc, calls, n = None, 0, val.num_levels
    for draw in range(draws):
        for i in range(len(val)):
            b = val.batch(i, draw)
            p = val.predict(b)
            acc = LR.level_error(p.cpu().numpy(), *host(b, "actions", "level"), n, *host(b, "action_mask", "valid"), into=acc)
            calls += 1
    return acc, calls


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_predict_is_the_denoiser_on_the_hand_built_noised_input(dtype):
    den, m, st, sweep, embed, val = setup(dtype)
    assert len(val) == 5 and val.num_levels == K and val.sigmas.dtype == torch.float32 and val.sigmas.is_cuda
    table = np.asarray(SIGMAS, np.float32)
    for i, draw in ((0, 0), (len(val) - 1, 4)):
        b = val.batch(i, draw)
        z = rollout.env_noise(V.window_noise_seeds(SEED, b["window"].tolist()), [draw] * 8, W, A, 1.0, "cuda")
        assert torch.equal(b["noise"], z)                                        # the sweep's unit-normal noise of (window, draw)
        level, sigma, noised = LR.noise_levels(*host(b, "actions", "noise", "window"), table, draw)
        assert np.array_equal(host(b, "level")[0], level) and level.tolist() == [(g + draw) % K for g in b["window"].tolist()]
        assert np.array_equal(V.bits(b["sigma"]), sigma.view(np.uint32)) and np.array_equal(V.bits(b["noised"]), noised.reshape(-1).view(np.uint32))
        got = val.predict(b)
        assert not den.training
        with torch.no_grad():
            ref = den(embed(b), torch.from_numpy(noised).cuda(), b["latent_goal"], torch.from_numpy(sigma).cuda())
        assert got.shape == (8, W, A) and got.dtype == torch.float32 and torch.isfinite(got).all() and torch.equal(got, ref)
    assert b["valid"].tolist() == [1.0] + [0.0] * 7                              # the last batch: one window, seven padding rows with a level each
    assert den.guidance_scale is None


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_run_accumulates_what_the_replay_gives_for_the_same_predictions(dtype):
    den, m, st, sweep, embed, val = setup(dtype)
    acc, calls = replay(val, K)
    res = val.run()                                                              # draws = K by default
    assert V.same(res, acc) and calls == K * 5
    assert res["count_per_level"].tolist() == [float(REAL_STEPS)] * K            # the full cross: every window at every level once
    assert all(v.is_cuda for v in res.values()) and res["sq"].shape == (K, W, A) and res["cnt"].shape == (K, W)
    assert torch.equal(res["sigmas"], val.sigmas) and bool((res["loss_per_level"] > 0).all()) and float(res["loss"]) > 0
    # the derived means, from the replay's sums; raw units: unit[a]^2 per dimension
    s = st.scale.cpu().numpy()
    unit = np.where(s != 0, 1.0 / np.where(s != 0, s, 1).astype(np.float64), 0.0)
    sq, cnt = acc[0].reshape(K, W, A), acc[1]
    close = lambda t, want: np.allclose(t.cpu().numpy(), want, rtol=1e-12, atol=0)
    raw = sq * unit ** 2
    assert close(res["mse_per_level"], raw.sum((1, 2)) / (A * cnt.sum(1))) and close(res["mse_per_level_step"], raw.sum(2) / (A * cnt))
    assert close(res["mse_per_level_dim"], raw.sum(1) / cnt.sum(1)[:, None])
    sig = np.asarray(SIGMAS, np.float32).astype(np.float64)
    lam = (sig ** 2 + 0.25) / (sig * 0.5) ** 2
    assert close(res["loss_per_level"], lam * sq.sum((1, 2)) / (A * cnt.sum(1))) and close(res["loss"], (lam * sq.sum((1, 2)) / (A * cnt.sum(1))).mean())
    # one draw: every window once, at one level each
    acc1, _ = replay(val, 1)
    res1 = val.run(draws=1)
    assert V.same(res1, acc1) and float(res1["count_per_level"].sum()) == REAL_STEPS and bool((res1["count_per_level"] > 0).all())
    # normalised units: the same sums, other means
    resn = M.LevelValidator(den, sweep, embed, levels=SIGMAS, raw_units=False).run()
    assert V.same(resn, acc) and close(resn["mse_per_level"], sq.sum((1, 2)) / (A * cnt.sum(1))) and torch.equal(resn["loss_per_level"], res["loss_per_level"])
    for kw in (dict(draws=0), dict(draws=1.5), dict(draws=True)):
        with pytest.raises(ValueError):
            val.run(**kw)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_the_sums_do_not_depend_on_the_sweeps_batch_size(dtype):
    den, m, st, sweep, embed, val8 = setup(dtype)
    val5 = M.LevelValidator(den, data.WindowSweep(st, 5, W, seed=SEED), embed, levels=SIGMAS)
    r8, r5 = val8.run(), val5.run()
    assert len(val8) == 5 and len(val5) == 7
    bound = LR.sum_bound(8, calls=K * 5) + LR.sum_bound(5, calls=K * 7)          # two ordered, accumulated sums of the same non-negative terms
    worst = 0.0
    for k in ("sq", "cnt"):
        a, b = r8[k].cpu().numpy(), r5[k].cpu().numpy()
        gap = np.abs(a - b) / np.maximum(np.maximum(a, b), np.finfo(np.float64).tiny)
        worst = max(worst, float(gap.max()))
        assert (gap <= bound).all(), (k, float(gap.max()), bound)
    print(f"batch size 8 vs 5 [{dtype}]: worst relative gap of an accumulator {worst:.3e}, bound {bound:.3e}")
    assert torch.equal(r8["count_per_level"], r5["count_per_level"])


def test_loss_per_level_is_the_training_objective_at_that_level():
    levels = [0.05, 0.5, 5.0, 50.0]
    n = len(levels)
    den, m, st, sweep, embed, val = setup("fp32", levels=levels)
    res = val.run()
    got = res["loss_per_level"].cpu().numpy()
    den.eval()
    num, dn = np.zeros(n), np.zeros(n)
    ss_d, ss_e = np.zeros(n), np.zeros(n)
    with torch.no_grad():
        for draw in range(n):
            for i in range(len(val)):
                b = val.batch(i, draw)
                pred, act, cmask = val.predict(b).double(), b["actions"].double(), (b["valid"][:, None] * b["action_mask"]).double()
                for k in range(n):
                    wk = b["valid"] * (b["level"] == k).float()                  # the rows that meet level k in this draw, with this draw's noise
                    loss, _ = den.loss(embed(b), b["actions"], b["latent_goal"], b["noise"], torch.full((8,), levels[k], device="cuda"),
                                       action_mask=b["action_mask"], sample_weight=wk)
                    d_b = A * float((wk[:, None] * b["action_mask"]).sum())
                    num[k] += float(loss) * d_b
                    dn[k] += d_b
                    c = (cmask * (b["level"] == k)[:, None])[:, :, None]
                    ss_d[k] += float((c * pred * pred).sum())
                    ss_e[k] += float((c * (pred - act) ** 2).sum())
    assert (dn == A * REAL_STEPS).all()
    want = num / dn
    gap = np.abs(got - want) / want
    allow = T.FP32_LOSS + 2 * 2.0 ** -23 * np.sqrt(ss_d / ss_e)
    for k in range(n):
        print(f"sigma {levels[k]:g}: loss_per_level {got[k]:.6e}, GCDenoiser.loss {want[k]:.6e}, relative gap {gap[k]:.3e}, allowance {allow[k]:.3e}")
    assert (gap <= allow).all(), (gap, allow)


def test_ema_swap_training_flags_and_guidance_scale_are_put_back():
    den, m, st, sweep, embed, val = setup("bf16")
    m.freeze_router()                                                            # a mixed pattern of training flags to restore
    flags = [(mod, mod.training) for mod in den.modules()]
    assert den.training and m.training and not all(f for _, f in flags)
    live_res = val.run()
    assert all(mod.training == f for mod, f in flags)
    eng = m.engine
    ema = ArenaEMA(m)
    ema.ensure(eng.arena)
    ema.flat.mul_(0.97)                                                          # an average that differs from the live weights
    eng.ensure_weights()
    live, avg, shadow = eng.arena.flat.clone(), ema.flat.clone(), eng.arena.lp.clone()
    unchanged = lambda: (eng.ensure_weights() is None and torch.equal(eng.arena.flat, live) and torch.equal(ema.flat, avg)
                         and torch.equal(eng.arena.lp, shadow))
    res = val.run(ema=ema)
    assert unchanged() and all(mod.training == f for mod, f in flags)
    ema.swap()
    manual = val.run()
    ema.swap()
    assert unchanged()
    assert all(torch.equal(res[k], manual[k]) for k in ("sq", "cnt", "loss_per_level", "loss", "mse_per_level", "count_per_level"))
    assert not torch.equal(res["sq"], live_res["sq"]) and torch.equal(res["cnt"], live_res["cnt"])
    assert all(torch.equal(val.run()[k], live_res[k]) for k in ("sq", "cnt"))    # the live weights validate as before

    den.guidance_scale = 2.0                                                     # left as the caller set it, and used
    guided = val.run()
    assert den.guidance_scale == 2.0 and all(mod.training == f for mod, f in flags)
    assert bool(torch.isfinite(guided["loss"])) and not torch.equal(guided["sq"], live_res["sq"]) and torch.equal(guided["cnt"], live_res["cnt"])
    calls = []

    def failing(batch):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("encoder failed")
        return embed(batch)
    bad = M.LevelValidator(den, sweep, failing, levels=SIGMAS)
    with pytest.raises(RuntimeError, match="encoder failed"):
        bad.run(ema=ema)
    assert len(calls) == 2 and unchanged() and all(mod.training == f for mod, f in flags) and den.guidance_scale == 2.0
    den.guidance_scale = None
    den.eval()
    val.run()
    assert not den.training and not m.training                                   # an evaluating model stays one
    for kw in (dict(sweep=object()), dict(embed=None), dict(levels=[]), dict(levels=[0.5, -1.0]), dict(levels=[0.5] * 257), dict(levels="density", num_levels=257)):
        args = {**dict(sweep=sweep, embed=embed, levels=SIGMAS), **kw}
        with pytest.raises(ValueError):
            M.LevelValidator(den, args.pop("sweep"), args.pop("embed"), **args)
    dens = M.LevelValidator(den, sweep, embed)                                   # the default: 16 quantiles of the training density
    sched = M.LevelValidator(den, sweep, embed, levels="schedule")
    assert dens.num_levels == 16 and bool((dens.sigmas[1:] > dens.sigmas[:-1]).all())
    assert torch.equal(sched.sigmas.cpu(), M.get_sigmas_exponential(10, 0.001, 80.0)[:-1])


def test_twenty_passes_hold_no_device_memory():
    den, m, st, sweep, embed, val = setup("bf16")
    for _ in range(3):
        val.run()
    torch.cuda.synchronize()
    gc.collect()
    was = gc.isenabled()
    gc.disable()                                                                 # only reference counts may free memory
    try:
        val.run()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        seen = []
        for _ in range(20):
            res = val.run()
            torch.cuda.synchronize()
            seen.append(torch.cuda.memory_allocated())
    finally:
        if was:
            gc.enable()
    assert max(seen) <= base + (1 << 20), (base, seen)
    assert torch.isfinite(res["loss"])


def test_a_hindsight_sweep_runs_unchanged():
    den, m, st, sweep, embed, val = setup("bf16", step_goals=True)
    hind = M.LevelValidator(den, data.WindowSweep(st, 8, W, seed=SEED, goal="hindsight", goal_horizon="last"), embed, levels=SIGMAS)
    b = hind.batch(0, 1)
    last = st.ep_begin.long()[b["episode"].long() + 1] - 1
    assert torch.equal(b["latent_goal"], st.step_goals[last]) and {"level", "sigma", "noised", "goal_index"} <= set(b)
    r_ep, r_hi = val.run(), hind.run()
    assert torch.equal(r_ep["cnt"], r_hi["cnt"]) and not torch.equal(r_ep["sq"], r_hi["sq"])      # another goal, the same windows and weights
    assert bool(torch.isfinite(r_hi["loss"])) and r_hi["count_per_level"].tolist() == [float(REAL_STEPS)] * K
