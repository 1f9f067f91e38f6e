"""GPU: validation.Validator on the tiny c1e4 denoiser and the four-episode test store - predict() is the sampler on the window's own noise, run()
accumulates exactly what the ordered reference (tests/val_refs.py) gives for the same predictions, the EMA swap and the training flag are put back,
a second pass replays the captured sampler, and repeated passes hold no device memory."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import data_refs as R  # noqa: E402
import val_refs as V  # noqa: E402
import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import data, rollout  # noqa: E402
from mode_diffusion_policy_amd.optim import ArenaEMA  # noqa: E402

W, A, SEED = 10, 7, 5


def setup(dtype, B=8, **kw):
    den, m, st, sweep, embed = V.held_out_setup(dtype, W, A, B, SEED)
    return den, m, st, sweep, embed, M.Validator(den, sweep, embed, **kw)


def unit_of(st):
    s = st.scale.cpu().numpy()
    return np.where(s != 0, 1.0 / np.where(s != 0, s, 1).astype(np.float64), 0.0)


def reference(val, unit, draws=1):
    """The ordered reference applied to the predict() outputs of every batch in order; also the number of real steps."""
    acc, steps = None, 0
    for draw in range(draws):
        for i in range(len(val)):
            b = val.batch(i, draw)
            p = val.predict(b)
            acc = V.action_error(p.cpu().numpy(), b["actions"].cpu().numpy(), b["action_mask"].cpu().numpy(), b["valid"].cpu().numpy(), unit, into=acc)
            steps += int((b["action_mask"] * b["valid"][:, None]).sum())
    return acc, steps


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_predict_is_the_sampler_on_the_windows_noise(dtype):
    den, m, st, sweep, embed, val = setup(dtype)
    assert len(val) == 5
    sig = rollout.get_noise_schedule(10, "exponential", 1e-3, 80.0, "cuda")
    for i in (0, len(val) - 1):
        b = val.batch(i)
        z = rollout.env_noise(V.window_noise_seeds(SEED, b["window"].tolist()), [0] * 8, W, A, 80.0, "cuda")
        assert torch.equal(b["noise"], z)                                        # the sweep's noise, scaled by sigma_max in its launch
        got = val.predict(b)
        ref = M.sample_ddim(den, embed(b), b["noise"], b["latent_goal"].unsqueeze(1), sig, disable=True)
        assert got.shape == (8, W, A) and torch.isfinite(got).all() and torch.equal(got, ref)
    assert b["valid"].tolist() == [1.0] + [0.0] * 7                              # the last batch: one window, seven padding rows


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_run_accumulates_what_the_reference_gives_for_the_same_predictions(dtype):
    den, m, st, sweep, embed, val = setup(dtype)
    lengths = R.episode_lengths(W)
    real_steps = sum(min(W, L - p) for L in lengths for p in range(L))
    acc, steps = reference(val, unit_of(st))
    assert steps == real_steps
    res = val.run()
    assert V.same(res, acc)
    assert float(res["count"]) == real_steps                                     # the partial last batch's padding rows count nothing
    sq, cnt = acc[0].reshape(W, A), acc[2]
    close = lambda t, want: np.allclose(t.cpu().numpy(), want, rtol=1e-12, atol=0)
    assert close(res["mse"], sq.sum() / (A * cnt.sum())) and close(res["mae"], acc[1].sum() / (A * cnt.sum()))
    assert close(res["mse_per_step"], sq.sum(1) / (A * cnt)) and close(res["mse_per_dim"], sq.sum(0) / cnt.sum())
    assert close(res.mse_executed(3), sq[:3].sum() / (A * cnt[:3].sum())) and close(res.mse_executed(W), sq.sum() / (A * cnt.sum()))
    assert all(v.is_cuda for v in res.values()) and float(res["mse"]) > 0
    # two draws: twice the steps, other noise on the second pass
    acc2, _ = reference(val, unit_of(st), draws=2)
    res2 = val.run(draws=2)
    assert V.same(res2, acc2) and float(res2["count"]) == 2 * real_steps and not np.array_equal(acc2[0], 2 * acc[0])
    # normalised units
    valn = M.Validator(den, sweep, embed, raw_units=False)
    assert valn.unit is None
    accn, _ = reference(valn, None)
    resn = valn.run()
    assert V.same(resn, accn) and not np.array_equal(accn[0], acc[0]) and np.array_equal(accn[2], acc[2])
    # another batch size sweeps the same windows: the same number of real steps (15 padding rows in its last batch)
    res16 = M.Validator(den, data.WindowSweep(st, 16, W, seed=SEED), embed).run()
    assert float(res16["count"]) == real_steps and torch.isfinite(res16["mse"])


def test_ema_swap_and_training_flag_are_put_back():
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
    assert all(torch.equal(res[k], manual[k]) for k in ("sq", "ab", "cnt", "mse", "mae", "count", "mse_per_step", "mse_per_dim"))
    assert not torch.equal(res["sq"], live_res["sq"]) and torch.equal(res["cnt"], live_res["cnt"])
    assert all(torch.equal(val.run()[k], live_res[k]) for k in ("sq", "ab", "cnt"))     # the live weights validate as before

    calls = []

    def failing(batch):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("encoder failed")
        return embed(batch)
    bad = M.Validator(den, sweep, failing)
    with pytest.raises(RuntimeError, match="encoder failed"):
        bad.run(ema=ema)
    assert len(calls) == 2 and unchanged() and all(mod.training == f for mod, f in flags)
    den.eval()
    val.run()
    assert not den.training and not m.training                                   # an evaluating model stays one
    for kw in (dict(draws=0), dict(draws=1.5)):
        with pytest.raises(ValueError):
            val.run(**kw)


def _graphs(m):
    return {k: id(v["graph"]) for k, v in m._route_cache.items() if isinstance(v, dict) and "graph" in v}


def test_a_second_pass_replays_the_captured_sampler():
    den, m, st, sweep, embed, val = setup("bf16")
    val.run()                                                                    # five batches, the last one padded: one shape
    first = _graphs(m)
    assert len(first) == 1 and not getattr(val.policy, "_chunk_graphs", None)    # ddim: MoDeDiT's fused chain, one entry
    val.run(draws=2)
    assert _graphs(m) == first
    with torch.no_grad():                                                        # weights move between validations: still no new capture
        for p in m.parameters():
            p.mul_(1.001)
    moved = val.run()
    assert _graphs(m) == first and torch.isfinite(moved["mse"])
    # a sampler that takes the policy's own capture path: one graph in the policy's cache, however many passes
    vala = M.Validator(den, sweep, embed, sampler_type="euler_ancestral")
    vala.run()
    vala.run()
    assert len(vala.policy._chunk_graphs) == 1


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
    assert torch.isfinite(res["mse"])
