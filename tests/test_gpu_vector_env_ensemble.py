"""Temporal ensembling in rollout.VectorEnvPolicy on the MI355X (c1e4 weights): every replanned plan against the fused sampler on the same
gathered batch (bit for bit), every emitted action against the rule restated in fp64 over those recomputed plans
(tests/test_vector_env_ensemble.py::ensemble_reference), the bit identities (stride = window is the policy without the option; an environment
alone emits the same stream), reset, pauses, the launch / replay / sync budget, raw frames, and flat device memory."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mode_diffusion_policy_amd import gc_sampling, rollout  # noqa: E402

from test_gpu_vector_env import SIGMA_MAX, build, policy  # noqa: E402
from test_vector_env_ensemble import ensemble_reference  # noqa: E402

W = 10                                                       # the c1e4 model's action_seq_len


def _events(n, steps, rng):
    """Staggered episodes: one or two environments reset at each of the listed steps, every environment pauses on ~20 % of the steps."""
    resets = {t: sorted(rng.choice(n, size=int(rng.integers(1, 3)), replace=False).tolist()) for t in (2, 5, 9, 12, 19, 26)}
    active = rng.random((steps, n)) > 0.2
    return resets, active


def _bucket(n, m):
    return next(b for b in rollout._buckets(n) if b >= m)


class Restated:
    """Host bookkeeping of the contract: local times and, per environment, every plan since its reset as (birth time, [W, A] fp64), recomputed
    from (seed, draw) with rollout.env_noise + the fused sampler at the policy's bucket."""

    def __init__(self, pol, den, n, s, m_ens, chunk_obs):
        self.pol, self.den, self.n, self.s, self.m = pol, den, n, s, m_ens
        self.K = -(-W // s)
        self.t = [0] * n
        self.plans = [[] for _ in range(n)]
        self.chunk_obs = chunk_obs                           # rows -> the observation tokens of the gathered batch
        self.worst = 0.0

    def reset(self, envs):
        for b in envs:
            self.t[b], self.plans[b] = 0, []

    def step(self, step_inputs, goal, act, seeds, A):
        pol, n, s = self.pol, self.n, self.s
        envs = [b for b in range(n) if act[b] and self.t[b] % s == 0]
        draws = pol.draws.cpu().tolist()
        out = pol.step(step_inputs, goal, active=act)
        assert pol.replanned == envs
        if envs:
            rows = envs + [envs[-1]] * (_bucket(n, len(envs)) - len(envs))
            x0 = rollout.env_noise([seeds[r] for r in rows], [draws[r] for r in rows], W, A, SIGMA_MAX, "cuda")
            ref = gc_sampling.sample_ddim(self.den, {"state_images": self.chunk_obs(rows)}, x0, goal[rows].contiguous(),
                                          pol._schedule(goal.device), disable=True)
            assert torch.equal(pol.plans[envs], ref[:len(envs)]), "the newest plans are the recomputed plans, exactly"
            for k, b in enumerate(envs):
                self.plans[b].append((self.t[b], ref[k].double().cpu().numpy()))
        assert pol.draws.cpu().tolist() == [d + (b in envs) for b, d in enumerate(draws)]
        got = out.double().cpu().numpy()
        for b in range(n):
            if not act[b]:
                assert not got[b].any()                      # inactive: a zero row, the local time stands
                continue
            t = self.t[b]
            live = [(tp, p) for tp, p in self.plans[b] if 0 <= t - tp < W]
            assert 1 <= len(live) <= self.K
            want = ensemble_reference(self.plans[b], t, W, self.m)
            # K fp32 fused multiply-adds, one divide and the fp32 weight table against fp64: (K + 2) 2^-23 max|x| per element
            bound = (self.K + 2) * 2.0 ** -23 * np.abs(np.stack([p[t - tp] for tp, p in live])).max(0)
            err = np.abs(got[b] - want)
            self.worst = max(self.worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (b, t, len(live), float((err / bound).max()))
            if len(live) == 1:
                assert np.array_equal(got[b], live[0][1][t - live[0][0]])       # one live plan: its row, bit for bit
            self.t[b] += 1
        assert pol.local_times.cpu().tolist() == self.t
        return out


# ------------------------------------------------------------------------------------------------------------------ 1. the rule
@pytest.mark.parametrize("m_ens", [0.0, 0.01, 1.0])
@pytest.mark.parametrize("s", [1, 3, 10])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_emitted_actions_match_the_restated_rule(dtype, s, m_ens):
    cfg, m, den = build("noise", dtype)
    assert cfg.action_seq_len == W
    n, steps = 5, 3 * W + 2
    rng = np.random.default_rng(7)
    resets, active = _events(n, steps, rng)
    g = torch.Generator().manual_seed(3)
    obs_t = [torch.randn(n, 2, cfg.obs_dim, generator=g).cuda() for _ in range(steps)]
    goal = torch.randn(n, cfg.goal_dim, generator=g).cuda()
    seeds = list(range(500, 500 + n))
    pol = policy(den, cfg, n, multistep=s, temporal_ensemble=m_ens)
    assert pol.ensemble_depth == -(-W // s) and pol.plan_ring.shape == (n, pol.ensemble_depth, W, cfg.action_dim)
    assert torch.equal(pol.ensemble_weight_table.cpu(), torch.from_numpy(rollout.ensemble_weights(m_ens, pol.ensemble_depth)))
    pol.reset(seeds=seeds)
    now = {}
    ref = Restated(pol, den, n, s, m_ens, lambda rows: now["img"][rows].contiguous())
    replans = 0
    for t in range(steps):
        if t in resets:
            new = [int(rng.integers(0, 2 ** 32)) for _ in resets[t]]
            pol.reset(envs=resets[t], seeds=new)
            ref.reset(resets[t])
            for b, sd in zip(resets[t], new):
                seeds[b] = sd
        now["img"] = obs_t[t]
        ref.step({"state_images": obs_t[t]}, goal, active[t], seeds, cfg.action_dim)
        replans += len(pol.replanned)
    births = pol.plan_births.cpu().numpy()
    for b in range(n):                                       # the ring holds exactly the plans a later step can still read, at their slots
        for tp, p in ref.plans[b][-pol.ensemble_depth:]:
            slot = (tp // s) % pol.ensemble_depth
            assert births[b, slot] == tp and np.array_equal(pol.plan_ring[b, slot].double().cpu().numpy(), p)
    assert replans >= (steps // s) * 2
    print(f"ensemble dtype={dtype} s={s} m={m_ens}: worst |a - a_ref| / bound = {ref.worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ 2. bit identities
@pytest.mark.parametrize("m_ens", [0.0, 0.01, 1.0])
def test_stride_equal_to_window_is_the_policy_without_the_option(m_ens):
    cfg, m, den = build("noise", "bf16")
    n, steps = 5, 3 * W
    rng = np.random.default_rng(11)
    resets, active = _events(n, steps, rng)
    g = torch.Generator().manual_seed(5)
    obs_t = [torch.randn(n, 2, cfg.obs_dim, generator=g).cuda() for _ in range(steps)]
    goal = torch.randn(n, cfg.goal_dim, generator=g).cuda()
    pols = [policy(den, cfg, n, seed=40, multistep=W), policy(den, cfg, n, seed=40, multistep=W, temporal_ensemble=m_ens)]
    assert pols[1].ensemble_depth == 1
    for t in range(steps):
        outs = []
        for pol in pols:
            if t in resets:
                pol.reset(envs=resets[t], seeds=[1000 * t + b for b in resets[t]])
            outs.append(pol.step({"state_images": obs_t[t]}, goal, active=active[t]))
        assert pols[0].replanned == pols[1].replanned
        assert torch.equal(outs[0], outs[1]), t
        assert torch.equal(pols[0].plans, pols[1].plans) and torch.equal(pols[0].draws, pols[1].draws)


@pytest.mark.parametrize("s,m_ens", [(5, 0.01), (3, 1.0), (3, 0.0)])
def test_environment_alone_emits_the_same_stream(s, m_ens):
    """Environment 0 of a batch of 4 against the same environment run alone (num_envs = 1), torch.equal.  The chain's bits depend on the bucket
    batch (tests/test_gpu_vector_env.py::test_staggered_episodes_equal_solo_agents holds a batch against solo agents to a tolerance for that
    reason), so the schedule lets environment 0 pause on the steps at which it would share a chunk: its chunks run at bucket 1 in both runs,
    while the others replan (in buckets of 1 to 3), reset and pause on the steps around and between them, and emit on the same steps as it."""
    cfg, m, den = build("noise", "bf16")
    n, steps = 4, 4 * W
    rng = np.random.default_rng(13)
    g = torch.Generator().manual_seed(6)
    obs_t = [torch.randn(n, 2, cfg.obs_dim, generator=g).cuda() for _ in range(steps)]
    goal = torch.randn(n, cfg.goal_dim, generator=g).cuda()
    others_active = rng.random((steps, n)) > 0.25
    resets = {t: [int(rng.integers(1, n))] for t in (4, 11, 17, 23, 31)}
    resets[14] = [0, 2]                                       # the environment under test resets once as well, with another one
    batch = policy(den, cfg, n, seed=70, multistep=s, temporal_ensemble=m_ens)
    solo = policy(den, cfg, 1, seed=70, multistep=s, temporal_ensemble=m_ens)
    shared_steps = mates = own_replans = 0
    for t in range(steps):
        if t in resets:
            batch.reset(envs=resets[t], seeds=[90 * t + b for b in resets[t]])
            if 0 in resets[t]:
                solo.reset(envs=[0], seeds=[90 * t])
        act = others_active[t].copy()
        others_replan = bool((act[1:] & (batch._counter[1:] == 0)).any())
        act[0] = not (batch._counter[0] == 0 and others_replan)
        out = batch.step({"state_images": obs_t[t]}, goal, active=act)
        mates = max(mates, len(batch.replanned))
        if not act[0]:
            assert not out[0].any()
            continue
        assert batch.replanned in ([0], []) or 0 not in batch.replanned
        own_replans += 0 in batch.replanned
        shared_steps += bool(act[1:].any())
        alone = solo.step({"state_images": obs_t[t][:1]}, goal[:1])
        assert torch.equal(out[0], alone[0]), t
    assert torch.equal(batch.local_times[:1], solo.local_times) and torch.equal(batch.plan_births[0], solo.plan_births[0])
    assert torch.equal(batch.plan_ring[0], solo.plan_ring[0])
    assert own_replans >= 5 and shared_steps >= 10 and mates >= 2


# ------------------------------------------------------------------------------------------------------------------ 3. reset
def test_reset_drops_every_earlier_plan():
    cfg, m, den = build("noise", "bf16")
    n, s, b = 3, 3, 1
    g = torch.Generator().manual_seed(8)
    img = torch.randn(n, 2, cfg.obs_dim, generator=g).cuda()
    goal = torch.randn(n, cfg.goal_dim, generator=g).cuda()
    wild = goal.clone()
    wild[b] *= 1000.0                                        # before the reset environment b plans for a wildly different goal
    only_b = np.arange(n) == b
    pol = policy(den, cfg, n, multistep=s, temporal_ensemble=0.0)
    before = [pol.step({"state_images": img}, wild)[b].clone() for _ in range(W - 3)]
    pol.reset(envs=[b], seeds=[4242])
    after = [pol.step({"state_images": img}, goal, active=only_b).clone() for _ in range(2 * W)]
    assert pol.plan_births[b].cpu().tolist() == [12, 15, 18, 9]          # born at 9 .. 18 since the reset, slot (t_p // 3) % 4
    fresh = policy(den, cfg, n, multistep=s, temporal_ensemble=0.0)
    fresh.reset(envs=[b], seeds=[4242])
    clean = [fresh.step({"state_images": img}, goal, active=only_b).clone() for _ in range(2 * W)]
    for t in range(2 * W):
        assert torch.equal(after[t][b], clean[t][b]), t      # no row from before the reset contributes, at any later step
        assert not after[t][~torch.from_numpy(only_b).cuda()].any()
    again = policy(den, cfg, n, multistep=s, temporal_ensemble=0.0)
    again.reset(envs=[b], seeds=[4242])
    a0 = again.step({"state_images": img}, goal, active=only_b)
    assert torch.equal(after[0][b], again.plans[b, 0]) and torch.equal(a0[b], again.plans[b, 0])       # row 0 of the new plan alone
    # the check can see a leak: the wild goal's plans are far from the clean ones
    far = max(float((x - clean[0][b]).abs().max()) for x in before)
    assert far > 1e-3 * float(clean[0][b].abs().max())


# ------------------------------------------------------------------------------------------------------------------ 4. pauses
@pytest.mark.parametrize("s", [1, 3])
def test_pause_does_not_advance_local_time(s):
    cfg, m, den = build("noise", "bf16")
    n, steps, cut = 3, 2 * W + 4, W + 2
    g = torch.Generator().manual_seed(9)
    obs_t = [torch.randn(n, 2, cfg.obs_dim, generator=g).cuda() for _ in range(steps)]
    goal = torch.randn(n, cfg.goal_dim, generator=g).cuda()
    straight = policy(den, cfg, n, seed=5, multistep=s, temporal_ensemble=0.01)
    paused = policy(den, cfg, n, seed=5, multistep=s, temporal_ensemble=0.01)
    none = np.zeros(n, dtype=bool)
    for t in range(steps):
        if t == cut:
            for _ in range(W + 1):                           # a pause longer than a plan lives
                assert not paused.step({"state_images": obs_t[t]}, goal, active=none).any() and paused.replanned == []
            assert torch.equal(paused.local_times, straight.local_times)
        a, b = straight.step({"state_images": obs_t[t]}, goal), paused.step({"state_images": obs_t[t]}, goal)
        assert torch.equal(a, b), t
        assert straight.replanned == paused.replanned
    assert torch.equal(paused.plan_ring, straight.plan_ring) and torch.equal(paused.plan_births, straight.plan_births)


# ------------------------------------------------------------------------------------------------------------------ 5. structure
def test_launch_budget_and_entry_points(monkeypatch):
    cfg, m, den = build("noise", "bf16")
    n, s = 8, 3
    g = torch.Generator().manual_seed(4)
    img, goal = torch.randn(n, 2, cfg.obs_dim, generator=g).cuda(), torch.randn(n, cfg.goal_dim, generator=g).cuda()
    # (the policy under the sync check is warmed up last: a policy's first chunk re-resolves the model's routing cache, after which the chunks
    # of another policy over the same model rebuild their schedule state once, reading the schedule on the host)
    plain = policy(den, cfg, n, multistep=s)
    plain.warmup({"state_images": img}, goal)
    pol = policy(den, cfg, n, multistep=s, temporal_ensemble=0.01)
    pol.warmup({"state_images": img}, goal)
    assert pol._hooks.store is not plain._hooks.store and len(pol._hooks.store) == len(plain._hooks.store) == len(rollout._buckets(n))
    cnt = dict(capture=0, replay=0, stage=0, mode_env_gather_noise=0, mode_env_commit_emit=0, mode_env_commit_emit_ens=0)
    cap, rep = torch.cuda.CUDAGraph.capture_begin, torch.cuda.CUDAGraph.replay

    def counted_capture(self, *a, **k):
        cnt["capture"] += 1
        return cap(self, *a, **k)

    def counted_replay(self):
        cnt["replay"] += 1
        return rep(self)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "capture_begin", counted_capture)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", counted_replay)
    lib = pol._lib
    for name in ("mode_env_gather_noise", "mode_env_commit_emit", "mode_env_commit_emit_ens"):
        def counted(*a, _f=getattr(lib, name), _n=name):
            cnt[_n] += 1
            return _f(*a)
        monkeypatch.setattr(lib, name, counted)
    for p in (pol, plain):
        def counted_stage(*a, _f=p._stage):
            cnt["stage"] += 1
            return _f(*a)
        monkeypatch.setattr(p, "_stage", counted_stage)

    def one_step(p, act):
        before = dict(cnt)
        p.step({"state_images": img}, goal, active=act)
        return {k: cnt[k] - before[k] for k in cnt}
    for t in range(10):                                      # staggered joins: replanning steps of 1..n rows, and steps without a replan
        pol.step({"state_images": img}, goal, active=np.arange(n) <= t)
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        seen = {True: 0, False: 0}
        for t in range(120):
            act = np.arange(n) != t % n
            if t % 7 == 3:
                act[:] = pol._counter != 0                   # a step on which nobody replans
            d = one_step(pol, act)
            replan = bool(pol.replanned)
            seen[replan] += 1
            if replan:                                       # one H2D copy of the control block, one gather launch, one replay (the commit is in it)
                assert d == dict(capture=0, replay=1, stage=1, mode_env_gather_noise=1, mode_env_commit_emit=0, mode_env_commit_emit_ens=0), (t, d)
            else:                                            # one launch: the ensembled commit + emit
                assert d == dict(capture=0, replay=0, stage=0, mode_env_gather_noise=0, mode_env_commit_emit=0, mode_env_commit_emit_ens=1), (t, d)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert seen[True] > 20 and seen[False] > 10 and cnt["capture"] == 0
    assert torch.cuda.memory_allocated() == mem
    # without the option the policy launches the kernel it always did, never the new entry point
    for t in range(12):
        d = one_step(plain, np.arange(n) != t % n)
        assert d["mode_env_commit_emit_ens"] == 0 and d["mode_env_commit_emit"] == (0 if plain.replanned else 1), (t, d)
        assert d["replay"] == bool(plain.replanned) and d["capture"] == 0


def test_ring_that_cannot_be_allocated_is_a_value_error(monkeypatch):
    cfg, m, den = build("noise", "bf16")
    real = torch.zeros

    def zeros(*shape, **kw):
        if len(shape) == 4:                                  # the ring [num_envs, K, W, A]
            raise torch.cuda.OutOfMemoryError("HIP out of memory (simulated)")
        return real(*shape, **kw)
    monkeypatch.setattr(rollout.torch, "zeros", zeros)
    with pytest.raises(ValueError, match="cannot allocate the plan ring"):
        policy(den, cfg, 4, multistep=1, temporal_ensemble=0.0)
    policy(den, cfg, 4, multistep=1)                         # without the option there is no ring to allocate


# ------------------------------------------------------------------------------------------------------------------ 6. raw frames
def test_raw_frames_compose_with_ensembling():
    import test_gpu_vector_env_frames as F
    cfg, m, den = build("noise", "bf16")
    encs = F.encoders(cfg)
    n, s, m_ens, steps = 2, 3, 0.01, W + 4                     # buckets 1 and 2
    pol = F.policy(den, cfg, encs, n, multistep=s, temporal_ensemble=m_ens)
    obs_t = [F.frames(cfg, n, 30 + t)[0] for t in range(steps)]
    goal = F.frames(cfg, n, 29)[1]
    seeds = [61, 62]
    pol.reset(seeds=seeds)
    now = {}
    ref = Restated(pol, den, n, s, m_ens, lambda rows: F.tokens(encs, F.rows_of(now["obs"], rows), goal[rows].contiguous()))
    sizes = set()
    for t in range(steps):
        act = np.array([True, t not in (1, 6)])               # environment 1 pauses twice: the two drift apart and replan alone
        now["obs"] = obs_t[t]
        ref.step(obs_t[t], goal, act, seeds, cfg.action_dim)
        if pol.replanned:
            sizes.add(len(pol.replanned))
    assert sizes == {1, 2}
    print(f"ensemble raw frames: worst |a - a_ref| / bound = {ref.worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ 7. memory
def test_ensembled_control_loop_holds_no_memory():
    cfg, m, den = build("noise", "bf16")
    n = 8
    pol = policy(den, cfg, n, multistep=3, temporal_ensemble=0.01)
    g = torch.Generator().manual_seed(12)
    img, goal = torch.randn(n, 2, cfg.obs_dim, generator=g).cuda(), torch.randn(n, cfg.goal_dim, generator=g).cuda()
    pol.warmup({"state_images": img}, goal)
    out = None
    for t in range(20):
        out = pol.step({"state_images": img}, goal, active=np.arange(n) <= t)
    torch.cuda.synchronize()
    gc.collect()
    was = gc.isenabled()
    gc.disable()                                             # only reference counts may free memory from here on
    try:
        base = torch.cuda.memory_allocated()
        seen = []
        for t in range(300):
            if t % 41 == 40:
                pol.reset(envs=[t % n])
            out = pol.step({"state_images": img}, goal, active=np.arange(n) != t % n)
            if t % 50 == 49:
                torch.cuda.synchronize()
                seen.append(torch.cuda.memory_allocated())
    finally:
        if was:
            gc.enable()
    assert out is not None and seen and all(v == base for v in seen), (base, seen)
