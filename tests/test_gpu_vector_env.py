"""rollout.VectorEnvPolicy on the MI355X (c1e4 weights, oracle.weights): the per-environment noise stream against a numpy restatement, replanned
plans against the fused sampler on the same gathered batch (bit for bit), staggered episodes against solo (num_envs = 1) agents in all three routing
modes, lockstep replanning, one capture per bucket and one replay per replanning step without host syncs, and the expert-usage counters."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import gc_sampling, rollout, samplers  # noqa: E402
from oracle import mode_oracle as O  # noqa: E402
from oracle.weights import get_config, make_state_dict  # noqa: E402

from tolerances import BF16_OUT, BF16_TOKROUTE_OUT  # noqa: E402

MODES = {"noise": (210, {}), "goal": (220, dict(use_goal_in_routing=True)), "token": (230, dict(cond_router=False))}
SAMPLERS = {"ddim": gc_sampling.sample_ddim, "heun": samplers.sample_heun, "dpmpp_2m": samplers.sample_dpmpp_2m}
SIGMA_MAX = 80.0


def build(mode="noise", dtype="bf16"):
    seed, over = MODES[mode]
    cfg = get_config("c1e4")
    m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cuda", goal_conditioned=True, action_dim=cfg.action_dim,
                  embed_dim=cfg.embed_dim, embed_pdrob=0, attn_pdrop=0.3, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1,
                  obs_seq_len=1, action_seq_len=cfg.action_seq_len, num_experts=cfg.num_experts, top_k=cfg.top_k, compute_dtype=dtype, **over)
    m.load_state_dict(make_state_dict(cfg, seed))
    m = m.to("cuda").eval()
    return dataclasses.replace(cfg, **over), m, M.GCDenoiser(m, 0.5).eval()


def policy(den, cfg, n, **kw):
    return rollout.VectorEnvPolicy(den, n, act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, sigma_max=SIGMA_MAX, **kw)


def obs(cfg, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 2, cfg.obs_dim, generator=g).cuda(), torch.randn(n, cfg.goal_dim, generator=g).cuda()


def np_noise(seed, draw, n_el):
    """include/mode_hip.h's stream, restated: the hash in numpy uint32 (oracle's lowbias32), Box-Muller in float64."""
    k = np.uint32(O.stream_seed(seed, draw))                        # mode_stream_seed(seed, draw)
    e = np.arange(n_el, dtype=np.uint32)
    h1, h2 = O._lowbias32(k ^ (np.uint32(2) * e)), O._lowbias32(k ^ (np.uint32(2) * e + np.uint32(1)))
    u1 = ((h1 >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (h2 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


# ------------------------------------------------------------------------------------------------------------------ 1. noise
def test_env_noise_matches_restatement_and_is_padding_invariant():
    seeds, draws = [0, 1, 7, 2 ** 32 - 1, 123456789], [0, 3, 0, 9, 2 ** 20]
    z = rollout.env_noise(seeds, draws, 10, 7, 1.0, "cuda").cpu().double().numpy()
    for i, (s, d) in enumerate(zip(seeds, draws)):
        ref = np_noise(s, d, 70).reshape(10, 7)
        assert np.all(np.abs(z[i] - ref) <= 2e-6 * np.maximum(1.0, np.abs(ref))), (s, d, np.abs(z[i] - ref).max())
    x = rollout.env_noise(seeds, draws, 10, 7, SIGMA_MAX, "cuda")
    alone = rollout.env_noise([7], [0], 10, 7, SIGMA_MAX, "cuda")
    padded = rollout.env_noise([1, 7, 7, 7], [3, 0, 0, 0], 10, 7, SIGMA_MAX, "cuda")
    assert torch.equal(alone[0], x[2]) and all(torch.equal(alone[0], padded[j]) for j in (1, 2, 3))
    assert torch.equal(x[1], padded[0])


def test_env_noise_moments():
    n = 1_000_000 // 70 + 1
    z = rollout.env_noise(range(n), [5] * n, 10, 7, 1.0, "cuda").double()
    assert z.numel() >= 1_000_000
    assert abs(float(z.mean())) < 5e-3 and abs(float(z.var()) - 1.0) < 5e-3


# ------------------------------------------------------------------------------------------------------------------ 2. exact plans
@pytest.mark.parametrize("sampler", ["ddim", "heun", "dpmpp_2m"])
def test_replanned_rows_equal_fused_sampler_on_gathered_batch(sampler):
    cfg, m, den = build("noise", "bf16")
    n = 8
    pol = policy(den, cfg, n, sampler_type=sampler)
    img, goal = obs(cfg, n, 1)
    seeds = [11, 12, 13, 14, 15, 16, 17, 18]
    pol.reset(seeds=seeds)
    for step, envs in enumerate(([1, 4, 6], [0, 2, 3, 5, 7], [4])):                  # m = 3 (bucket 4), 5 (bucket 8), 1
        act = np.zeros(n, dtype=bool)
        act[envs] = True
        pol.reset(envs=envs)
        draws = pol.draws.cpu().tolist()
        out = pol.step({"state_images": img}, goal, active=act)
        assert pol.replanned == envs
        mb = next(b for b in (1, 2, 4, 8) if b >= len(envs))
        rows = envs + [envs[-1]] * (mb - len(envs))
        x0 = rollout.env_noise([seeds[r] for r in rows], [draws[r] for r in rows], cfg.action_seq_len, cfg.action_dim, SIGMA_MAX, "cuda")
        ref = SAMPLERS[sampler](den, {"state_images": img[rows].contiguous()}, x0, goal[rows].contiguous(), pol._schedule(img.device), disable=True)
        assert torch.equal(pol.plans[envs], ref[:len(envs)]), (sampler, step)
        assert torch.equal(out[envs], ref[:len(envs), 0])
        assert not out[~torch.from_numpy(act).cuda()].any()                           # inactive rows are zero
        assert pol.draws.cpu().tolist() == [d + (i in envs) for i, d in enumerate(draws)]


# ------------------------------------------------------------------------------------------------------------------ 3. staggered = solo
def _schedule_of_events(n, steps, rng):
    resets = {t: sorted(rng.choice(n, size=int(rng.integers(1, 3)), replace=False).tolist()) for t in (2, 5, 9, 12)}
    active = rng.random((steps, n)) > 0.2
    return resets, active


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["noise", "goal", "token"])
def test_staggered_episodes_equal_solo_agents(mode, dtype):
    cfg, m, den = build(mode, dtype)
    n, steps, multistep = 5, 16, 4
    rng = np.random.default_rng(5)
    resets, active = _schedule_of_events(n, steps, rng)
    g = torch.Generator().manual_seed(9)
    obs_t = [torch.randn(n, 2, cfg.obs_dim, generator=g).cuda() for _ in range(steps)]
    goals = {(t, b): torch.randn(1, cfg.goal_dim, generator=g).cuda() for t in [0] + sorted(resets) for b in range(n)}
    seeds = {(t, b): int(rng.integers(0, 2 ** 32)) for t in sorted(resets) for b in range(n)}

    def run(pol, envs):
        cur = {b: goals[(0, b)] for b in envs}
        outs = []
        for t in range(steps):
            hit = [b for b in resets.get(t, []) if b in envs]
            if hit:
                pol.reset(envs=[envs.index(b) for b in hit], seeds=[seeds[(t, b)] for b in hit])
                cur.update({b: goals[(t, b)] for b in hit})
            outs.append(pol.step({"state_images": obs_t[t][envs]}, torch.cat([cur[b] for b in envs]), active=active[t, envs]).clone())
        return torch.stack(outs, 1)                                                   # [len(envs), steps, A]

    batched = run(policy(den, cfg, n, seed=100, multistep=multistep), list(range(n)))
    for b in range(n):
        solo = run(policy(den, cfg, 1, seed=100 + b, multistep=multistep), [b])[0]
        got = batched[b]
        assert not got[~torch.from_numpy(active[:, b]).cuda()].any()                   # inactive steps emit zero rows
        if dtype == "fp32":
            err = float((got - solo).abs().max())
            assert err <= 1e-5 * float(solo.abs().max()), (mode, b, err)
        else:                                                  # bf16 token routing: a bucket's rounding can flip a token's experts (tolerances.py)
            err = float((got - solo).double().norm() / solo.double().norm())
            assert err <= (BF16_TOKROUTE_OUT if mode == "token" else BF16_OUT), (mode, b, err)


# ------------------------------------------------------------------------------------------------------------------ 4. lockstep
def test_lockstep_replans_like_chunked_rollout_policy():
    cfg, m, den = build("noise", "bf16")
    n, multistep = 4, 3
    pol = policy(den, cfg, n, multistep=multistep)
    ref = rollout.ChunkedRolloutPolicy(den, act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, multistep=multistep)
    img, goal = obs(cfg, n, 3)
    calls = []
    orig = ref.denoise_actions
    ref.denoise_actions = lambda *a, **k: calls.append(True) or orig(*a, **k)
    pol.reset()
    for t in range(10):
        before = len(calls)
        ref.step({"state_images": img}, goal)
        out = pol.step({"state_images": img}, goal)
        assert pol.replanned == (list(range(n)) if t % multistep == 0 else []), t
        assert (len(calls) > before) == bool(pol.replanned)
        assert torch.equal(out, pol.plans[:, t % multistep])


# ------------------------------------------------------------------------------------------------------------------ 5. graphs and budget
def test_one_capture_per_bucket_one_replay_per_replan_no_sync(monkeypatch):
    cfg, m, den = build("noise", "bf16")
    n = 8
    pol = policy(den, cfg, n)
    img, goal = obs(cfg, n, 4)
    pol.warmup({"state_images": img}, goal)
    cnt = {"capture": 0, "replay": 0}
    cap, rep = torch.cuda.CUDAGraph.capture_begin, torch.cuda.CUDAGraph.replay

    def counted_capture(self, *a, **k):
        cnt["capture"] += 1
        return cap(self, *a, **k)

    def counted_replay(self):
        cnt["replay"] += 1
        return rep(self)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "capture_begin", counted_capture)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", counted_replay)
    for size in (1, 3, 1, 5, 2, 8):
        envs = list(range(size))
        act = np.zeros(n, dtype=bool)
        act[envs] = True
        pol.reset(envs=envs)
        before = cnt["replay"]
        pol.step({"state_images": img}, goal, active=act)
        assert pol.replanned == envs and cnt["replay"] == before + 1, size
    assert cnt["capture"] == 0
    # steady state: replanning and non-replanning steps, staggered, without a host sync, with flat device memory
    for t in range(10):
        pol.step({"state_images": img}, goal, active=np.arange(n) <= t)
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        replans = 0
        for t in range(200):
            pol.step({"state_images": img}, goal, active=np.arange(n) != t % n)
            replans += bool(pol.replanned)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert replans > 20 and cnt["capture"] == 0
    assert torch.cuda.memory_allocated() == mem


# ------------------------------------------------------------------------------------------------------------------ 6. usage counters
@pytest.mark.parametrize("mode", ["noise", "goal", "token"])
def test_usage_counters_count_real_rows_only(mode):
    cfg, m, den = build(mode, "bf16")
    n = 8
    pol = policy(den, cfg, n)
    img, goal = obs(cfg, n, 6)
    pol.warmup({"state_images": img}, goal)
    m.sync_expert_usage()
    for blk in m.blocks:
        blk.reset_expert_usage()
    envs = [2, 5, 7]
    act = np.zeros(n, dtype=bool)
    act[envs] = True
    pol.step({"state_images": img}, goal, active=act)
    m.sync_expert_usage()
    T, n_evals, E = m.seq_len, 10, m.num_experts
    idx = m._last_topk.long().cpu()
    if mode == "noise":                                        # [L, n, k]: every token of the chunk
        exp = torch.stack([torch.bincount(idx[l].reshape(-1), minlength=E) * 3 * T for l in range(m.num_layers)])
    elif mode == "goal":                                       # [L, n, B, k]: one decision per sample
        exp = torch.stack([torch.bincount(idx[l, :, :3].reshape(-1), minlength=E) * T for l in range(m.num_layers)])
    else:                                                      # [L, n, B*T, k]: one decision per token
        exp = torch.stack([torch.bincount(idx[l, :, :3 * T].reshape(-1), minlength=E) for l in range(m.num_layers)])
    for l, blk in enumerate(m.blocks):
        assert blk.total_tokens_processed == 3 * T * n_evals
        assert torch.equal(blk.inference_expert_usage, exp[l].float()), (mode, l)
        assert int(blk.inference_expert_usage.sum()) == 3 * T * n_evals * m.top_k


# ------------------------------------------------------------------------------------------------------------------ 7. validation
def test_validation_errors():
    cfg, m, den = build("noise", "bf16")
    n = 4
    for bad in ("euler_ancestral", "lms"):
        with pytest.raises(ValueError, match="deterministic fused samplers"):
            policy(den, cfg, n, sampler_type=bad)
    with pytest.raises(ValueError, match="extra_args"):
        policy(den, cfg, n, extra_args={"s_churn": 1.0})
    pol = policy(den, cfg, n)
    img, goal = obs(cfg, n + 1, 7)
    with pytest.raises(ValueError, match="one row per environment"):
        pol.step({"state_images": img}, goal[:n])
    with pytest.raises(ValueError, match="latent_goal"):
        pol.step({"state_images": img[:n]}, goal)
    with pytest.raises(ValueError, match="HOST mask"):
        pol.step({"state_images": img[:n]}, goal[:n], active=torch.ones(n, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="embed raw camera"):
        pol.step({"rgb_obs": {}}, goal[:n])
