"""rollout.VectorEnvPolicy(warm_start=k) on the MI355X (c1e4 weights, oracle.weights): the warm gather kernel against the fp64 restatement of
tests/warm_refs.py, warm replans against the fused sampler on the gathered batch and the sub-schedule (bit for bit), steps with cold and warm
replanners against solo agents, the capture / replay / sync budget with cold, warm and mixed replans alternating at the same buckets, and the
default path against a policy built without the keyword."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd import gc_sampling, rollout, samplers  # noqa: E402
from oracle.weights import get_config, make_state_dict  # noqa: E402

from tolerances import BF16_OUT  # noqa: E402
from warm_refs import warm_latents  # noqa: E402

SAMPLERS = {"ddim": gc_sampling.sample_ddim, "heun": samplers.sample_heun, "dpmpp_2m": samplers.sample_dpmpp_2m}
SIGMA_MAX = 80.0


def build(dtype="bf16"):
    cfg = get_config("c1e4")
    m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cuda", goal_conditioned=True, action_dim=cfg.action_dim,
                  embed_dim=cfg.embed_dim, embed_pdrob=0, attn_pdrop=0.3, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1,
                  obs_seq_len=1, action_seq_len=cfg.action_seq_len, num_experts=cfg.num_experts, top_k=cfg.top_k, compute_dtype=dtype)
    m.load_state_dict(make_state_dict(cfg, 210))
    m = m.to("cuda").eval()
    return dataclasses.replace(cfg), m, M.GCDenoiser(m, 0.5).eval()


def policy(den, cfg, n, **kw):
    return rollout.VectorEnvPolicy(den, n, act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, sigma_max=SIGMA_MAX, **kw)


def obs(cfg, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 2, cfg.obs_dim, generator=g).cuda(), torch.randn(n, cfg.goal_dim, generator=g).cuda()


def count_graphs(monkeypatch):
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
    return cnt


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
NUM_ENVS = 5
SEEDS, DRAWS = [0, 7, 2 ** 32 - 1, 123456789, 2 ** 20], [0, 3, 2 ** 20, 2 ** 32 - 1, 9]
SENTINEL, GUARD = -12345.0, 64


def _gather_warm(rows, plan, shift, sigma):
    """mode_env_gather_warm on a sentinel-filled x0 with GUARD words in front of and behind it.  Returns (x0 [len(rows), W, A], guards)."""
    n, W, A = plan.shape
    r = torch.tensor(rows, dtype=torch.int32, device="cuda")
    s, d = rollout._u32_as_i32(SEEDS).cuda(), rollout._u32_as_i32(DRAWS).cuda()
    buf = torch.full((2 * GUARD + len(rows) * W * A,), SENTINEL, device="cuda")
    x0 = buf[GUARD:GUARD + len(rows) * W * A]
    L.check(L.load().mode_env_gather_warm(r.data_ptr(), len(rows), n, s.data_ptr(), d.data_ptr(), None, 0, None, 0, None, None, x0.data_ptr(),
                                          plan.data_ptr(), W, A, shift, sigma, torch.cuda.current_stream().cuda_stream), "env_gather_warm")
    torch.cuda.synchronize()
    return x0.view(len(rows), W, A), torch.cat([buf[:GUARD], buf[GUARD + len(rows) * W * A:]])


def _plans(W, A):
    """Entries of every magnitude from 1e-3 up to 1e3, both signs."""
    rng = np.random.default_rng(W * 1000 + A)
    p = rng.uniform(-1.0, 1.0, (NUM_ENVS, W, A)) * 10.0 ** rng.uniform(-3.0, 3.0, (NUM_ENVS, W, A))
    p[0, 0, 0], p[1, W - 1, A - 1] = 1e3, -1e3
    return torch.from_numpy(p.astype(np.float32)).cuda()


@pytest.mark.parametrize("sigma", [0.0, 0.37, 80.0])
@pytest.mark.parametrize("W,A,shift", [(10, 7, 1), (10, 7, 9), (37, 7, 5), (64, 64, 63)])
def test_warm_gather_matches_restatement(W, A, shift, sigma):
    """|x - ref| <= sigma_start * 2e-6 * max(1, |z|) + 2^-23 |ref| per element: the project's bound on the noise element
    (test_env_noise_matches_restatement_and_is_padding_invariant) and two fp32 roundings of the sum."""
    plan = _plans(W, A)
    rows = [3, 0, 2, -1, NUM_ENVS, 4, 1, 1, 1]                                        # two entries out of range; padding by repetition
    x0, guards = _gather_warm(rows, plan, shift, sigma)
    assert (guards == SENTINEL).all()
    host, got = plan.cpu().numpy(), x0.cpu().double().numpy()
    idx = np.minimum(np.arange(W) + shift, W - 1)
    worst = 0.0
    for j, r in enumerate(rows):
        if not 0 <= r < NUM_ENVS:
            assert (x0[j] == SENTINEL).all(), j                                       # untouched
            continue
        ref, z = warm_latents(host[r], SEEDS[r], DRAWS[r], shift, sigma)
        bound = float(np.float32(sigma)) * 2e-6 * np.maximum(1.0, np.abs(z)) + 2.0 ** -23 * np.abs(ref)
        err = np.abs(got[j] - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (j, r, float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))
        if sigma == 0.0:
            assert torch.equal(x0[j], plan[r][idx]), (j, r)                           # the shifted plan, bit for bit
    print(f"warm gather W={W} A={A} shift={shift} sigma={sigma}: worst error / bound = {worst:.3f}")
    solo, g2 = _gather_warm([1], plan, shift, sigma)                                  # a padded call and a solo call: identical rows
    assert (g2 == SENTINEL).all()
    assert all(torch.equal(solo[0], x0[j]) for j in (6, 7, 8))


def test_env_warm_latents_is_the_kernel_on_explicit_rows():
    W, A, shift = 10, 7, 4
    plan = _plans(W, A)
    x0, _ = _gather_warm(list(range(NUM_ENVS)), plan, shift, 0.37)
    assert torch.equal(rollout.env_warm_latents(plan, SEEDS, DRAWS, shift, 0.37), x0)
    pick = [4, 1, 1]
    assert torch.equal(rollout.env_warm_latents(plan[pick], [SEEDS[i] for i in pick], [DRAWS[i] for i in pick], shift, 0.37), x0[pick])
    # the same stream element as the cold replan's latent
    cold = rollout.env_noise(SEEDS, DRAWS, W, A, 1.0, "cuda")
    zero = torch.zeros_like(plan)
    assert torch.equal(rollout.env_warm_latents(zero, SEEDS, DRAWS, shift, 1.0), cold)
    with pytest.raises(RuntimeError, match="env_gather_warm"):
        rollout.env_warm_latents(plan, SEEDS, DRAWS, W, 0.37)                         # shift >= W
    with pytest.raises(ValueError, match="one seed"):
        rollout.env_warm_latents(plan, SEEDS[:2], DRAWS, shift, 0.37)


# ------------------------------------------------------------------------------------------------------------------ 2. exact plans
def _drain(pol, img, goal, envs):
    """Step the listed environments, alone, until each is due to replan (counter 0): steps without a replan."""
    while pol._counter[envs].any():
        act = np.zeros(pol.num_envs, dtype=bool)
        act[[b for b in envs if pol._counter[b]]] = True
        pol.step({"state_images": img}, goal, active=act)
        assert pol.replanned == [] and pol.replanned_warm == []


@pytest.mark.parametrize("sampler,w", [("ddim", None), ("heun", None), ("dpmpp_2m", None), ("ddim", 2.5)])
def test_warm_replans_equal_fused_sampler_on_gathered_batch_and_sub_schedule(sampler, w):
    cfg, m, den = build("bf16")
    den.guidance_scale = w
    n, s, k = 8, 4, 5
    pol = policy(den, cfg, n, sampler_type=sampler, multistep=s, warm_start=k)
    img, goal = obs(cfg, n, 1)
    seeds = [11, 12, 13, 14, 15, 16, 17, 18]
    pol.reset(seeds=seeds)
    pol.step({"state_images": img}, goal)                                             # the first replan of an episode is cold
    assert pol.replanned == list(range(n)) and pol.replanned_warm == []
    sched = pol._schedule(img.device)
    sub = sched[k:].clone()
    assert sched.numel() == 11 and sub.numel() == 6
    for step, envs in enumerate(([1, 4, 6], [0, 2, 3, 5, 7], [4])):                  # m = 3 (bucket 4), 5 (bucket 8), 1
        _drain(pol, img, goal, envs)
        act = np.zeros(n, dtype=bool)
        act[envs] = True
        draws, prev = pol.draws.cpu().tolist(), pol.plans.clone()
        out = pol.step({"state_images": img}, goal, active=act)
        assert pol.replanned == envs and pol.replanned_warm == envs
        mb = next(b for b in (1, 2, 4, 8) if b >= len(envs))
        rows = envs + [envs[-1]] * (mb - len(envs))
        x0 = rollout.env_warm_latents(prev[rows], [seeds[r] for r in rows], [draws[r] for r in rows], s, sched[k])
        ref = SAMPLERS[sampler](den, {"state_images": img[rows].contiguous()}, x0, goal[rows].contiguous(), sub, disable=True)
        assert torch.equal(pol.plans[envs], ref[:len(envs)]), (sampler, step)
        assert torch.equal(out[envs], ref[:len(envs), 0])
        assert not out[~torch.from_numpy(act).cuda()].any()                           # inactive rows are zero
        assert pol.draws.cpu().tolist() == [d + (i in envs) for i, d in enumerate(draws)]
        others = [b for b in range(n) if b not in envs]
        assert torch.equal(pol.plans[others], prev[others])
    # a reset makes an environment cold again: the full schedule from sigma_max * z
    pol.reset(envs=[4])
    _drain(pol, img, goal, [2])
    act = np.zeros(n, dtype=bool)
    act[[2, 4]] = True
    draws, prev = pol.draws.cpu().tolist(), pol.plans.clone()
    pol.step({"state_images": img}, goal, active=act)
    assert pol.replanned == [2, 4] and pol.replanned_warm == [2]
    x0 = rollout.env_noise([seeds[4]], [draws[4]], cfg.action_seq_len, cfg.action_dim, SIGMA_MAX, "cuda")
    ref = SAMPLERS[sampler](den, {"state_images": img[[4]].contiguous()}, x0, goal[[4]].contiguous(), sched, disable=True)
    assert torch.equal(pol.plans[4], ref[0])
    x0 = rollout.env_warm_latents(prev[[2]], [seeds[2]], [draws[2]], s, sched[k])
    ref = SAMPLERS[sampler](den, {"state_images": img[[2]].contiguous()}, x0, goal[[2]].contiguous(), sub, disable=True)
    assert torch.equal(pol.plans[2], ref[0])


# ------------------------------------------------------------------------------------------------------------------ 3. cold and warm in one step
@pytest.mark.parametrize("ens", [None, 0.5])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_cold_and_warm_replanners_in_one_step_equal_solo_agents(dtype, ens):
    """Five environments replan together every 4 steps; two of them are reset in the step of the second replan, so that step runs a cold chunk
    (bucket 2) and a warm chunk (bucket 4).  Every solo agent decides cold or warm by itself.  Comparison and tolerances:
    tests/test_gpu_vector_env.py::test_staggered_episodes_equal_solo_agents."""
    cfg, m, den = build(dtype)
    n, steps, s, k = 5, 12, 4, 5
    g = torch.Generator().manual_seed(9)
    obs_t = [torch.randn(n, 2, cfg.obs_dim, generator=g).cuda() for _ in range(steps)]
    goal = torch.randn(n, cfg.goal_dim, generator=g).cuda()
    hit, new_seeds = [1, 3], {1: 4001, 3: 4003}
    kinds = []

    def run(pol, envs):
        outs, plans = [], []
        for t in range(steps):
            mine = [b for b in hit if b in envs]
            if t == 4 and mine:
                pol.reset(envs=[envs.index(b) for b in mine], seeds=[new_seeds[b] for b in mine])
            outs.append(pol.step({"state_images": obs_t[t][envs]}, goal[envs]).clone())
            plans.append(pol.plans.clone())
            kinds.append((len(envs), t, [envs[i] for i in pol.replanned], [envs[i] for i in pol.replanned_warm]))
        return torch.stack(outs, 1), torch.stack(plans, 1)                            # [len(envs), steps, ...]

    batched, bplans = run(policy(den, cfg, n, seed=100, multistep=s, warm_start=k, temporal_ensemble=ens), list(range(n)))
    got_kinds = {t: (r, w) for size, t, r, w in kinds if size == n and r}
    assert got_kinds == {0: (list(range(n)), []), 4: (list(range(n)), [0, 2, 4]), 8: (list(range(n)), list(range(n)))}
    for b in range(n):
        del kinds[:]
        solo, splans = run(policy(den, cfg, 1, seed=100 + b, multistep=s, warm_start=k, temporal_ensemble=ens), [b])
        assert [(t, w) for _, t, r, w in kinds if r] == [(0, []), (4, [] if b in hit else [b]), (8, [b])]
        for name, got, want in (("actions", batched[b], solo[0]), ("plans", bplans[b], splans[0])):
            if dtype == "fp32":
                err = float((got - want).abs().max())
                print(f"{dtype} ens={ens} env {b} {name}: max abs err {err:.3e}, bound {1e-5 * float(want.abs().max()):.3e}")
                assert err <= 1e-5 * float(want.abs().max()), (name, b, err)
            else:
                err = float((got - want).double().norm() / want.double().norm())
                print(f"{dtype} ens={ens} env {b} {name}: rel err {err:.3e}, bound {BF16_OUT:.3e}")
                assert err <= BF16_OUT, (name, b, err)


# ------------------------------------------------------------------------------------------------------------------ 4. budget
def test_no_capture_one_replay_per_kind_no_sync_flat_memory(monkeypatch):
    cfg, m, den = build("bf16")
    n, s, k = 4, 2, 5
    pol = policy(den, cfg, n, multistep=s, warm_start=k)
    img, goal = obs(cfg, n, 4)
    pol.warmup({"state_images": img}, goal)
    assert len(pol._hooks.store) == len(pol._hooks_warm.store) == len(rollout._buckets(n)) and pol._hooks.store is not pol._hooks_warm.store
    assert not pol._warm.any() and not pol.draws.any()                                # warming up changes no state
    cnt = count_graphs(monkeypatch)
    # the replanning steps cycle through: all cold (bucket 4), all warm (4), cold 2 + warm 2, cold 1 + warm 3 (4), cold 3 (4) + warm 1
    cycle = ([0, 1, 2, 3], [], [0, 1], [0], [0, 1, 2])

    def loop(steps):
        seen = {"cold": 0, "warm": 0, "mixed": 0, "none": 0}
        for t in range(steps):
            resets = cycle[(t // s) % len(cycle)] if t % s == 0 else []
            if resets:
                pol.reset(envs=resets)
            before = cnt["replay"]
            pol.step({"state_images": img}, goal)
            if t % s:
                assert pol.replanned == [] and cnt["replay"] == before, t
                seen["none"] += 1
                continue
            warm = [b for b in range(n) if b not in resets] if t else []              # (the very first replan: everybody is cold)
            assert pol.replanned == list(range(n)) and pol.replanned_warm == warm, t
            mixed = 0 < len(warm) < n
            assert cnt["replay"] == before + (2 if mixed else 1), (t, warm)
            seen["mixed" if mixed else "warm" if warm else "cold"] += 1
        return seen
    loop(2 * s * len(cycle))
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        seen = loop(200)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert seen == {"cold": 20, "warm": 20, "mixed": 60, "none": 100} and cnt["capture"] == 0
    assert torch.cuda.memory_allocated() == mem


def test_alternating_cold_and_warm_replans_never_recapture_the_encoder_graph(monkeypatch):
    """Raw frames (two FiLM-ResNet-18 encoders, 64 x 64 and 48 x 48, T = 1: the smallest geometry of tests/test_gpu_vector_env_frames.py): a chunk
    is an encoder replay and a chain replay, and cold and warm chunks at one bucket keep their own encoder graphs."""
    from oracle import resnet_oracle as R
    cfg, m, den = build("bf16")
    encs = []
    for seed in (1, 2):
        e = M.FiLMResNet18Policy(cfg.goal_dim).cuda().eval()
        e.load_state_dict({k: v.cuda() for k, v in R.fill_encoder_state_dict(e.state_dict(), seed).items()})
        encs.append(e)
    n, s, k = 2, 2, 5
    pol = policy(den, cfg, n, multistep=s, warm_start=k, static_resnet=encs[0], gripper_resnet=encs[1])
    g = torch.Generator().manual_seed(5)
    frames = {"rgb_obs": {"rgb_static": torch.randn(n, 1, 3, 64, 64, generator=g).cuda(), "rgb_gripper": torch.randn(n, 1, 3, 48, 48, generator=g).cuda()}}
    goal = torch.randn(n, cfg.goal_dim, generator=g).cuda()
    pol.warmup(frames, goal)
    assert sorted(pol._hooks.enc) == sorted(pol._hooks_warm.enc) == [1, 2] and pol._hooks.enc is pol._enc_store
    cnt = count_graphs(monkeypatch)
    cycle = ([0, 1], [], [0, 1], [], [1], [])                                         # bucket 2: cold, warm, cold, warm; bucket 1: cold + warm; warm
    torch.cuda.set_sync_debug_mode("error")
    try:
        for r, resets in enumerate(cycle * 2):
            if resets:
                pol.reset(envs=resets)
            before = cnt["replay"]
            pol.step(frames, goal)
            warm = [b for b in range(n) if b not in resets] if r else []
            assert pol.replanned == [0, 1] and pol.replanned_warm == warm, r
            assert cnt["replay"] == before + (4 if 0 < len(warm) < n else 2), r
            pol.step(frames, goal)
            assert pol.replanned == [] and cnt["replay"] == before + (4 if 0 < len(warm) < n else 2), r
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert cnt["capture"] == 0


# ------------------------------------------------------------------------------------------------------------------ 5. defaults
def test_warm_start_none_is_the_policy_without_the_keyword():
    cfg, m, den = build("bf16")
    n, steps, s = 5, 16, 4
    rng = np.random.default_rng(5)
    resets = {t: sorted(rng.choice(n, size=int(rng.integers(1, 3)), replace=False).tolist()) for t in (2, 5, 9, 12)}
    active = rng.random((steps, n)) > 0.2
    g = torch.Generator().manual_seed(9)
    obs_t = [torch.randn(n, 2, cfg.obs_dim, generator=g).cuda() for _ in range(steps)]
    goal = torch.randn(n, cfg.goal_dim, generator=g).cuda()
    plain, none = policy(den, cfg, n, seed=100, multistep=s), policy(den, cfg, n, seed=100, multistep=s, warm_start=None)
    assert none.warm_start is None
    replans = 0
    for t in range(steps):
        for p in (plain, none):
            if t in resets:
                p.reset(envs=resets[t], seeds=[1000 * t + b for b in resets[t]])
        a, b = plain.step({"state_images": obs_t[t]}, goal, active=active[t]), none.step({"state_images": obs_t[t]}, goal, active=active[t])
        assert torch.equal(a, b) and torch.equal(plain.plans, none.plans) and torch.equal(plain.draws, none.draws), t
        assert plain.replanned == none.replanned and none.replanned_warm == [] and plain.replanned_warm == []
        replans += bool(none.replanned)
    assert replans >= 6 and len(none._hooks_warm.store) == 0
