"""rollout.VectorEnvPolicy with raw camera frames on the MI355X (c1e4 denoiser, two FiLM-ResNet-18 encoders at 64 x 64, oracle.resnet_oracle):
the frame gather kernel against indexing, replanned plans against the composition "encoders on the gathered rows, then the fused sampler",
isolation of an environment from its bucket mates and from the rows that do not replan, staggered episodes against solo agents, frames against
embeddings, and the replay / capture / sync budget of a control loop."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd import gc_sampling, rollout  # noqa: E402

from test_gpu_vector_env import SIGMA_MAX, _schedule_of_events, build  # noqa: E402
from tolerances import BF16_OUT, BF16_TOKROUTE_OUT  # noqa: E402

HW = 64


def encoders(cfg):
    from oracle import resnet_oracle as R
    out = []
    for seed in (1, 2):
        e = M.FiLMResNet18Policy(cfg.goal_dim).cuda().eval()
        e.load_state_dict({k: v.cuda() for k, v in R.fill_encoder_state_dict(e.state_dict(), seed).items()})
        out.append(e)
    assert out[0].resnet.num_features == cfg.obs_dim
    return out


def policy(den, cfg, encs, n, **kw):
    return rollout.VectorEnvPolicy(den, n, act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, sigma_max=SIGMA_MAX,
                                   static_resnet=encs[0], gripper_resnet=encs[1], **kw)


def frames(cfg, n, seed, hg=HW):
    g = torch.Generator().manual_seed(seed)
    return ({"rgb_obs": {"rgb_static": torch.randn(n, 1, 3, HW, HW, generator=g).cuda(), "rgb_gripper": torch.randn(n, 1, 3, hg, hg, generator=g).cuda()}},
            torch.randn(n, cfg.goal_dim, generator=g).cuda())


def rows_of(obs, rows):
    return {"rgb_obs": {k: v[rows].contiguous() for k, v in obs["rgb_obs"].items()}}


def nan_except(obs, keep):
    """A copy of the frames with NaN in every environment row not in ``keep``."""
    out = {"rgb_obs": {k: v.clone() for k, v in obs["rgb_obs"].items()}}
    drop = [b for b in range(len(obs["rgb_obs"]["rgb_static"])) if b not in keep]
    for v in out["rgb_obs"].values():
        v[drop] = float("nan")
    return out


def tokens(encs, obs, goal):
    """The reference embedding: the eager towers under the policy's default bf16 autocast."""
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        return M.embed_visual_obs(encs[0], encs[1], obs["rgb_obs"]["rgb_static"], obs["rgb_obs"]["rgb_gripper"], goal)["state_images"].float()


def rel(a, b):
    return float((a - b).double().norm() / b.double().norm())


# ------------------------------------------------------------------------------------------------------------------ 1. the gather kernel
def _gather(rows, num_envs, cams):
    """mode_env_gather_frames on (src [num_envs, ...] view, dst [m_b, row] tensor) pairs."""
    r = torch.tensor(rows, dtype=torch.int32, device="cuda")
    d = L.ModeEnvFramesDesc(rows=r.data_ptr(), m_b=len(rows), num_envs=num_envs)
    dt = {torch.float32: L.MODE_F32, torch.bfloat16: L.MODE_BF16}
    for k, (src, dst) in enumerate(cams):
        d.cam[k] = L.ModeEnvFramesCam(src=src.data_ptr(), src_stride=src.stride(0), row_elems=src[0].numel(), dst=dst.data_ptr(),
                                      src_dtype=dt[src.dtype], dst_dtype=dt[dst.dtype])
    L.check(L.load().mode_env_gather_frames(C.byref(d), torch.cuda.current_stream().cuda_stream), "env_gather_frames")
    torch.cuda.synchronize()


@pytest.mark.parametrize("src_dt,dst_dt", [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)])
@pytest.mark.parametrize("shape,pad,offset", [((2, 3, 13, 11), 0, 0), ((1, 3, 64, 64), 0, 0), ((1, 3, 64, 64), 3, 1), ((2, 3, 224, 224), 8, 0)])
def test_gather_frames_equals_indexing(src_dt, dst_dt, shape, pad, offset):
    num_envs = 7
    row = int(np.prod(shape))
    g = torch.Generator().manual_seed(row + pad)
    base = torch.randn(num_envs * (row + pad) + offset, generator=g).to(src_dt).cuda()
    src = base[offset:offset + num_envs * (row + pad)].view(num_envs, row + pad)[:, :row].view(num_envs, *shape)   # pitch row + pad, maybe misaligned
    listed = [5, 2, 0]
    src[[b for b in range(num_envs) if b not in listed]] = float("nan")           # never read
    src[5, 0, 0, 0, :3] = torch.tensor([float("nan"), 1.00390625, -3.0e38])        # NaN and rounding cases inside a listed row
    rows = [5, 2, 2, 9, -1, 0, 5]                                                  # a repeat, two entries out of range, padding by repetition
    dst = torch.full((len(rows), row), 7.0, device="cuda").to(dst_dt)
    other = torch.randn(num_envs, 3, 5, 5, generator=g).cuda()                     # the second camera: another geometry, fp32 -> fp32
    dst2 = torch.zeros(len(rows), 75, device="cuda")
    _gather(rows, num_envs, [(src, dst), (other, dst2)])
    for j, r in enumerate(rows):
        if 0 <= r < num_envs:
            want = src[r].reshape(-1).to(dst_dt)
            bits = torch.int16 if dst_dt == torch.bfloat16 else torch.int32
            fin = torch.isfinite(want)
            assert torch.equal(dst[j][fin].view(bits), want[fin].view(bits)), (j, r)
            assert torch.equal(torch.isnan(dst[j]), torch.isnan(want)) and torch.equal(dst[j][torch.isinf(want)], want[torch.isinf(want)])
            assert torch.equal(dst2[j], other[r].reshape(-1))
        else:
            assert (dst[j] == 7.0).all() and (dst2[j] == 0).all(), j             # untouched


# ------------------------------------------------------------------------------------------------------------------ 2. exact replans
def _chunk_img(pol, mb):
    (ent,) = [e for (gkey, b), e in pol._hooks.store.items() if b == mb]
    return ent["img"]


def test_replanned_rows_equal_encoders_then_fused_sampler():
    cfg, m, den = build("noise", "bf16")
    encs = encoders(cfg)
    n = 8
    pol = policy(den, cfg, encs, n)
    obs, goal = frames(cfg, n, 1)
    seeds = [21, 22, 23, 24, 25, 26, 27, 28]
    pol.reset(seeds=seeds)
    for step, envs in enumerate(([4], [1, 4, 6], [0, 2, 3, 5, 7])):                 # m = 1, 3, 5: buckets 1, 4, 8
        act = np.zeros(n, dtype=bool)
        act[envs] = True
        pol.reset(envs=envs)
        draws = pol.draws.cpu().tolist()
        out = pol.step(nan_except(obs, envs), goal, active=act)
        assert pol.replanned == envs
        mb = next(b for b in (1, 2, 4, 8) if b >= len(envs))
        rows = envs + [envs[-1]] * (mb - len(envs))
        tok = tokens(encs, rows_of(obs, rows), goal[rows].contiguous())          # the policy's encoders at batch mb * T on the gathered goals
        got_tok = _chunk_img(pol, mb)
        assert torch.equal(got_tok, tok), (step, rel(got_tok, tok))
        x0 = rollout.env_noise([seeds[r] for r in rows], [draws[r] for r in rows], cfg.action_seq_len, cfg.action_dim, SIGMA_MAX, "cuda")
        ref = gc_sampling.sample_ddim(den, {"state_images": tok}, x0, goal[rows].contiguous(), pol._schedule(goal.device), disable=True)
        assert torch.equal(pol.plans[envs], ref[:len(envs)]), step
        assert torch.equal(out[envs], ref[:len(envs), 0])
        assert torch.isfinite(pol.plans).all()


# ------------------------------------------------------------------------------------------------------------------ 3. isolation
def test_plan_does_not_depend_on_bucket_mates_or_other_rows():
    cfg, m, den = build("noise", "bf16")
    encs = encoders(cfg)
    n = 6
    obs_a, goal = frames(cfg, n, 2)
    obs_b, _ = frames(cfg, n, 3)
    for b in (2,):                                                                 # env 2: the same frames and goal in both runs
        for v_a, v_b in zip(obs_a["rgb_obs"].values(), obs_b["rgb_obs"].values()):
            v_b[b] = v_a[b]
    plans = []
    for obs, envs in ((obs_a, [0, 2, 4]), (obs_b, [1, 2, 3])):                     # env 2 at row 1 of bucket 4 with other mates, other contents
        pol = policy(den, cfg, encs, n)
        act = np.zeros(n, dtype=bool)
        act[envs] = True
        pol.step(nan_except(obs, envs), goal, active=act)
        assert torch.isfinite(pol.plans[envs]).all()
        plans.append(pol.plans[2].clone())
    assert torch.equal(plans[0], plans[1])


# ------------------------------------------------------------------------------------------------------------------ 4. staggered = solo
@pytest.mark.parametrize("mode", ["noise", "goal", "token"])
def test_staggered_episodes_with_frames_equal_solo_agents(mode):
    cfg, m, den = build(mode, "bf16")
    encs = encoders(cfg)
    n, steps, multistep = 4, 14, 4
    rng = np.random.default_rng(11)
    resets, active = _schedule_of_events(n, steps, rng)
    obs_t = [frames(cfg, n, 100 + t)[0] for t in range(steps)]
    g = torch.Generator().manual_seed(12)
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
            outs.append(pol.step(rows_of(obs_t[t], envs), torch.cat([cur[b] for b in envs]), active=active[t, envs]).clone())
        return torch.stack(outs, 1)

    batched = run(policy(den, cfg, encs, n, seed=300, multistep=multistep), list(range(n)))
    for b in range(n):
        solo = run(policy(den, cfg, encs, 1, seed=300 + b, multistep=multistep), [b])[0]
        got = batched[b]
        assert not got[~torch.from_numpy(active[:, b]).cuda()].any()
        assert rel(got, solo) <= (BF16_TOKROUTE_OUT if mode == "token" else BF16_OUT), (mode, b, rel(got, solo))


# ------------------------------------------------------------------------------------------------------------------ 5. frames = embeddings
def test_frames_equal_embeddings():
    cfg, m, den = build("noise", "bf16")
    encs = encoders(cfg)
    n, multistep = 4, 3
    pf, pe = policy(den, cfg, encs, n, multistep=multistep), policy(den, cfg, encs, n, multistep=multistep)
    rng = np.random.default_rng(4)
    for t in range(8):
        obs, goal = frames(cfg, n, 40 + t)
        act = np.ones(n, dtype=bool) if t == 0 else rng.random(n) > 0.3
        if t == 4:
            pf.reset(envs=[1, 3]); pe.reset(envs=[1, 3])
        a = pf.step(obs, goal, active=act)
        b = pe.step(pe.embed(obs, goal), goal, active=act)
        assert pf.replanned == pe.replanned
        if t == 0:                                                                 # lockstep: the encoder batch is num_envs on both routes
            assert pf.replanned == list(range(n)) and torch.equal(a, b) and torch.equal(pf.plans, pe.plans)
        elif pf.replanned:
            assert rel(pf.plans[pf.replanned], pe.plans[pe.replanned]) <= BF16_OUT, t
        assert torch.equal(a[~torch.from_numpy(act).cuda()], b[~torch.from_numpy(act).cuda()])              # inactive: zero rows on both
        if b.any():
            assert rel(a, b) <= BF16_OUT, t


# ------------------------------------------------------------------------------------------------------------------ 6. budget
def test_capture_replay_budget_no_sync_and_weight_updates(monkeypatch):
    cfg, m, den = build("noise", "bf16")
    encs = encoders(cfg)
    n = 8
    pol = policy(den, cfg, encs, n)
    obs, goal = frames(cfg, n, 5, hg=48)
    pol.warmup(obs, goal)
    assert sorted(pol._enc_store) == [1, 2, 4, 8] and len(pol.encoders._graphs) == 0
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
        pol.step(obs, goal, active=act)
        assert pol.replanned == envs and cnt["replay"] == before + 2, size
    assert cnt["capture"] == 0
    for t in range(10):
        pol.step(obs, goal, active=np.arange(n) <= t)
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        replans = 0
        for t in range(200):
            before = cnt["replay"]
            pol.step(obs, goal, active=np.arange(n) != t % n)
            replans += bool(pol.replanned)
            assert cnt["replay"] - before == (2 if pol.replanned else 0)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert replans > 20 and cnt["capture"] == 0
    assert torch.cuda.memory_allocated() == mem
    # an in-place weight change is seen by the next replan: env 0 replans from the same seed and draw before and after
    def replan0():
        pol.reset(envs=[0], seeds=[77])
        act = np.zeros(n, dtype=bool)
        act[0] = True
        pol.step(obs, goal, active=act)
        return pol.plans[0].clone(), _chunk_img(pol, 1)[0].clone()
    before_plan, _ = replan0()
    with torch.no_grad():
        encs[0].resnet.conv1.weight.mul_(1.05); encs[1].film4.gamma.weight.add_(0.01)
    after_plan, after_tok = replan0()
    assert cnt["capture"] == 0 and not torch.equal(before_plan, after_plan)
    assert torch.equal(after_tok, tokens(encs, rows_of(obs, [0]), goal[:1])[0])


def test_eager_fallback_matches_graphs(monkeypatch):
    cfg, m, den = build("noise", "bf16")
    encs = encoders(cfg)
    n = 4
    obs, goal = frames(cfg, n, 6)
    act = np.array([True, False, True, True])
    graphed = policy(den, cfg, encs, n)
    graphed.step(obs, goal, active=act)
    monkeypatch.setenv("MODE_HIP_GRAPH", "0")
    eager = policy(den, cfg, encs, n)
    eager.step(obs, goal, active=act)
    assert eager._enc_store[4]["graph"] is None
    assert torch.equal(eager.plans, graphed.plans)
