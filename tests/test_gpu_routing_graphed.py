"""Goal-routed (use_goal_in_routing=True, fixture F9_goalroute) and token-routed (cond_router=False, fixture F14) denoisers on the captured sampling
paths: sample_ddim / sample_dpmpp_2m / heun / dpm_2 / dpmpp_2s as ONE hipGraph replay per sampler call, the ancestral samplers as one
denoise_graphed replay per denoiser call, a replanning ChunkedRolloutPolicy.step as one replay.  Each result is checked against the per-step path
(MODE_HIP_GRAPH=0: same inputs, fp32 within 1e-5 rel, identical experts at every level and layer) and against the oracle's step loop
(tests/tolerances.py), with fresh goals, per-sample routing and the expert-usage counters."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import gc_sampling, rollout, samplers  # noqa: E402
from oracle import mode_oracle as O  # noqa: E402
from oracle.weights import get_config, make_inputs, make_state_dict  # noqa: E402

from tolerances import BF16_OUT, BF16_TOKROUTE_AGREE, BF16_TOKROUTE_OUT, FP32_OUT  # noqa: E402

MODES = {"goal": (220, dict(use_goal_in_routing=True)),           # F9_goalroute: c1e4, seed 220
         "token": (230, dict(cond_router=False))}                  # F14_c1e4_token_routing: c1e4, seed 230

CHUNK_SAMPLERS = {
    "ddim": lambda den, st, x, g, s: gc_sampling.sample_ddim(den, st, x, g, s, disable=True),
    "dpmpp_2m": lambda den, st, x, g, s: samplers.sample_dpmpp_2m(den, st, x, g, s, disable=True),
    "heun": lambda den, st, x, g, s: samplers.sample_heun(den, st, x, g, s, disable=True),
    "dpm_2": lambda den, st, x, g, s: samplers.sample_dpm_2(den, st, x, g, s, disable=True),
    "dpmpp_2s": lambda den, st, x, g, s: samplers.sample_dpmpp_2s(den, st, x, g, s, disable=True),
}


def rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def build(mode, dtype):
    seed, over = MODES[mode]
    cfg = get_config("c1e4")
    m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cuda", goal_conditioned=True, action_dim=cfg.action_dim,
                  embed_dim=cfg.embed_dim, embed_pdrob=0, attn_pdrop=0.3, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1,
                  obs_seq_len=1, action_seq_len=cfg.action_seq_len, num_experts=cfg.num_experts, top_k=cfg.top_k, compute_dtype=dtype, **over)
    sd = make_state_dict(cfg, seed)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    return dataclasses.replace(cfg, **over), sd, m, M.GCDenoiser(m, 0.5).eval()


def inputs(cfg, B, seed):
    return {k: v.cuda() for k, v in make_inputs(cfg, B, seed).items()}


@pytest.fixture
def replays(monkeypatch):
    """Counts torch.cuda.CUDAGraph.replay calls."""
    cnt = {"n": 0}
    orig = torch.cuda.CUDAGraph.replay

    def counted(self):
        cnt["n"] += 1
        return orig(self)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", counted)
    return cnt


def per_step(monkeypatch, m, fn):
    """Run ``fn`` on the per-step path (MODE_HIP_GRAPH=0); returns (result, experts of every denoiser call stacked on dim 1 - [L, calls, ...])."""
    rec = []
    orig = m.denoise

    def recording(*a, **k):
        out = orig(*a, **k)
        rec.append(m._last_topk.clone())
        return out
    monkeypatch.setenv("MODE_HIP_GRAPH", "0")
    m.denoise = recording
    try:
        out = fn()
    finally:
        del m.denoise
        monkeypatch.delenv("MODE_HIP_GRAPH")
    return out, torch.stack(rec, 1)


def oracle_run(sd, cfg, name, st, x0, goals, sig):
    """The sampler's step loop on the oracle's denoiser (CPU fp32); returns (result, experts per call stacked on dim 1)."""
    rec = []

    def den(state, action, goal, sigma, **kw):
        out, aux = O.denoiser_forward(sd, cfg, 0.5, state["state_images"], action, goal, sigma, return_aux=True)
        idx = torch.stack(aux.topk_idx)                                    # [L, B, T, k]
        rec.append(idx[:, :, 0, :] if cfg.cond_router else idx.reshape(idx.shape[0], -1, idx.shape[-1]))
        return out
    cpu = lambda t: t.detach().cpu()
    out = CHUNK_SAMPLERS[name](den, {"state_images": cpu(st["state_images"])}, cpu(x0), cpu(goals), cpu(sig))
    return out, torch.stack(rec, 1)


def agreement(a, b):
    """Fraction of routing decisions (rows of k experts, order-free) that agree."""
    a, b = a.cpu().long().sort(-1).values, b.cpu().long().sort(-1).values
    return (a == b).all(-1).float().mean().item()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["goal", "token"])
def test_chunk_samplers_are_one_replay_and_match(mode, dtype, replays, monkeypatch):
    cfg, sd, m, den = build(mode, dtype)
    B = 5
    inp = inputs(cfg, B, MODES[mode][0] + 1)
    st = {"state_images": inp["state_images"]}
    sig = gc_sampling.get_sigmas_exponential(10, 1e-3, 80.0, "cuda")
    for name, fn in CHUNK_SAMPLERS.items():
        replays["n"] = 0
        x = fn(den, st, inp["x0"], inp["goals"], sig)
        assert replays["n"] == 1, (name, replays["n"])                         # the whole sampler call is one replay
        got_idx = m._last_topk.clone()                                         # [L, evaluations, B, k] (goal) / [L, evaluations, B*T, k] (token)
        replays["n"] = 0
        assert torch.equal(x, fn(den, st, inp["x0"], inp["goals"], sig)) and replays["n"] == 1, name     # replay of the cached graph
        ref, ref_idx = per_step(monkeypatch, m, lambda: fn(den, st, inp["x0"], inp["goals"], sig))
        assert replays["n"] == 1, name                                         # (the per-step path replays nothing)
        orc, orc_idx = oracle_run(sd, cfg, name, st, inp["x0"], inp["goals"], sig)
        assert got_idx.shape == ref_idx.shape == orc_idx.shape, (name, tuple(got_idx.shape), tuple(ref_idx.shape))
        if dtype == "fp32":
            assert torch.equal(got_idx.cpu(), ref_idx.cpu()), name
            assert rel(x, ref) < 1e-5, (name, rel(x, ref))
            assert rel(x, orc) < FP32_OUT, (name, rel(x, orc))
        if mode == "goal":                                                     # router input emb(sigma) + goal_emb(goal): fp32 in both modes
            assert torch.equal(got_idx.cpu().long(), orc_idx.long()), name
            if dtype == "bf16":
                assert rel(x, orc) < BF16_OUT, (name, rel(x, orc))
        else:
            assert agreement(got_idx, orc_idx) >= BF16_TOKROUTE_AGREE, (name, agreement(got_idx, orc_idx))
            if dtype == "bf16":
                assert rel(x, orc) < BF16_TOKROUTE_OUT, (name, rel(x, orc))
        print(f"{mode} {dtype} {name}: vs per-step {rel(x, ref):.2e}, vs oracle {rel(x, orc):.2e}")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["goal", "token"])
def test_ancestral_is_one_denoise_replay_per_call(mode, dtype, replays, monkeypatch):
    cfg, sd, m, den = build(mode, dtype)
    B = 5
    inp = inputs(cfg, B, MODES[mode][0] + 1)
    st = {"state_images": inp["state_images"]}
    sig = gc_sampling.get_sigmas_exponential(10, 1e-3, 80.0, "cuda")
    run = lambda eta: samplers.sample_euler_ancestral(den, st, inp["x0"], inp["goals"], sig, disable=True, eta=eta)
    torch.manual_seed(3)
    x = run(1.0)
    assert replays["n"] == len(sig) - 1                                        # one denoise_graphed replay per denoiser call
    torch.manual_seed(3)
    ref, _ = per_step(monkeypatch, m, lambda: run(1.0))
    tol = 1e-5 if dtype == "fp32" else (BF16_OUT if mode == "goal" else BF16_TOKROUTE_OUT)
    assert rel(x, ref) < tol, rel(x, ref)
    x0 = run(0.0)                                                              # eta = 0: deterministic, comparable with the oracle's step loop
    cpu = lambda t: t.detach().cpu()
    orc = samplers.sample_euler_ancestral(lambda s, a, g, sg, **kw: O.denoiser_forward(sd, cfg, 0.5, s["state_images"], a, g, sg),
                                          {"state_images": cpu(st["state_images"])}, cpu(inp["x0"]), cpu(inp["goals"]), cpu(sig), eta=0.0)
    assert rel(x0, orc) < (FP32_OUT if dtype == "fp32" else tol), rel(x0, orc)


@pytest.mark.parametrize("mode", ["goal", "token"])
def test_fresh_goals_and_in_place_edits(mode, monkeypatch):
    """Two calls with different goals, and a call after an in-place edit of the goals (same tensor object): every result is the per-step path's."""
    cfg, sd, m, den = build(mode, "fp32")
    B = 5
    inp = inputs(cfg, B, 41)
    st = {"state_images": inp["state_images"]}
    sig = gc_sampling.get_sigmas_exponential(10, 1e-3, 80.0, "cuda")
    goals = [inp["goals"].clone(), torch.randn_like(inp["goals"])]
    runs = {"ddim": lambda g: gc_sampling.sample_ddim(den, st, inp["x0"], g, sig, disable=True),
            "heun": lambda g: samplers.sample_heun(den, st, inp["x0"], g, sig, disable=True),
            "euler_ancestral": lambda g: samplers.sample_euler_ancestral(den, st, inp["x0"], g, sig, disable=True, eta=0.0)}
    for name, fn in runs.items():
        outs = []
        for g in goals + [None]:
            if g is None:
                g = goals[1]
                g.mul_(-0.5).add_(0.25)                                         # in place: same object, new values
            x = fn(g)
            ref, _ = per_step(monkeypatch, m, lambda: fn(g))
            assert rel(x, ref) < 1e-5, (name, rel(x, ref))
            outs.append(x)
        assert rel(outs[0], outs[1]) > 1e-3 and rel(outs[1], outs[2]) > 1e-3, name


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["goal", "token"])
def test_per_sample_routing(mode, dtype):
    """B = 32 distinct goals in one graphed chunk: sample b routes (and, in fp32, denoises) as a B = 1 run on sample b alone."""
    cfg, sd, m, den = build(mode, dtype)
    B = 32
    inp = inputs(cfg, B, 57)
    sig = gc_sampling.get_sigmas_exponential(10, 1e-3, 80.0, "cuda")
    x = gc_sampling.sample_ddim(den, {"state_images": inp["state_images"]}, inp["x0"], inp["goals"], sig, disable=True)
    idx = m._last_topk.clone()
    T = m.seq_len
    for b in range(B):
        xb = gc_sampling.sample_ddim(den, {"state_images": inp["state_images"][b:b + 1]}, inp["x0"][b:b + 1], inp["goals"][b:b + 1], sig, disable=True)
        ib = m._last_topk
        mine = idx[:, :, b:b + 1] if mode == "goal" else idx[:, :, b * T:(b + 1) * T]
        if mode == "goal" or dtype == "fp32":
            assert torch.equal(mine, ib), b
        else:
            assert agreement(mine, ib) >= BF16_TOKROUTE_AGREE, b
        if dtype == "fp32":
            assert rel(x[b:b + 1], xb) < 1e-5, (b, rel(x[b:b + 1], xb))
        elif mode == "goal":
            assert rel(x[b:b + 1], xb) < BF16_OUT, b
        # (token routing in bf16: two runs whose GEMM row counts differ round differently, near-tied tokens flip, and one sample's error is not
        # bounded by the batch tolerance - their decisions are held to BF16_TOKROUTE_AGREE above, the outputs to the oracle in the tests above)
    goal_rows = idx.shape[2] if mode == "goal" else idx.shape[2] // T
    assert goal_rows == B


@pytest.mark.parametrize("mode", ["goal", "token"])
def test_usage_counters_match_the_per_step_path(mode, monkeypatch):
    cfg, sd, m, den = build(mode, "fp32")
    B = 5
    inp = inputs(cfg, B, 63)
    st = {"state_images": inp["state_images"]}
    sig = gc_sampling.get_sigmas_exponential(10, 1e-3, 80.0, "cuda")

    def counters(fn):
        m.sync_expert_usage()
        for blk in m.blocks:
            blk.reset_expert_usage()
        fn()
        m.sync_expert_usage()
        return torch.stack([blk.get_expert_usage().clone() for blk in m.blocks]), [blk.total_tokens_processed for blk in m.blocks]

    for name in ("ddim", "heun"):
        fn = lambda: CHUNK_SAMPLERS[name](den, st, inp["x0"], inp["goals"], sig)
        got, got_tok = counters(fn)
        ref, ref_tok = counters(lambda: per_step(monkeypatch, m, fn))
        assert torch.equal(got, ref) and got_tok == ref_tok, (name, got, ref, got_tok, ref_tok)
        n_eval = len(sig) - 1 if name == "ddim" else 2 * (len(sig) - 2) + 1
        assert float(got.sum()) == n_eval * m.num_layers * B * m.seq_len * m.top_k, name


@pytest.mark.parametrize("mode", ["goal", "token"])
@pytest.mark.parametrize("B", [1, 32])
def test_rollout_replans_in_one_replay(mode, B, replays, monkeypatch):
    """A replanning ChunkedRolloutPolicy.step is one replay (DDIM through the fused chunk, euler_ancestral through the policy's whole-call graph) and plans
    what the per-step path plans from the same noise - the routing cache filled from the first environment's goal routes nobody."""
    cfg, sd, m, den = build(mode, "fp32")
    inp = inputs(cfg, B, 71)
    obs = {"state_images": inp["state_images"]}
    goal = inp["goals"].squeeze(1)
    for sampler in ("ddim", "euler_ancestral"):
        mk = lambda: rollout.ChunkedRolloutPolicy(den, sampler_type=sampler, multistep=4, generator=torch.Generator(device="cuda").manual_seed(9))
        pol = mk()
        for t in range(5):                                                      # replans at control steps 0 and 4
            replays["n"] = 0
            a = pol.step(obs, goal)
            assert a.shape == (B, cfg.action_dim) and torch.isfinite(a).all()
            assert replays["n"] == (1 if t % 4 == 0 else 0), (sampler, t, replays["n"])
        if sampler == "ddim":
            torch.manual_seed(4)
            plan = mk().denoise_actions(obs, goal)
            torch.manual_seed(4)
            ref, _ = per_step(monkeypatch, m, lambda: mk().denoise_actions(obs, goal))
            assert rel(plan, ref) < 1e-5, rel(plan, ref)
