"""Action chunks longer than 12 steps (T = 17 .. 64 tokens per sample) and action widths above 8 (up to 32) through the whole HIP path - MoDeDiT
forward, the fused samplers, the training chain (forward with stash, HIP backward, EDM loss, attention / expert dropout) and the chunked rollout
policy on both sides of the small-batch (skinny GEMM) switch - against the oracle.  Not fixture geometries: bf16 outputs are held to
tolerances.OUT_FUZZ, fp32 to FP32_OUT / FP32_GRAD, bf16 training to BF16_TRAIN_OUT / BF16_GRAD."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import gc_sampling, rollout, samplers  # noqa: E402
from oracle import mode_oracle as O  # noqa: E402
from oracle.weights import make_inputs, make_state_dict  # noqa: E402

from tolerances import BF16_GRAD, BF16_TRAIN_OUT, FP32_GRAD, FP32_LOSS, OUT_FUZZ  # noqa: E402


def rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _cfg(A_len, A_dim, **kw):
    base = dict(obs_dim=64, goal_dim=32, action_dim=A_dim, embed_dim=256, n_layers=2, n_heads=2, action_seq_len=A_len, num_experts=4, top_k=2)
    base.update(kw)
    return O.DiTConfig(**base)


def _model(cfg, sd, dtype, train=False, **kw):
    args = dict(attn_pdrop=0.3, mlp_pdrop=0.1, goal_drop=0.1)
    if train:
        args.update(attn_pdrop=0.0, mlp_pdrop=0.0, goal_drop=0.0, use_argmax=True)
    args.update(kw)
    m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cuda", goal_conditioned=True, action_dim=cfg.action_dim,
                  embed_dim=cfg.embed_dim, embed_pdrob=0, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1, obs_seq_len=1,
                  action_seq_len=cfg.action_seq_len, state_dim=None, num_experts=cfg.num_experts, top_k=cfg.top_k, compute_dtype=dtype,
                  router_normalize=cfg.router_normalize, use_goal_in_routing=cfg.use_goal_in_routing,
                  use_noise_token_as_input=cfg.use_noise_token_as_input, cond_router=cfg.cond_router, **args)
    m.load_state_dict(sd)
    return m.to("cuda").train() if train else m.to("cuda").eval()


FWD_CASES = [(13, 7, {}), (16, 14, {"n_heads": 4}), (20, 7, {"use_noise_token_as_input": False}), (32, 16, {}), (60, 32, {"n_heads": 4})]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("A_len,A_dim,extra", FWD_CASES)
def test_forward_and_fused_ddim_vs_oracle(A_len, A_dim, extra, dtype):
    cfg = _cfg(A_len, A_dim, **extra)
    assert 16 < cfg.seq_len <= 64
    seed = 40 + A_len + A_dim
    sd = make_state_dict(cfg, seed)
    m = _model(cfg, sd, dtype)
    B = 6
    inp = make_inputs(cfg, B, seed + 1)
    sig = O.rand_log_logistic((B,), float(np.log(0.5)), 0.5, 1e-3, 80.0, generator=torch.Generator().manual_seed(seed))
    ref, aux = O.dit_forward(sd, cfg, inp["state_images"], inp["actions"], inp["goals"], sig, return_aux=True)
    c = {k: v.cuda() for k, v in inp.items()}
    with torch.no_grad():
        out = m({"state_images": c["state_images"]}, c["actions"], c["goals"], sig.cuda())
    what = f"{dataclasses.asdict(cfg)} {dtype}"
    assert out.shape == (B, A_len, A_dim)
    assert torch.equal(m._last_topk.cpu().long(), torch.stack(aux.topk_idx)[:, :, 0, :]), what
    assert rel(out, ref) < OUT_FUZZ[dtype], (what, rel(out, ref))
    den = M.GCDenoiser(m, 0.5).eval()
    sched = M.get_sigmas_exponential(10, 1e-3, 80.0)
    x = M.sample_ddim(den, {"state_images": c["state_images"]}, c["x0"], c["goals"], sched.cuda(), disable=True)
    xr = O.sample_ddim(sd, cfg, 0.5, inp["state_images"], inp["x0"], inp["goals"], sched)
    assert rel(x, xr) < OUT_FUZZ[dtype], (what, rel(x, xr))


@pytest.mark.parametrize("A_len,A_dim", [(20, 14), (60, 32)])
def test_token_routing_vs_oracle(A_len, A_dim):
    """cond_router=False (every token routed on its own state, inside the chain), fp32: asserted like the fuzz file's token-routing test."""
    cfg = _cfg(A_len, A_dim, cond_router=False)
    sd = make_state_dict(cfg, 77)
    m = _model(cfg, sd, "fp32")
    B = 5
    inp = make_inputs(cfg, B, 78)
    sig = torch.full((B,), 0.9)
    ref, aux = O.dit_forward(sd, cfg, inp["state_images"], inp["actions"], inp["goals"], sig, return_aux=True)
    c = {k: v.cuda() for k, v in inp.items()}
    with torch.no_grad():
        out = m({"state_images": c["state_images"]}, c["actions"], c["goals"], sig.cuda())
    want = torch.stack(aux.topk_idx).reshape(cfg.n_layers, -1, cfg.top_k).long()
    got = m._last_topk.cpu().long()
    same = (got.sort(-1).values == want.sort(-1).values).all(-1).float().mean().item()
    assert same >= 0.995, same
    if same == 1.0:
        assert rel(out, ref) < 1e-3


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_multistep_and_two_stage_samplers(dtype):
    """dpmpp_2m (fused multistep head) and heun (two-stage head) on a 24-token model with 14-wide actions: the fused chain equals the sampler's own
    step loop (forced by a callback), as tests/test_samplers.py checks at T = 14, and the DDIM chunk matches the oracle."""
    cfg = _cfg(20, 14)
    sd = make_state_dict(cfg, 91)
    m = _model(cfg, sd, dtype)
    den = M.GCDenoiser(m, 0.5).eval()
    inp = {k: v.cuda() for k, v in make_inputs(cfg, 6, 92).items()}
    state = {"state_images": inp["state_images"]}
    sig = gc_sampling.get_sigmas_exponential(10, 0.001, 80.0, "cuda")
    for name, fn, t32 in (("dpmpp_2m", samplers.sample_dpmpp_2m, 3e-6), ("heun", samplers.sample_heun, 1e-5)):
        tol = t32 if dtype == "fp32" else OUT_FUZZ["bf16"]
        steps = []
        loop = fn(den, state, inp["x0"], inp["goals"], sig, disable=True, callback=lambda d: steps.append(d["i"]))
        assert steps == list(range(len(sig) - 1))
        fused = fn(den, state, inp["x0"], inp["goals"], sig, disable=True)
        assert fused.shape == (6, 20, 14) and torch.isfinite(fused).all()
        assert rel(fused, loop) < tol, (name, rel(fused, loop))
        assert torch.equal(fused, fn(den, state, inp["x0"], inp["goals"], sig, disable=True))


def _grad_check(m, sdg, tol, min_checked):
    gmax = max(float(v.grad.norm()) for v in sdg.values() if v.grad is not None)
    checked, worst = 0, (0.0, "")
    for n, p in m.named_parameters():
        r = sdg[n].grad
        if r is None or float(r.norm()) < 1e-6 * gmax:
            assert p.grad is None or float(p.grad.norm()) < 1e-5 * gmax, n
            continue
        e = rel(p.grad, r)
        assert e < tol, (n, e)
        worst = max(worst, (e, n))
        checked += 1
    assert checked >= min_checked
    return worst


@pytest.mark.parametrize("A_len,A_dim", [(20, 14), (60, 32)])
def test_training_vs_oracle_autograd_fp32(A_len, A_dim):
    cfg = _cfg(A_len, A_dim, n_heads=4)
    sd = make_state_dict(cfg, 300 + A_len)
    m = _model(cfg, sd, "fp32", train=True)
    B = 6
    inp = make_inputs(cfg, B, 301 + A_len)
    sig = O.rand_log_logistic((B,), float(np.log(0.5)), 0.5, 1e-3, 80.0, generator=torch.Generator().manual_seed(A_len))
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref_loss, _ = O.denoiser_loss(sdg, cfg, 0.5, inp["state_images"], inp["actions"], inp["goals"], inp["noise"], sig)
    ref_loss.backward()
    c = {k: v.cuda() for k, v in inp.items()}
    den = M.GCDenoiser(m, 0.5).train()
    loss, _ = den.loss({"state_images": c["state_images"]}, c["actions"], c["goals"], c["noise"], sig.cuda())
    loss.backward()
    assert abs(float(loss) - float(ref_loss)) < FP32_LOSS * abs(float(ref_loss))
    _grad_check(m, sdg, FP32_GRAD, 15)


def test_training_with_dropout_vs_oracle():
    """Attention dropout 0.3 and expert dropout 0.1 at T = 36 (32-step chunk, 16-wide actions), fp32: the hash masks are restated by the oracle
    (attn_keep_scale / mlp_keep_scale), the routing is top-k (use_argmax) so that the comparison is exact up to arithmetic precision."""
    torch.manual_seed(11)
    cfg = _cfg(32, 16)
    sd = make_state_dict(cfg, 411)
    m = _model(cfg, sd, "fp32", train=True, attn_pdrop=0.3, mlp_pdrop=0.1)
    B = 8
    inp = make_inputs(cfg, B, 412)
    sig = O.rand_log_logistic((B,), float(np.log(0.5)), 0.5, 1e-3, 80.0, generator=torch.Generator().manual_seed(413))
    c = {k: v.cuda() for k, v in inp.items()}
    den = M.GCDenoiser(m, 0.5).train()
    loss, _ = den.loss({"state_images": c["state_images"]}, c["actions"], c["goals"], c["noise"], sig.cuda())
    loss.backward()
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref_loss, _ = O.denoiser_loss(sdg, cfg, 0.5, inp["state_images"], inp["actions"], inp["goals"], inp["noise"], sig,
                                  dropout=dict(seed=m._last_seed, attn_p=0.3, mlp_p=0.1))
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) < FP32_LOSS * abs(float(ref_loss)), (float(loss), float(ref_loss))
    _grad_check(m, sdg, FP32_GRAD, 15)


def test_training_bf16_vs_oracle():
    """The bf16 training chain at T = 24 with 14-wide actions against the fp32 oracle's autograd, at the reference's own bf16 bounds."""
    torch.manual_seed(12)
    cfg = _cfg(20, 14, n_heads=4)
    sd = make_state_dict(cfg, 421)
    m = _model(cfg, sd, "bf16", train=True)
    B = 8
    inp = make_inputs(cfg, B, 422)
    sig = O.rand_log_logistic((B,), float(np.log(0.5)), 0.5, 1e-3, 80.0, generator=torch.Generator().manual_seed(423))
    c = {k: v.cuda() for k, v in inp.items()}
    den = M.GCDenoiser(m, 0.5).train()
    loss, _ = den.loss({"state_images": c["state_images"]}, c["actions"], c["goals"], c["noise"], sig.cuda())
    loss.backward()
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref_loss, _ = O.denoiser_loss(sdg, cfg, 0.5, inp["state_images"], inp["actions"], inp["goals"], inp["noise"], sig)
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) < BF16_TRAIN_OUT * abs(float(ref_loss)), (float(loss), float(ref_loss))
    _grad_check(m, sdg, BF16_GRAD, 15)


def _rollout_model(dtype):
    cfg = _cfg(20, 14)
    sd = make_state_dict(cfg, 501)
    return cfg, sd, _model(cfg, sd, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 2, 32])
def test_chunked_rollout_long_window(B, dtype, monkeypatch):
    """ChunkedRolloutPolicy(act_window_size=20, multistep=10) with 14-wide actions (T = 24): B = 1 takes the small-batch chain (24 token rows
    <= gemm_skinny_rows), B = 2 and 32 the tiled one.  Graphed and eager chunks give the same actions; the plan is the oracle's DDIM from the
    same noise."""
    cfg, sd, m = _rollout_model(dtype)
    den = M.GCDenoiser(m, 0.5).eval()
    inp = make_inputs(cfg, B, 502)
    c = {k: v.cuda() for k, v in inp.items()}
    obs = {"state_images": c["state_images"]}
    mk = lambda: rollout.ChunkedRolloutPolicy(den, num_sampling_steps=10, multistep=10, act_window_size=20, action_dim=14,
                                              generator=torch.Generator(device="cuda").manual_seed(7))
    pol = mk()
    acts = [pol.step(obs, c["goals"].squeeze(1)).clone() for _ in range(10)]
    assert all(a.shape == (B, 14) and torch.isfinite(a).all() for a in acts)
    plan = mk().denoise_actions(obs, c["goals"])
    assert plan.shape == (B, 20, 14)
    for t in range(10):
        assert torch.equal(acts[t], plan[:, t])
    monkeypatch.setenv("MODE_HIP_GRAPH", "0")
    eager = mk().denoise_actions(obs, c["goals"])
    monkeypatch.delenv("MODE_HIP_GRAPH")
    assert torch.equal(plan, eager)
    sig = rollout.get_noise_schedule(10, "exponential", 1e-3, 80.0, "cpu")
    x0 = torch.randn((B, 20, 14), device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) * 80.0
    ref = O.sample_ddim(sd, cfg, 0.5, inp["state_images"], x0.cpu(), inp["goals"], sig)
    assert rel(plan, ref) < OUT_FUZZ[dtype], rel(plan, ref)
