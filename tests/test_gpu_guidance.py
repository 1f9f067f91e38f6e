"""Classifier-free guidance on the MI355X: D_w = D_u + w (D_c - D_u) formed inside the fused chain (GCDenoiser(guidance_scale=w)).

1. the two new kernels alone (guided embed / guided head, through ctypes) against torch restatements and against their unguided twins;
2. ``denoise`` against the oracle's composition of two calls (the second with zero goals), three routing modes x fp32 / bf16;
3. the fused samplers against their own step loops and against an oracle loop;
4. batch sizes on both sides of the chain's geometry switches against two unguided GPU calls;
5. scale changes and guided <-> unguided switches on the cached graphs;
6. the rollout policies;  7. refusals before any launch.

Model: c1e4 (embed_dim 256, 2 layers, 4 experts, top-2, 10 action steps) with n_heads = 2 (head dim 128).  The output bound everywhere is the suite's
per-evaluation tolerance pushed through the combine: ||got - ref|| <= OUT_FUZZ[dtype] (|w| ||D_c|| + |1 - w| ||D_u||)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd import gc_sampling, rollout, samplers  # noqa: E402
from oracle import mode_oracle as O  # noqa: E402
from oracle.weights import get_config, make_inputs, make_state_dict  # noqa: E402

import hip_helpers as H  # noqa: E402
from tolerances import BF16_OUT, BF16_TOKROUTE_AGREE, BF16_TOKROUTE_OUT, OUT_FUZZ  # noqa: E402

MODES = {"noise": (310, {}), "goal": (320, dict(use_goal_in_routing=True)), "token": (330, dict(cond_router=False))}
WS = (0.0, 1.0, 2.5)
SIGMA_DATA = 0.5


def nrm(t):
    return float(torch.as_tensor(t).double().cpu().norm())


def rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def combine(d_c, d_u, w):
    return d_u + w * (d_c - d_u)


def bound(dtype, w, d_c, d_u):
    return OUT_FUZZ[dtype] * (abs(w) * nrm(d_c) + abs(1.0 - w) * nrm(d_u))


def build(mode, dtype, **over):
    seed, flags = MODES[mode]
    cfg = dataclasses.replace(get_config("c1e4"), n_heads=2, **flags)
    kw = dict(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cuda", goal_conditioned=True, action_dim=cfg.action_dim, embed_dim=cfg.embed_dim,
              embed_pdrob=0, attn_pdrop=0.3, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1, obs_seq_len=1,
              action_seq_len=cfg.action_seq_len, num_experts=cfg.num_experts, top_k=cfg.top_k, compute_dtype=dtype, **flags)
    kw.update(over)
    m = M.MoDeDiT(**kw)
    sd = make_state_dict(cfg, seed)
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    return cfg, sd, m, M.GCDenoiser(m, SIGMA_DATA).eval()


def inputs(cfg, B, seed):
    return {k: v.cuda() for k, v in make_inputs(cfg, B, seed).items()}


_ORACLE = {}


def oracle_pair(mode, tag):
    """(D_c, D_u, idx_c, idx_u) of the oracle for the mode's B = 5 inputs at one shared / per-sample sigma; computed once, shared, never modified."""
    if (mode, tag) not in _ORACLE:
        seed, flags = MODES[mode]
        cfg = dataclasses.replace(get_config("c1e4"), n_heads=2, **flags)
        sd, inp = make_state_dict(cfg, seed), make_inputs(cfg, 5, seed + 1)
        sig = torch.full((5,), 0.9) if tag == "shared" else torch.tensor([0.9, 0.02, 3.0, 40.0, 0.3])
        out = []
        for goal in (inp["goals"], torch.zeros_like(inp["goals"])):
            d, aux = O.denoiser_forward(sd, cfg, SIGMA_DATA, inp["state_images"], inp["actions"], goal, sig, return_aux=True)
            idx = torch.stack(aux.topk_idx)                                   # [L, B, T, k]
            out.append((d, idx[:, :, 0, :] if cfg.cond_router else idx.reshape(idx.shape[0], -1, idx.shape[-1])))
        _ORACLE[(mode, tag)] = (out[0][0], out[1][0], out[0][1].long(), out[1][1].long(), sig)
    return _ORACLE[(mode, tag)]


# ================================================================================================================== 1. kernels alone
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


@pytest.mark.parametrize("cond_stride", [0, 1])
@pytest.mark.parametrize("lp", ["fp32", "bf16"])
@pytest.mark.parametrize("A_dim", [7, 14])
@pytest.mark.parametrize("D", [256, 1280])
def test_guided_embed_kernel(D, A_dim, lp, cond_stride):
    """3 pairs, A_len = 3: the conditional half is the unguided kernel's output bit for bit, the unconditional half the unguided kernel's on zero goal
    embeddings - with the pair's own sigma token, images, latent and c_in, and its OWN conditioning row (stride D: 2B rows) - plus a torch restatement."""
    lib, p, st = L.load(), H.p, H.stream()
    B, A_len, n_img = 3, 3, 2
    T = 1 + 1 + n_img + A_len
    emb_t, goal_e, img_e = rnd(B, D, seed=1), rnd(B, D, seed=2), rnd(B, n_img, D, seed=3)
    act, c_in = rnd(B, A_len, A_dim, seed=4, scale=5.0), (0.1 + rnd(B, seed=5).abs())
    w_act, pos, g = rnd(D, A_dim, seed=6, scale=0.3), rnd(1 + A_len, D, seed=7, scale=0.2), 1.0 + 0.1 * rnd(D, seed=8)
    cond = rnd(2 * B if cond_stride else 1, D, seed=9)
    dt, tdt = (L.MODE_BF16, torch.bfloat16) if lp == "bf16" else (L.MODE_F32, torch.float32)

    def desc(nb, ge, cnd, x, h):
        return L.ModeEmbedDesc(B=nb, T=T, D=D, A_len=A_len, A_dim=A_dim, n_img=n_img, use_noise_token=1, emb_t=p(emb_t), emb_row_stride=D, goal_e=p(ge),
                               img_e=p(img_e), actions=p(act), c_in=p(c_in), c_in_stride=1, w_act=p(w_act), pos=p(pos), g=p(g), cond=p(cnd),
                               cond_row_stride=D * cond_stride, eps=1e-6, x=p(x), h=p(h), h_dtype=dt)
    x = torch.full((2 * B * T, D), float("nan"), device="cuda"); h = torch.full((2 * B * T, D), float("nan"), dtype=tdt, device="cuda")
    L.check(lib.mode_embed_tokens_guided_fwd(C.byref(L.ModeEmbedGuidedDesc(emb=desc(B, goal_e, cond, x, h))), st), "guided embed")
    halves = []
    for half, ge in enumerate((goal_e, torch.zeros_like(goal_e))):
        xh = torch.empty(B * T, D, device="cuda"); hh = torch.empty(B * T, D, dtype=tdt, device="cuda")
        cnd = cond[half * B:(half + 1) * B].contiguous() if cond_stride else cond
        L.check(lib.mode_embed_tokens_fwd(C.byref(desc(B, ge, cnd, xh, hh)), st), "embed")
        halves.append((xh, hh))
    assert torch.equal(x, torch.cat([halves[0][0], halves[1][0]])) and torch.equal(h, torch.cat([halves[0][1], halves[1][1]]))
    # restatement (fp64)
    f = lambda t: t.double().cpu()
    seq = torch.zeros(2 * B, T, D, dtype=torch.float64)
    for bi in range(2 * B):
        b = bi % B
        seq[bi, 0] = f(emb_t[b])
        seq[bi, 1] = (f(goal_e[b]) if bi < B else 0.0) + f(pos[0])
        seq[bi, 2:2 + n_img] = f(img_e[b]) + f(pos[1])
        seq[bi, 2 + n_img:] = (f(act[b]) * f(c_in[b])) @ f(w_act).t() + f(pos[1:])
    n = (seq.pow(2).sum(-1, keepdim=True).sqrt() * D ** -0.5).clamp_min(1e-6)
    hw = seq / n * f(g) + (f(cond)[:, None, :] if cond_stride else f(cond)[None])
    assert rel(x, seq.reshape(-1, D)) < 1e-6 and rel(h.float(), hw.reshape(-1, D)) < (1e-6 if lp == "fp32" else 4e-3)


@pytest.mark.parametrize("ybf", [False, True])
@pytest.mark.parametrize("A_dim", [7, 14])
@pytest.mark.parametrize("D", [256, 1280])
def test_guided_head_kernel(D, A_dim, ybf):
    """3 pairs, A_len = 3; k in {1, 2}, y_splits in {1, 4}, with / without fused-ln_2 partials, the den_prev and the lin update forms, per-pair and shared
    scalings.  Restatement in fp64; bound: fp32 rounding of D-term reductions (<= 1e-5 relative per branch) through the combine.  Also against the
    combine of two unguided head launches (the twin on all 2B rows), and each branch of the twin directly against its restatement at that
    per-branch bound: the unguided head row kernel's own check."""
    lib, p, st = L.load(), H.p, H.stream()
    B, A_len, n_img, eps = 3, 3, 2, 1e-6
    T = 1 + 1 + n_img + A_len
    N = 2 * B * T
    f = lambda t: t.double().cpu()
    g, g2 = 1.0 + 0.1 * rnd(D, seed=11), 1.0 + 0.2 * rnd(D, seed=12)
    w_out, b_out = rnd(A_dim, D, seed=13, scale=D ** -0.5), rnd(A_dim, seed=14, scale=0.1)
    x_a, den_prev = rnd(B, A_len, A_dim, seed=15, scale=3.0), rnd(B, A_len, A_dim, seed=16)
    aux1, aux2, lin = rnd(B, A_len, A_dim, seed=17), rnd(B, A_len, A_dim, seed=18), torch.tensor([0.3, -0.7, 1.2, 0.5], device="cuda")
    u = rnd(N, D, seed=19)
    ss = u.double().pow(2).view(N, D // 64, 64).sum(-1).float().contiguous()
    scale = torch.tensor([2.5], device="cuda")
    for k in (1, 2):
        NK = N * k
        pos = torch.randperm(NK, generator=torch.Generator().manual_seed(20 + k)).to(torch.int32).view(N, k).cuda()
        posw = (0.2 + rnd(N, k, seed=22).abs()).contiguous()
        for S in (1, 4):
            Y = rnd(S, NK, D, seed=23 + S, scale=0.5).to(torch.bfloat16 if ybf else torch.float32)
            for fused in (False, True):
                for form in ("den_prev", "lin"):
                    for scal_stride in (4, 0):
                        scal = torch.tensor([[0.4, 0.8, 0.6, 0.35], [0.1, 1.1, 0.2, 0.0], [0.9, 0.3, 0.5, 1.5]], device="cuda")[: B if scal_stride else 1].contiguous()
                        what = (D, A_dim, ybf, k, S, fused, form, scal_stride)

                        def head(nb, xa, sc, sc_stride, **out):
                            return L.ModeHeadDesc(B=nb, T=T, D=D, A_len=A_len, A_dim=A_dim, k=k, u=p(u), Y=p(Y), y_dtype=L.MODE_BF16 if ybf else L.MODE_F32,
                                                  y_splits=S, y_split_stride=NK * D, pos=p(pos), posw=p(posw), g=p(g), eps=eps, w_out=p(w_out), b_out=p(b_out),
                                                  x_a=p(xa), scal=p(sc), scal_stride=sc_stride, u_ss=p(ss) if fused else None, u_ss_n=D // 64,
                                                  u_gain=p(g2) if fused else None, **out)
                        den = torch.full_like(x_a, float("nan")); xn = torch.full_like(x_a, float("nan"))
                        upd = dict(den_prev=p(den_prev)) if form == "den_prev" else dict(lin=p(lin), aux1=p(aux1), aux2=p(aux2))
                        gd = L.ModeHeadGuidedDesc(head=head(B, x_a, scal, scal_stride, denoised=p(den), x_next=p(xn), **upd), scale=p(scale))
                        L.check(lib.mode_head_ddim_guided_fwd(C.byref(gd), st), "guided head")
                        # the twin on all 2B rows: each branch's own prediction
                        both = torch.empty(2 * B, A_len, A_dim, device="cuda")
                        sc2 = torch.cat([scal, scal]).contiguous() if scal_stride else scal
                        L.check(lib.mode_head_ddim_fwd(C.byref(head(2 * B, torch.cat([x_a, x_a]).contiguous(), sc2, scal_stride, denoised=p(both))), st), "head")
                        twin = combine(both[:B], both[B:], 2.5)
                        # restatement
                        rows = torch.tensor([[(b + hf * B) * T + (T - A_len) + ai for ai in range(A_len)] for hf in range(2) for b in range(B)]).view(2, B, A_len)
                        uu = f(u)
                        if fused:
                            uu = uu / (f(ss).sum(1, keepdim=True).sqrt() * D ** -0.5).clamp_min(eps) * f(g2)
                        ysum = f(Y.float()).sum(0)
                        v = uu + (f(posw)[:, :, None] * ysum[pos.long().cpu()]).sum(1)
                        nv = v / (v.pow(2).sum(1, keepdim=True).sqrt() * D ** -0.5).clamp_min(eps) * f(g)
                        Fh = (nv @ f(w_out).t() + f(b_out))[rows]                        # [2, B, A_len, A_dim]
                        s = f(scal).expand(B, 4)[:, None, None, :]
                        dh = Fh * s[None, ..., 1] + f(x_a) * s[None, ..., 0]
                        want = combine(dh[0], dh[1], 2.5)
                        tol = 1e-5 * (2.5 * nrm(dh[0]) + 1.5 * nrm(dh[1]))
                        assert nrm(f(den) - want) <= tol, (what, nrm(f(den) - want), tol)
                        assert nrm(f(den) - f(twin)) <= tol, what
                        for hf, br in enumerate((both[:B], both[B:])):                    # the unguided head row kernel itself, per branch
                            assert nrm(f(br) - dh[hf]) <= 1e-5 * nrm(dh[hf]), (what, hf, nrm(f(br) - dh[hf]), 1e-5 * nrm(dh[hf]))
                        if form == "den_prev":
                            dd = torch.where(s[..., 3] != 0, (1 + s[..., 3]) * want - s[..., 3] * f(den_prev), want)
                            xw = s[..., 2] * f(x_a) + (1 - s[..., 2]) * dd
                        else:
                            l = f(lin)
                            xw = l[0] * f(x_a) + l[1] * want + l[2] * f(aux1) + l[3] * f(aux2)
                        assert nrm(f(xn) - xw) <= 3 * tol, (what, nrm(f(xn) - xw), tol)
    bad = L.ModeHeadGuidedDesc(head=head(B, x_a, scal, 0, denoised=p(den), F=p(xn)), scale=p(scale))
    assert lib.mode_head_ddim_guided_fwd(C.byref(bad), st) == -1                      # MODE_ERR_BAD_ARG: the raw output F has no guided form


# ================================================================================================================== 2. denoise vs the oracle
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["noise", "goal", "token"])
def test_denoise_vs_oracle_composition(mode, dtype):
    cfg, sd, m, den = build(mode, dtype)
    inp = inputs(cfg, 5, MODES[mode][0] + 1)
    st = {"state_images": inp["state_images"]}
    L_, T = cfg.n_layers, cfg.seq_len
    for tag in ("shared", "persample"):
        d_c, d_u, i_c, i_u, sig = oracle_pair(mode, tag)
        for w in WS:
            den.guidance_scale = w
            with torch.no_grad():
                got = den(st, inp["actions"], inp["goals"], sig[:1].cuda() if tag == "shared" else sig.cuda())
            idx = m._last_topk.cpu().long()
            ref = combine(d_c, d_u, w)
            keep = slice(None)
            if cfg.cond_router:                                                       # conditioning-row routing: the router input is fp32 in both compute modes
                one_row = mode == "noise" and tag == "shared"                        # one routing row for all 2B samples
                want = i_c[:, :1] if one_row else torch.cat([i_c, i_u], 1)          # else [L, 2B, k]: the conditional half first
                assert torch.equal(idx, want), (mode, tag, w)
            else:
                want = torch.cat([i_c, i_u], 1)                                       # [L, 2B*T, k]
                same = (idx.sort(-1).values == want.sort(-1).values).all(-1)         # [L, 2B*T]
                agree = same.float().mean().item()
                ok = same.view(L_, 2, 5, T).all(3).all(1).all(0)                     # per sample: every decision of both branches
                print(f"guidance denoise {mode} {dtype} {tag} w={w}: agreement {agree:.4f}, samples with identical routing {int(ok.sum())}/5")
                assert agree >= 0.995, (mode, dtype, tag, w, agree)
                assert int(ok.sum()) * 2 >= 5, (mode, dtype, tag, w, ok)
                keep = ok
            err, b = nrm(got.cpu()[keep] - ref[keep]), bound(dtype, w, d_c[keep], d_u[keep])
            print(f"guidance denoise {mode} {dtype} {tag} w={w}: err {err:.3e} bound {b:.3e} (rel {err / max(nrm(ref[keep]), 1e-30):.2e})")
            assert err <= b, (mode, dtype, tag, w, err, b)


# ================================================================================================================== 3. fused samplers
SAMPLERS = {"ddim": (gc_sampling.sample_ddim, 1e-5), "dpmpp_2m": (samplers.sample_dpmpp_2m, 3e-6), "heun": (samplers.sample_heun, 1e-5)}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["noise", "goal", "token"])
def test_fused_samplers_equal_their_step_loops(mode, dtype):
    """The guided graph against the sampler's own step loop (forced by a callback), as tests/test_samplers.py compares the unguided ones, at its strictness:
    fp32 rounding of the rearranged update (ddim / heun 1e-5, dpmpp_2m 3e-6), bf16 the output tolerance - under token routing in bf16 the number
    tests/test_gpu_routing_graphed.py holds graph vs per-step to (near-tied tokens flip between the two paths' row geometries)."""
    cfg, sd, m, den = build(mode, dtype)
    den.guidance_scale = 2.5
    inp = inputs(cfg, 5, MODES[mode][0] + 2)
    st = {"state_images": inp["state_images"]}
    sig = gc_sampling.get_sigmas_exponential(10, 1e-3, 80.0, "cuda")
    plain = M.GCDenoiser(m, SIGMA_DATA).eval()
    for name, (fn, tol32) in SAMPLERS.items():
        loop = fn(den, st, inp["x0"], inp["goals"], sig, disable=True, callback=lambda d: None)
        fused = fn(den, st, inp["x0"], inp["goals"], sig, disable=True)
        r = rel(fused, loop)
        print(f"guidance sampler {mode} {dtype} {name}: graph vs step loop {r:.2e}")
        assert r < (tol32 if dtype == "fp32" else BF16_TOKROUTE_OUT if mode == "token" else BF16_OUT), (name, r)
        assert torch.equal(fused, fn(den, st, inp["x0"], inp["goals"], sig, disable=True)), name
        assert ("graph:" + name if name != "ddim" else "graph") + ":cfg" in m._route_cache
        assert rel(fused, fn(plain, st, inp["x0"], inp["goals"], sig, disable=True)) > 1e-2, name     # guidance changes the plan


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["noise", "goal", "token"])
def test_guided_ddim_vs_oracle_loop(mode, dtype):
    """10-step guided DDIM against the same loop on the oracle's two-call composition: rel < OUT_FUZZ[dtype] (|w| + |1 - w|).
    Token routing in fp32, the rule of test 2 over the whole chunk: >= 99.5 % of the decisions of all steps identical, the output compared on the samples
    whose every decision (both branches, every step, layer and token) agrees - samples do not interact - and at least half of the samples must qualify.
    Token routing in bf16: that rule cannot hold over a chunk for ANY implementation.  The reference's own fp32-vs-autocast agreement is 99.0-99.6 % per
    decision (tests/golden/bf16_tokroute_gap.json), a sample has 2 branches x 10 steps x 2 layers x 14 tokens = 560 decisions - all of them agree with
    probability 0.4-11 % -, and a flipped token changes the latent every later step routes on.  Measured here: w = 1: 99.75 % of the decisions, 1 sample
    of 5 with none flipped; w = 2.5: 98.96 %, 1 of 5.  This cell is therefore held to the suite's existing contract for exactly this quantity, a
    token-routed bf16 sampler result against the oracle loop (tests/test_gpu_routing_graphed.py): decisions >= BF16_TOKROUTE_AGREE, the whole output
    within BF16_TOKROUTE_OUT, pushed through the combine like the other cells."""
    cfg, sd, m, den = build(mode, dtype)
    B = 5
    inp = make_inputs(cfg, B, MODES[mode][0] + 2)
    sig = O.get_sigmas_exponential(10, 1e-3, 80.0)
    rec = []

    def oracle_den(w):
        def f(state, action, goal, sigma, **kw):
            d = [O.denoiser_forward(sd, cfg, SIGMA_DATA, state["state_images"], action, g_, sigma, return_aux=True) for g_ in (goal, torch.zeros_like(goal))]
            rec.append(torch.cat([torch.stack(aux.topk_idx).reshape(cfg.n_layers, -1, cfg.top_k) for _, aux in d], 1))   # token routing: [L, 2B*T, k]
            return combine(d[0][0], d[1][0], w)
        return f
    c = {k: v.cuda() for k, v in inp.items()}
    for w in (1.0, 2.5):
        rec.clear()
        ref = gc_sampling.sample_ddim(oracle_den(w), {"state_images": inp["state_images"]}, inp["x0"], inp["goals"], sig, disable=True)
        den.guidance_scale = w
        got = gc_sampling.sample_ddim(den, {"state_images": c["state_images"]}, c["x0"], c["goals"], sig.cuda(), disable=True).cpu()
        keep = slice(None)
        if mode == "token":
            want, idx = torch.stack(rec, 1).long(), m._last_topk.cpu().long()          # [L, n, 2B*T, k]
            same = (idx.sort(-1).values == want.sort(-1).values).all(-1)
            agree = same.float().mean().item()
            keep = same.view(cfg.n_layers, len(rec), 2, B, cfg.seq_len).permute(3, 0, 1, 2, 4).reshape(B, -1).all(1)
            print(f"guidance ddim vs oracle {mode} {dtype} w={w}: agreement {agree:.4f}, samples with identical routing {int(keep.sum())}/{B}")
            if dtype == "fp32":
                assert agree >= 0.995, (dtype, w, agree)
                assert int(keep.sum()) * 2 >= B, (dtype, w, keep)
            else:
                assert agree >= BF16_TOKROUTE_AGREE, (dtype, w, agree)
                keep = slice(None)
        tol = BF16_TOKROUTE_OUT if (mode, dtype) == ("token", "bf16") else OUT_FUZZ[dtype]
        r, b = rel(got[keep], ref[keep]), tol * (abs(w) + abs(1 - w))
        print(f"guidance ddim vs oracle {mode} {dtype} w={w}: rel {r:.3e} bound {b:.3e}")
        assert r < b, (mode, dtype, w, r, b)


# ================================================================================================================== 4. geometry switches
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 16, 17, 28])
def test_internal_batches_across_the_geometry_switches(B, dtype):
    """Internal batches 2, 32, 34, 56 (gemm_skinny_rows = 32, fuse_qkv_attn_min_b = 56) against two unguided denoise calls on the GPU."""
    cfg, sd, m, den = build("goal", dtype)
    inp = inputs(cfg, B, 77)
    st = {"state_images": inp["state_images"]}
    sig = torch.tensor([0.9], device="cuda")
    plain = M.GCDenoiser(m, SIGMA_DATA).eval()
    with torch.no_grad():
        d_c, d_u = plain(st, inp["actions"], inp["goals"], sig), plain(st, inp["actions"], torch.zeros_like(inp["goals"]), sig)
        for w in (2.5, -1.0):
            den.guidance_scale = w
            got = den(st, inp["actions"], inp["goals"], sig)
            err, b = nrm(got - combine(d_c, d_u, w)), bound(dtype, w, d_c, d_u)
            print(f"guidance geometry B={B} {dtype} w={w}: err {err:.3e} bound {b:.3e}")
            assert err <= b, (B, dtype, w, err, b)
            fast = den.denoise_uniform(st, inp["actions"], inp["goals"], sig)           # the graphed denoiser: the same chain, replayed
            assert fast is not None and nrm(fast - got) <= 1e-6 * nrm(got)


# ================================================================================================================== 5. scale changes, mode switches
def test_scale_changes_reuse_the_graph_and_none_restores_the_unguided_chain():
    cfg, sd, m, den = build("noise", "bf16")
    _, _, m0, den0 = build("noise", "bf16")                                           # a model that is never guided
    inp = inputs(cfg, 4, 5)
    st = {"state_images": inp["state_images"]}
    sig = gc_sampling.get_sigmas_exponential(10, 1e-3, 80.0, "cuda")
    s1 = torch.tensor(1.3, device="cuda")
    @torch.no_grad()
    def run(d):
        return (gc_sampling.sample_ddim(d, st, inp["x0"], inp["goals"], sig, disable=True), samplers.sample_heun(d, st, inp["x0"], inp["goals"], sig, disable=True),
                d.denoise_uniform(st, inp["actions"], inp["goals"], s1))
    base = run(den0)
    assert all(torch.equal(a, b) for a, b in zip(run(den), base))
    den.guidance_scale = 2.0
    g2 = run(den)
    ent, graph = m._route_cache["graph:cfg"], m._route_cache["graph:cfg"]["graph"]
    den.guidance_scale = 3.0
    g3 = run(den)
    assert m._route_cache["graph:cfg"] is ent and ent["graph"] is graph                # same entry, same graph object: the scale is a device scalar
    with torch.no_grad():
        plain = M.GCDenoiser(m0, SIGMA_DATA).eval()
        d_c, d_u = plain(st, inp["actions"], inp["goals"], s1.reshape(1)), plain(st, inp["actions"], torch.zeros_like(inp["goals"]), s1.reshape(1))
    for w, out in ((2.0, g2), (3.0, g3)):
        assert nrm(out[2] - combine(d_c, d_u, w)) <= bound("bf16", w, d_c, d_u), w     # the results follow the new value
    assert rel(g2[0], g3[0]) > 1e-3 and rel(g2[1], g3[1]) > 1e-3
    sizes = None
    for i in range(20):                                                                 # alternate guided / unguided: never the wrong chain, no new graphs
        den.guidance_scale = None if i % 2 == 0 else 2.0
        out = run(den)
        assert all(torch.equal(a, b) for a, b in zip(out, base if i % 2 == 0 else g2)), i
        now = (len(m._route_cache), len(m._route_cache["denoise_graphs"]))
        assert sizes is None or now == sizes, (i, now, sizes)
        sizes = now
    assert m._route_cache["graph:cfg"]["graph"] is graph


# ================================================================================================================== 6. rollout policies
def policy(den, cfg, n, **kw):
    return rollout.VectorEnvPolicy(den, n, act_window_size=cfg.action_seq_len, action_dim=cfg.action_dim, sigma_max=80.0, **kw)


def usage(m):
    m.sync_expert_usage()
    return torch.stack([blk.get_expert_usage().clone() for blk in m.blocks]), [blk.total_tokens_processed for blk in m.blocks]


@pytest.mark.parametrize("mode,ensemble", [("noise", None), ("goal", None), ("token", None), ("noise", 0.1)])
def test_vector_env_policy_plans_guided(mode, ensemble):
    """3 environments replanning at different steps: the plans are the guided fused sampler's on env_noise latents, bit for bit (as
    tests/test_gpu_vector_env.py compares the unguided ones); the usage counters count both branches of the REAL rows."""
    cfg, sd, m, den = build(mode, "bf16")
    den.guidance_scale = 2.5
    n = 3
    kw = dict(multistep=4, temporal_ensemble=ensemble) if ensemble is not None else {}
    pol = policy(den, cfg, n, **kw)
    g = torch.Generator().manual_seed(3)
    img, goal = torch.randn(n, 2, cfg.obs_dim, generator=g).cuda(), torch.randn(n, cfg.goal_dim, generator=g).cuda()
    seeds = [21, 22, 23]
    pol.reset(seeds=seeds)
    for step, envs in enumerate(([0, 1, 2], [1], [0, 2])):                           # m = 3 (bucket 4: one padded row), 1, 2
        act = np.zeros(n, dtype=bool); act[envs] = True
        pol.reset(envs=envs)
        draws = pol.draws.cpu().tolist()
        m.sync_expert_usage()
        for blk in m.blocks:
            blk.reset_expert_usage()
        pol.step({"state_images": img}, goal, active=act)
        got_use, got_tok = usage(m)
        assert pol.replanned == envs
        mb = next(b for b in (1, 2, 4) if b >= len(envs))
        rows = envs + [envs[-1]] * (mb - len(envs))
        x0 = rollout.env_noise([seeds[r] for r in rows], [draws[r] for r in rows], cfg.action_seq_len, cfg.action_dim, 80.0, "cuda")
        ref = gc_sampling.sample_ddim(den, {"state_images": img[rows].contiguous()}, x0, goal[rows].contiguous(), pol._schedule(img.device), disable=True)
        assert torch.equal(pol.plans[envs], ref[:len(envs)]), (mode, step)
        tokens = 2 * len(envs) * cfg.seq_len * 10                                     # both branches, 10 evaluations
        assert got_tok == [tokens] * cfg.n_layers and float(got_use.sum()) == tokens * cfg.top_k * cfg.n_layers, (mode, step, got_tok, tokens)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("sampler", ["ddim", "euler_ancestral"])
def test_chunked_rollout_policy_guided(B, sampler, dtype, monkeypatch):
    """ChunkedRolloutPolicy reads the denoiser's scale.  Internal batches 2 and 6: in bf16 the two sides of the skinny switch (2·14 = 28 token rows take the
    small-batch weight-streaming chain, 84 the tiled one); fp32 has the tiled chain only.  The plan is the per-step path's (MODE_HIP_GRAPH=0) from the
    same noise - DDIM through the fused chunk, euler_ancestral through the policy's whole-call graph, with eta = 0 so that the sampler's in-loop
    noise (the capture's own draws) has weight zero and the two paths are comparable.  Every denoiser call ran both branches: 2·B·T tokens per call."""
    import functools
    cfg, sd, m, den = build("goal", dtype)
    den.guidance_scale = 2.5
    monkeypatch.setattr(rollout.gs, "sample_euler_ancestral", functools.partial(samplers.sample_euler_ancestral, eta=0.0))
    inp = inputs(cfg, B, 71)
    obs, goal = {"state_images": inp["state_images"]}, inp["goals"].squeeze(1)
    mk = lambda d: rollout.ChunkedRolloutPolicy(d, sampler_type=sampler, multistep=4, generator=torch.Generator(device="cuda").manual_seed(9))
    m.sync_expert_usage()
    for blk in m.blocks:
        blk.reset_expert_usage()
    plan = mk(den).denoise_actions(obs, goal)
    got_use, got_tok = usage(m)
    assert got_tok == [2 * B * cfg.seq_len * 10] * cfg.n_layers and float(got_use.sum()) == 2 * B * cfg.seq_len * 10 * cfg.top_k * cfg.n_layers
    unguided = mk(M.GCDenoiser(m, SIGMA_DATA).eval()).denoise_actions(obs, goal)
    assert torch.isfinite(plan).all() and rel(plan, unguided) > 1e-2
    monkeypatch.setenv("MODE_HIP_GRAPH", "0")
    ref = mk(den).denoise_actions(obs, goal)
    monkeypatch.delenv("MODE_HIP_GRAPH")
    r = rel(plan, ref)
    print(f"guidance rollout {sampler} B={B} {dtype}: graph vs per-step {r:.2e}")
    assert r < (1e-5 if dtype == "fp32" else BF16_OUT), r
    a = mk(den).step(obs, goal)
    assert a.shape == (B, cfg.action_dim) and torch.isfinite(a).all()


# ================================================================================================================== 7. errors before any launch
def test_refusals_before_any_launch():
    cfg, sd, m, den = build("noise", "bf16")
    inp = inputs(cfg, 2, 9)
    st, sig = {"state_images": inp["state_images"]}, torch.tensor([0.9], device="cuda")
    den.guidance_scale = 2.0
    m.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            den(st, inp["actions"], inp["goals"], sig)
        den.loss(st, inp["actions"], inp["goals"], inp["noise"], sig.expand(2))       # loss ignores the scale
    finally:
        m.eval()
    for over, what in ((dict(top_k=3), "top_k"), (dict(embed_dim=4352, n_heads=34, n_layers=1, num_experts=1, top_k=1), "embed_dim")):
        with torch.device("meta"):
            big = M.MoDeDiT(obs_dim=8, goal_dim=8, device="cuda", goal_conditioned=True, action_dim=7, embed_pdrob=0, attn_pdrop=0.0, goal_seq_len=1, obs_seq_len=1,
                            action_seq_len=10, **{**dict(embed_dim=256, n_layers=1, n_heads=2, num_experts=4, top_k=2), **over}).eval()
        gd = M.GCDenoiser(big, SIGMA_DATA, guidance_scale=2.0).eval()
        for call in (lambda: gd(st, inp["actions"], inp["goals"], sig), lambda: gc_sampling.sample_ddim(gd, st, inp["x0"], inp["goals"], torch.tensor([1.0, 0.5, 0.0]))):
            with pytest.raises(ValueError, match=what):
                call()
    # the C entry point refuses the same shapes itself
    lib = L.load()
    dims = L.ModeDims(D=256, H=2, L=1, E=4, k=3, T=14, A_len=10, A_dim=7, O=8, G=8, n_img=2, use_noise_token=1, router_normalize=1, eps=1e-6)
    lw = (L.ModeLayerWeights * 1)()
    mw = L.ModeModelWeights(layers=C.cast(lw, C.POINTER(L.ModeLayerWeights)))
    ga = L.ModeGuidedArgs(fwd=L.ModeForwardArgs(B=1, dtype=L.MODE_BF16, goal_e=16, img_e=16, actions=16, cond=16, scal=16, denoised=16), scale=16)
    assert lib.mode_dit_forward_guided(C.byref(dims), C.byref(mw), C.byref(ga), 16, 1 << 30, None) == -2      # k = 3: MODE_ERR_UNSUPPORTED
