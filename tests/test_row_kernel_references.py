"""The fp64 restatements of tests/row_refs.py, validated without a GPU against what already exists: the oracle's rmsnorm, per-expert combine loop,
sequence assembly, model forward and EDM scalings, torch autograd of the oracle's own sequence assembly, and finite differences.  A mismatch between
a HIP kernel and row_refs on the GPU is then the kernel's, not the reference's.  The last test turns each reference wrong the way the GPU tests'
sensitivity checks do, and requires the difference to be far outside the GPU tests' bounds."""
import dataclasses

import pytest
import torch

from oracle import mode_oracle as O
from oracle.weights import get_config, make_inputs, make_state_dict

import row_refs as R
from row_refs import rel


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def routed(N, E, k, seed):
    """idx / w of a random top-k routing, the oracle's dispatch permutation, and (pos, posw) as mode_moe_dispatch_meta defines them."""
    probs = torch.rand(N, E, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    idx = torch.sort(probs, dim=-1, descending=True, stable=True).indices[:, :k].contiguous()
    w = probs.gather(1, idx); w = w / w.sum(-1, keepdim=True)
    counts, perm, slot = O.dispatch_permutation(idx, E)
    pos, posw, fill = torch.zeros(N, k, dtype=torch.int32), torch.zeros(N, k, dtype=torch.float64), [0] * N
    for s in range(N * k):                                  # sorted rows are in ascending expert id: a token meets its experts in that order
        t = int(perm[s])
        pos[t, fill[t]], posw[t, fill[t]] = s, w[t, slot[s]]
        fill[t] += 1
    return idx, w, counts, perm, slot, pos, posw


def expert_loop(u, Y, w, counts, perm, slot):
    """x + next_states of the oracle's per-expert loop (mode_oracle.dit_forward; tests/test_gpu_kernels.py::test_grouped_gather_gemm)."""
    nxt, off = torch.zeros_like(u), 0
    for e in range(len(counts)):
        n = int(counts[e]); rows = perm[off: off + n]; sl = slot[off: off + n]
        nxt[rows] += w[rows, sl].unsqueeze(-1) * Y[off: off + n]
        off += n
    return u + nxt


@pytest.mark.parametrize("N,E,k,D,S", [(9, 4, 2, 68, 1), (21, 8, 3, 256, 2), (9, 8, 8, 64, 3), (5, 2, 1, 1284, 9)])
def test_combine_reference_is_the_oracles_expert_loop(N, E, k, D, S):
    idx, w, counts, perm, slot, pos, posw = routed(N, E, k, seed=N + k)
    u, Y = rnd(N, D, seed=1), rnd(S, N * k, D, seed=2, scale=0.5)
    gain, cond, rpc = 1 + 0.1 * rnd(D, seed=3), rnd(3, D, seed=4), (N + 2) // 3
    x, h = R.combine(u, Y, pos, posw, gain, cond, rpc)
    xref = expert_loop(u, Y.sum(0), w, counts, perm, slot)
    assert rel(x, xref) < 1e-14
    assert rel(h, O.rmsnorm(xref, gain) + cond[torch.arange(N) // rpc]) < 1e-14
    x_only, none = R.combine(u, Y, pos, posw)
    assert none is None and torch.equal(x_only, x)


@pytest.mark.parametrize("D,nss", [(256, 16), (272, 17), (1280, 20), (3076, 769), (1284, 107)])
def test_fused_ln2_reference_is_the_unfused_one_on_normalised_u(D, nss):
    """u with its partial sums of squares and the ln_2 gain == the oracle's rmsnorm(u, gain) fed as an already normalised u; the partials are rounded to
    fp32 as the producer GEMM publishes them, hence 1e-7 and not 1e-14."""
    N, k = 9, 2
    _, _, _, _, _, pos, posw = routed(N, 4, k, seed=D)
    u, Y, g2, g = rnd(N, D, seed=1).float(), rnd(2, N * k, D, seed=2), 1 + 0.2 * rnd(D, seed=3), 1 + 0.1 * rnd(D, seed=4)
    fused = R.combine(u, Y, pos, posw, g, u_ss=R.partial_ss(u, nss), u_gain=g2)
    plain = R.combine(O.rmsnorm(u.double(), g2), Y, pos, posw, g)
    assert rel(fused[0], plain[0]) < 1e-7 and rel(fused[1], plain[1]) < 1e-7
    assert rel(fused[0], R.combine(u, Y, pos, posw, g)[0]) > 1e-2            # and it is not the un-normalised one


def one_block():
    cfg = dataclasses.replace(get_config("tiny"), n_layers=1)
    sd = {k: v.double() for k, v in make_state_dict(cfg, 5).items()}
    return cfg, sd, {k: v.double() for k, v in make_inputs(cfg, 3, 6).items()}


def test_embed_reference_is_the_oracles_sequence_assembly():
    cfg, sd, inp = one_block()
    B, D = 3, cfg.embed_dim
    emb_t, g, cond = rnd(B, D, seed=1), 1 + 0.1 * rnd(D, seed=2), rnd(B, D, seed=3)
    c_in = 0.1 + rnd(B, seed=4).abs()
    goal_e = inp["goals"].reshape(B, -1) @ sd["goal_emb.weight"].t()
    img_e = inp["state_images"] @ sd["tok_emb.weight"].t()
    want = O.embed_sequence(sd, cfg, inp["state_images"], inp["actions"] * c_in[:, None, None], inp["goals"], emb_t)
    x, h = R.embed(goal_e, img_e, inp["actions"], sd["action_emb.weight"], sd["pos_emb"][0], g, emb_t=emb_t, c_in=c_in, cond=cond)
    assert x.shape == want.shape and rel(x, want) < 1e-14
    assert rel(h, O.rmsnorm(want, g) + cond[:, None]) < 1e-14
    # without the sigma token, shared rows
    cfg0 = dataclasses.replace(cfg, use_noise_token_as_input=False)
    want0 = O.embed_sequence(sd, cfg0, inp["state_images"], inp["actions"], inp["goals"], emb_t)
    x0, h0 = R.embed(goal_e, img_e, inp["actions"], sd["action_emb.weight"], sd["pos_emb"][0], g, cond=cond[:1])
    assert x0.shape == want0.shape and rel(x0, want0) < 1e-14 and rel(h0, O.rmsnorm(want0, g) + cond[0]) < 1e-14
    assert rel(R.rmsnorm_cond(want.reshape(-1, D), g, cond, cfg.seq_len), h.reshape(-1, D)) < 1e-14


def test_head_reference_is_the_oracles_model_tail_and_ddim_update():
    """One-block model: the oracle's last block output fed as u (k = 1, a zero expert row) must give the oracle's network output, its denoiser output and
    its DDIM update; then the den_prev and lin updates element by element from the header's formulas."""
    cfg, sd, inp = one_block()
    B, T, D, A_len, A_dim = 3, cfg.seq_len, cfg.embed_dim, cfg.action_seq_len, cfg.action_dim
    sigma, sigma_next = torch.tensor([0.9, 0.02, 30.0], dtype=torch.float64), torch.tensor([0.5, 0.0, 11.0], dtype=torch.float64)
    c_skip, c_out, c_in = O.edm_scalings(sigma, 0.5)
    out, aux = O.dit_forward(sd, cfg, inp["state_images"], inp["actions"] * c_in[:, None, None], inp["goals"], sigma, return_aux=True)
    den = O.denoiser_forward(sd, cfg, 0.5, inp["state_images"], inp["actions"], inp["goals"], sigma)
    u = aux.block_out[-1].reshape(B * T, D)
    Y, pos, posw = torch.zeros(1, B * T, D), torch.arange(B * T, dtype=torch.int32)[:, None], torch.ones(B * T, 1)
    scal = torch.stack([c_skip, c_out, sigma_next / sigma, torch.tensor([0.35, 0.0, 1.5], dtype=torch.float64)], 1)
    args = (u, Y, pos, posw, sd["ln.g"], sd["out.weight"], sd["out.bias"], B, T, A_len)
    Fh, dn, xn = R.head(*args, x_a=inp["actions"], scal=scal)
    assert rel(Fh, out) < 1e-13 and rel(dn, den) < 1e-13
    want = torch.stack([O.ddim_update(inp["actions"][b], den[b], float(sigma[b]), float(sigma_next[b])) for b in range(B)])
    assert rel(xn, want) < 1e-13
    assert R.head(*args)[1:] == (None, None) and rel(R.head(*args)[0], out) < 1e-13
    sd_, sx = R.ddim_edm_step(out.reshape(B, -1), inp["actions"].reshape(B, -1), scal)
    assert rel(sd_, den.reshape(B, -1)) < 1e-13 and rel(sx, want.reshape(B, -1)) < 1e-13
    prev, a1, a2, lin = rnd(B, A_len, A_dim, seed=1), rnd(B, A_len, A_dim, seed=2), rnd(B, A_len, A_dim, seed=3), torch.tensor([0.3, -0.7, 1.2, 0.5])
    _, _, xp = R.head(*args, x_a=inp["actions"], scal=scal, den_prev=prev)
    _, _, xl = R.head(*args, x_a=inp["actions"], scal=scal, lin=lin, aux1=a1, aux2=a2)
    for b in range(B):
        c, r = float(scal[b, 3]), float(scal[b, 2])
        dd = den[b] if c == 0 else (1 + c) * den[b] - c * prev[b]
        assert rel(xp[b], r * inp["actions"][b] + (1 - r) * dd) < 1e-13
        assert rel(xl[b], 0.3 * inp["actions"][b] - 0.7 * den[b] + 1.2 * a1[b] + 0.5 * a2[b]) < 1e-6      # (lin is fp32: 0.3f != 0.3)
    assert torch.equal(xp[1], xn[1]) and rel(xp[0], xn[0]) > 1e-2                    # c == 0 is the DDIM update; c != 0 is not


def test_small_forward_references_are_the_oracles():
    cfg, sd, inp = one_block()
    sigma = torch.tensor([1e-3, 0.7, 80.0], dtype=torch.float64)
    sd1 = dict(sd); sd1["sigma_linear.weight"] = torch.eye(cfg.embed_dim, dtype=torch.float64)
    assert rel(R.sigma_embed(sigma, sd["sigma_emb.weight"], sd["sigma_emb.bias"]), O.sigma_embedding(sd1, sigma)) < 1e-14
    c_skip, c_out, c_in = (t[:, None] for t in O.edm_scalings(sigma, 0.5))
    a, n, Fh = inp["actions"].flatten(1), inp["noise"].flatten(1), rnd(3, inp["actions"][0].numel(), seed=1)
    assert rel(R.edm_noise_scale(a, n, sigma, 0.5), (a + n * sigma[:, None]) * c_in) < 1e-14
    loss, dF, terms = R.edm_loss(Fh, a, n, sigma, 0.5)
    target = (a - c_skip * (a + n * sigma[:, None])) / c_out
    assert rel(loss, (Fh - target).pow(2).flatten(1).mean()) < 1e-14 and rel(terms.sum(), loss) < 1e-14
    assert rel(dF, 2 * (Fh - target) / Fh.numel()) < 1e-13


@pytest.mark.parametrize("noise_token", [True, False])
def test_pos_emb_reference_is_autograd_of_the_oracles_sequence_assembly(noise_token):
    cfg, sd, inp = one_block()
    cfg = dataclasses.replace(cfg, use_noise_token_as_input=noise_token)
    sd = dict(sd); sd["pos_emb"] = sd["pos_emb"].clone().requires_grad_(True)
    x = O.embed_sequence(sd, cfg, inp["state_images"], inp["actions"], inp["goals"], rnd(3, cfg.embed_dim, seed=1))
    dx0 = rnd(*x.shape, seed=2)
    (x * dx0).sum().backward()
    dpos, mag = R.pos_emb_bwd(dx0, int(noise_token), cfg.n_img_tokens, cfg.action_seq_len)
    assert rel(dpos, sd["pos_emb"].grad[0]) < 1e-14
    assert bool((mag >= dpos.abs() - 1e-12).all())


def test_sigma_embed_bwd_and_gelu_references():
    de1, sigma = rnd(5, 12, seed=1), torch.tensor([1e-3, 0.2, 1.0, 9.0, 80.0], dtype=torch.float64)
    dw, db, mw, mb = R.sigma_embed_bwd(de1, sigma)
    assert rel(dw, (de1 * sigma.log()[:, None] / 4).sum(0)) < 1e-14 and rel(db, de1.sum(0)) < 1e-14 and bool((mw >= dw.abs() - 1e-12).all())
    x, dout = torch.linspace(-6, 6, 41, dtype=torch.float64), rnd(41, seed=2)
    y, dx = R.gelu(x, dout)
    cdf = 0.5 * (1 + torch.erf(x / 2 ** 0.5))
    assert rel(y, x * cdf) < 1e-14 and rel(dx, dout * (cdf + x * torch.exp(-x * x / 2) / (2 * torch.pi) ** 0.5)) < 1e-13


@pytest.mark.parametrize("E,k", [(4, 2), (3, 3), (8, 3), (16, 8), (40, 5)])
@pytest.mark.parametrize("normalize", [0, 1])
def test_router_backward_reference_against_finite_differences(E, k, normalize):
    """Autograd of softmax -> clamp -> gather -> renormalisation (+ load balancing + z-loss through the max shift) against central differences in fp64,
    away from the clamp and from ties (where the function has a kink and a difference quotient means nothing)."""
    B, T, gen = 4, 3, torch.Generator().manual_seed(E + k)
    logits = rnd(B, E, seed=E, scale=1.5)
    idx = torch.rand(B, T, E, generator=gen).argsort(-1)[..., :k].int()            # unsorted, distinct per row
    dw, lb, zc = rnd(B * T, k, seed=2), rnd(2, E, seed=3, scale=0.1), 0.37
    for aux in ({}, dict(lb_coef=lb, rows_per_layer=2), dict(z_coef=zc), dict(lb_coef=lb, z_coef=zc, rows_per_layer=2)):
        got = R.router_bwd(logits, dw, idx, normalize, T, **aux)
        fd, hstep = torch.zeros_like(logits), 1e-6
        for b in range(B):
            for e in range(E):
                lp, lm = logits.clone(), logits.clone()
                lp[b, e] += hstep; lm[b, e] -= hstep
                fd[b, e] = (R.router_loss(lp, dw, idx, normalize, T, **aux) - R.router_loss(lm, dw, idx, normalize, T, **aux)) / (2 * hstep)
        assert rel(got, fd) < 1e-7, (aux.keys(), rel(got, fd))


def test_router_reference_clamp_and_tie():
    logits = torch.tensor([[40.0, 0.0, -1.0, 0.5], [1.0, 1.0, 0.2, -0.3]], dtype=torch.float64)
    idx, dw = torch.tensor([[[2, 0]], [[1, 3]]], dtype=torch.int32), rnd(2, 2, seed=1)
    g = R.router_bwd(logits, dw, idx, 1, 1)
    assert bool((g[0] == 0).all()) and float(g[1].abs().sum()) > 0                   # the clamp at 1 - 1e-9 (and at 1e-9) passes no gradient
    gz = R.router_bwd(logits, dw, idx, 0, 1, z_coef=1.0) - R.router_bwd(logits, dw, idx, 0, 1)
    assert abs(float(gz[1].sum())) < 1e-15 and gz[1, 0] < 0 < gz[1, 1]               # the FIRST of the tied maxima carries the shift's gradient


def test_wrong_references_are_far_outside_the_gpu_bounds():
    """The three perturbations the GPU tests hold their kernels against: a dropped last slab, the weights of two expert slots swapped, an off-by-one in
    the pos_emb row map.  Each moves the reference by orders of magnitude more than the bounds (1e-6 / 1e-5), so a kernel with that bug fails."""
    N, D, k = 9, 256, 2
    _, _, _, _, _, pos, posw = routed(N, 4, k, seed=1)
    u, Y = rnd(N, D, seed=1), rnd(3, N * k, D, seed=2, scale=0.5)
    x, _ = R.combine(u, Y, pos, posw)
    assert rel(R.combine(u, Y[:-1], pos, posw)[0], x) > 1e-2
    assert rel(R.combine(u, Y, pos, posw.flip(1))[0], x) > 1e-2
    dx0 = rnd(5, 14, 8, seed=3)
    good, mag = R.pos_emb_bwd(dx0, 1, 2, 10)
    bad, _ = R.pos_emb_bwd(dx0, 1, 2, 10, shift=1)
    assert bool(((good - bad).abs() > 1e-3 * mag)[1:].any(1).all())                  # every row but the goal's moves
