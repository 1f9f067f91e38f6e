"""GPU: LoraAdapter on the smallest model the GPU tests use (width 128, 2 layers, 4 experts, top-2, B = 3): attach / merge / detach on the shadow,
the adapted forward and sampler against a twin whose master holds the folded weights, the projected gradients of every layer, expert and target
against the twin's dense gradients, training with FlatAdamW, the hot swap under a captured rollout graph, the refused combinations."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import lora_refs as R  # noqa: E402
import mode_diffusion_policy_amd as M  # noqa: E402
from gemm_refs import half_ulp_bf16  # noqa: E402
from mode_diffusion_policy_amd import gc_sampling, rollout  # noqa: E402
from mode_diffusion_policy_amd.lora import LoraAdapter, target_shapes  # noqa: E402
from mode_diffusion_policy_amd.optim import ArenaEMA, FlatAdamW, FusedAdamW  # noqa: E402
from oracle import mode_oracle as O  # noqa: E402
from oracle.weights import make_inputs, make_state_dict  # noqa: E402
from tolerances import BF16_GRAD, BF16_OUT  # noqa: E402

CFG = O.DiTConfig(obs_dim=64, goal_dim=32, action_dim=7, embed_dim=128, n_layers=2, n_heads=4, action_seq_len=10, num_experts=4, top_k=2)
B_ = 3
RANK, ALPHA = 8, 12.0                                                              # s = 1.5


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


def rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def build(seed=21, dtype="bf16", train=False):
    cfg = CFG
    m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cuda", goal_conditioned=True, action_dim=7, embed_dim=cfg.embed_dim, embed_pdrob=0,
                  attn_pdrop=0.0, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1, obs_seq_len=1, action_seq_len=10, mlp_pdrop=0.0, goal_drop=0.0,
                  num_experts=cfg.num_experts, top_k=cfg.top_k, use_argmax=True, compute_dtype=dtype)
    m.load_state_dict(make_state_dict(cfg, seed))
    m = m.to("cuda")
    return m.train() if train else m.eval()


def inputs(seed=5):
    return {k: v.cuda() for k, v in make_inputs(CFG, B_, seed).items()}


def random_adapter(m, seed, rank=RANK, alpha=ALPHA, **kw):
    """An adapter whose A AND B are random, different for every layer and expert."""
    ad = LoraAdapter(m, rank=rank, alpha=alpha, seed=seed, **kw)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for _, _, b in ad.pairs():
            b.copy_((torch.randn(b.shape, generator=g) * 0.02).cuda())
    return ad


def folded_twin(ad, seed=21, train=False):
    """A second model whose fp32 master holds W + s B A, formed by torch in fp32 (no kernel of this feature involved)."""
    t = build(seed, train=train)
    ar = t.engine.arena
    with torch.no_grad():
        for tg, a, b in ad.pairs():
            for i in range(t.num_layers):
                ar.w[f"l{i}.{tg}"].add_((ad.scale * (b[i] @ a[i])).view(ar.w[f"l{i}.{tg}"].shape))
    t.engine.weights_updated(lp_synced=False)
    return t


def forward(m, inp, sigma=0.7):
    with torch.no_grad():
        return m({"state_images": inp["state_images"]}, inp["actions"], inp["goals"], torch.full((B_,), sigma, device="cuda"))


def sample(m, inp):
    den = M.GCDenoiser(m, 0.5).eval()
    sig = gc_sampling.get_sigmas_exponential(10, 1e-3, 80.0, "cuda")
    with torch.no_grad():
        return gc_sampling.sample_ddim(den, {"state_images": inp["state_images"]}, inp["x0"], inp["goals"], sig, disable=True)


def test_fresh_adapter_is_the_identity_and_detach_restores_everything():
    m, inp = build(), inputs()
    m.freeze_router()
    flags = [p.requires_grad for p in m.parameters()]
    base_out = forward(m, inp)
    ar = m.engine.arena
    lp0, flat0 = bits(ar.lp), bits(ar.flat)
    ad = LoraAdapter(m, rank=RANK, seed=1).attach()                               # B = 0
    assert m.engine.arena is ar and torch.equal(bits(ar.lp), lp0) and torch.equal(bits(forward(m, inp)), bits(base_out))
    with torch.no_grad():
        ad.B_w1.normal_(0, 0.02)                                                   # bumps the parameter's version: the next engine access re-merges
    assert not torch.equal(bits(m.engine.arena.lp), lp0) and rel(forward(m, inp), base_out) > 1e-3
    ad.alpha = 0.0                                                                 # the scale alone (no parameter touched) re-merges as well
    assert torch.equal(bits(m.engine.arena.lp), lp0)
    ad.alpha = float(RANK)
    assert not torch.equal(bits(m.engine.arena.lp), lp0)
    ad.detach()
    assert getattr(m, "_lora", None) is None and [p.requires_grad for p in m.parameters()] == flags
    assert torch.equal(bits(m.engine.arena.lp), lp0) and torch.equal(bits(ar.flat), flat0) and torch.equal(bits(forward(m, inp)), bits(base_out))


def test_merged_shadow_forward_and_sampler_match_the_folded_twin():
    m, inp = build(), inputs()
    plain = bits(m.engine.arena.lp)
    ad = random_adapter(m, 2, targets=("wqkv", "w1", "w2")).attach()               # wo is NOT targeted
    ar = m.engine.arena
    total = differing = 0
    for tg, a, b in ad.pairs():
        for i in range(m.num_layers):
            key = f"l{i}.{tg}"
            acc = torch.zeros(b[i].shape[0], b[i].shape[1], a[i].shape[2], device="cuda")
            for k in range(ad.rank):                                               # the stated order, one fp32 tensor operation per rounding
                acc = acc + b[i][:, :, k:k + 1].detach() * a[i][:, k:k + 1, :].detach()
            want = (ar.w[key].detach() + (ad.scale * acc).view(ar.w[key].shape)).bfloat16()
            got = ar.wl[key]
            ulp = 2 * half_ulp_bf16(want.double().cpu())
            assert bool(((got.double().cpu() - want.double().cpu()).abs() <= ulp).all()), key     # within one bf16 ulp of torch's fp32 expression
            total += got.numel(); differing += int((bits(got) != bits(want)).sum())
    print(f"merged shadow vs torch fp32 W + s B A rounded to bf16: {differing} of {total} elements differ (by one ulp)")
    # every element that belongs to no targeted tensor keeps the bits of the plain cast
    mask = torch.ones(ar.lp.numel(), dtype=torch.bool)
    for key, shp, off in ar.layout:
        if key.split(".")[-1] in ad.targets and key.startswith("l"):
            mask[off: off + int(torch.Size(shp).numel())] = False
    assert torch.equal(bits(ar.lp)[mask], plain[mask]) and not torch.equal(bits(ar.lp)[~mask], plain[~mask])
    twin = folded_twin(ad)
    e_f, e_s = rel(forward(m, inp), forward(twin, inp)), rel(sample(m, inp), sample(twin, inp))
    print(f"adapted vs folded twin: forward rel-L2 {e_f:.2e}, 10-step DDIM rel-L2 {e_s:.2e} (tol {BF16_OUT})")
    assert e_f <= BF16_OUT and e_s <= BF16_OUT
    assert rel(forward(m, inp), forward(build(), inp)) > 10 * BF16_OUT             # the adapter does change the model


def _loss_backward(m, inp, seed):
    den = M.GCDenoiser(m, 0.5).train()
    torch.manual_seed(seed)                                                        # the same step seed (model._last_seed) on both models
    loss, _ = den.loss({"state_images": inp["state_images"]}, inp["actions"], inp["goals"], inp["noise"], torch.full((B_,), 0.9, device="cuda"))
    loss.backward()
    return loss.detach()


def _dense_grads(twin):
    """{(layer, target): dW [G, rows, cols]} of the twin from its parameters' .grad, BY PARAMETER NAME (the reference's names)."""
    g = {n: p.grad for n, p in twin.named_parameters()}
    out = {}
    for i in range(twin.num_layers):
        p = f"blocks.{i}."
        out[i, "wqkv"] = torch.cat([g[p + f"attn.{n}.weight"] for n in ("query", "key", "value")])[None]
        out[i, "wo"] = g[p + "attn.c_proj.weight"][None]
        out[i, "w1"] = torch.stack([g[p + f"experts.expert_{e}.mlp.0.project.weight"] for e in range(twin.num_experts)])
        out[i, "w2"] = torch.stack([g[p + f"experts.expert_{e}.mlp.2.weight"] for e in range(twin.num_experts)])
    return out


def test_projected_gradients_match_the_folded_twins_dense_gradients():
    m, inp = build(train=True), inputs()
    ad = random_adapter(m, 3).attach()
    twin = folded_twin(ad, train=True)
    la = _loss_backward(m, inp, 77)
    lt = _loss_backward(twin, inp, 77)
    torch.cuda.synchronize()
    assert m._last_seed == twin._last_seed and abs(float(la.detach()) - float(lt.detach())) <= 1e-2 * abs(float(lt.detach()))
    assert all(p.grad is None for p in m.parameters())                             # the base receives nothing
    dense = _dense_grads(twin)
    s32 = float(torch.tensor(ad.scale, dtype=torch.float32))
    worst, live = (0.0, None), 0
    for tg, a, b in ad.pairs():
        G, rows, cols = target_shapes(m)[tg]
        assert a.grad is not None and b.grad is not None and tuple(a.grad.shape) == tuple(a.shape) and tuple(b.grad.shape) == tuple(b.shape)
        for i in range(m.num_layers):
            (rA, rB), (bA, bB) = R.grad_ref(dense[i, tg].reshape(G, rows, cols), a[i], b[i], s32)
            for e in range(G):
                for name, got, ref, bound in (("dA", a.grad[i, e], rA[e], bA[e]), ("dB", b.grad[i, e], rB[e], bB[e])):
                    err = float((got.double().cpu() - ref).norm())
                    # the projection's own bound plus BF16_GRAD on the dense gradient the two models computed separately
                    lim = float(bound.norm()) + BF16_GRAD * float(ref.norm())
                    assert err <= lim, (tg, i, e, name, err, lim)                  # (an expert no token was routed to: both exactly zero)
                    live += float(ref.norm()) > 0
                    q = err / max(float(ref.norm()), 1e-300)
                    if q > worst[0]:
                        worst = (q, (tg, i, e, name))
    assert live >= 24                                                              # per layer: dA and dB of wqkv, wo and of at least two experts of w1 and w2
    print(f"projected gradients vs fp64 projection of the twin's dense gradients: worst rel-L2 {worst[0]:.2e} at {worst[1]} (tol {BF16_GRAD})")
    # a second backward before the optimizer step accumulates, as autograd does
    first = [p.grad.clone() for p in ad.parameters()]
    _loss_backward(m, inp, 77)
    for p, f in zip(ad.parameters(), first):
        assert rel(p.grad, 2 * f) <= 1e-6


def test_five_flat_adamw_steps_train_the_adapter_and_leave_the_base_alone():
    m, inp = build(train=True), inputs()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    ad = LoraAdapter(m, rank=RANK, seed=4).attach()
    flat0 = bits(m.engine.arena.flat)
    opt = FlatAdamW(ad.parameters(), lr=2e-3, weight_decay=0.0)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        losses.append(float(_loss_backward(m, inp, 78)))
        opt.step()
    losses.append(float(_loss_backward(m, inp, 78)))
    opt.zero_grad()
    print("adapter-only training, loss per step:", " ".join(f"{v:.5f}" for v in losses))
    assert losses[-1] < losses[0] and all(p.grad is None for p in m.parameters())
    assert torch.equal(bits(m.engine.arena.flat), flat0)
    assert all(torch.equal(bits(v), bits(sd0[k])) for k, v in m.state_dict().items()) and list(m.state_dict()) == list(sd0)
    assert all(float(b.detach().abs().max()) > 0 for _, _, b in ad.pairs())
    # fold() into a copy reproduces the attached model
    m.eval()
    out = forward(m, inp)
    copy = build()
    twin_ad = LoraAdapter(copy, rank=RANK, seed=0)
    twin_ad.load_state_dict(ad.state_dict())
    twin_ad.attach()
    twin_ad.fold()
    assert getattr(copy, "_lora", None) is None and all(p.requires_grad for p in copy.parameters())
    assert not torch.equal(bits(copy.engine.arena.flat), flat0) and rel(forward(copy, inp), out) <= BF16_OUT
    assert [(k, tuple(v.shape)) for k, v in copy.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sd0.items()]


def test_hot_swap_under_a_captured_rollout_graph():
    m, inp = build(), inputs()
    den = M.GCDenoiser(m, 0.5).eval()
    first, second = random_adapter(m, 6), random_adapter(m, 7)
    other = LoraAdapter(m, rank=RANK, alpha=ALPHA, seed=0)
    first.attach()

    def policy(d):
        return rollout.ChunkedRolloutPolicy(d, act_window_size=10, multistep=10, action_dim=7, generator=torch.Generator(device="cuda").manual_seed(9))
    pol = policy(den)
    emb = {"state_images": inp["state_images"]}
    a1 = pol.denoise_actions(emb, inp["goals"])
    ent = m._route_cache["graph"]
    graph = ent["graph"]
    other.load_state_dict(second.state_dict())
    other.attach()
    assert m._lora is other and not first._attached
    a2 = pol.denoise_actions(emb, inp["goals"])
    assert m._route_cache["graph"] is ent and ent["graph"] is graph               # no recapture
    assert rel(a2, a1) > 10 * BF16_OUT

    def fresh(ad, calls):
        p = policy(M.GCDenoiser(folded_twin(ad), 0.5).eval())
        return [p.denoise_actions(emb, inp["goals"]) for _ in range(calls)][-1]   # the same position of the generator's stream
    e1, e2 = rel(a1, fresh(first, 1)), rel(a2, fresh(second, 2))
    print(f"graphed rollout chunk vs a fresh folded model: first adapter {e1:.2e}, after the swap {e2:.2e} (tol {BF16_OUT})")
    assert e1 <= BF16_OUT and e2 <= BF16_OUT


def test_hot_swap_to_an_adapter_with_fewer_targets_restores_the_plain_cast_elsewhere():
    """all four targets -> ("w1",): what the first adapter merged into wqkv, wo and w2 must not survive the swap."""
    m, inp = build(), inputs()
    plain = bits(m.engine.arena.lp)
    first = random_adapter(m, 11).attach()
    ar = m.engine.arena
    out_first = forward(m, inp)
    second = random_adapter(m, 12, targets=("w1",)).attach()
    assert m._lora is second and not first._attached and m.engine.arena is ar
    mask = torch.ones(ar.lp.numel(), dtype=torch.bool)
    for key, shp, off in ar.layout:
        if key.startswith("l") and key.endswith(".w1"):
            mask[off: off + int(torch.Size(shp).numel())] = False
    assert torch.equal(bits(ar.lp)[mask], plain[mask]) and not torch.equal(bits(ar.lp)[~mask], plain[~mask])
    out = forward(m, inp)
    e = rel(out, forward(folded_twin(second), inp))
    print(f"all four targets -> (w1,): output vs a twin folded with the second adapter only, rel-L2 {e:.2e} (tol {BF16_OUT})")
    assert e <= BF16_OUT and rel(out, out_first) > 10 * BF16_OUT
    # and back: more targets again, then nothing
    first.attach()
    assert torch.equal(bits(forward(m, inp)), bits(out_first))
    first.detach()
    assert torch.equal(bits(m.engine.arena.lp), plain) and not m.engine._lora_bufs


def test_backward_refuses_an_adapter_changed_since_its_forward():
    m, inp = build(train=True), inputs()
    ad = random_adapter(m, 13).attach()
    den = M.GCDenoiser(m, 0.5).train()
    loss, _ = den.loss({"state_images": inp["state_images"]}, inp["actions"], inp["goals"], inp["noise"], torch.full((B_,), 0.9, device="cuda"))
    with torch.no_grad():
        ad.A_wo.mul_(1.5)
    with pytest.raises(RuntimeError, match="between this forward and its"):
        loss.backward()
    assert all(p.grad is None for p in ad.parameters())
    _loss_backward(m, inp, 3)                                                      # a new forward is fine
    assert all(p.grad is not None for p in ad.parameters())
    assert set(m.engine._lora_bufs) == {"flat", "ws"} and not hasattr(ad, "_scratch")     # the arena-sized scratch belongs to the model, not the adapter


def test_refused_combinations_raise_before_anything_changes():
    m32 = build(dtype="fp32")
    flags = [p.requires_grad for p in m32.parameters()]
    with pytest.raises(ValueError, match="bf16"):
        LoraAdapter(m32, rank=4).attach()
    assert getattr(m32, "_lora", None) is None and [p.requires_grad for p in m32.parameters()] == flags
    m = build(train=True)
    lp0 = bits(m.engine.arena.lp)
    opt = FusedAdamW(m)
    with pytest.raises(RuntimeError, match="FusedAdamW"):
        LoraAdapter(m, rank=4).attach()
    assert getattr(m, "_lora", None) is None and all(p.requires_grad for p in m.parameters()) and torch.equal(bits(m.engine.arena.lp), lp0)
    del opt
    m2 = build(train=True)
    ad = random_adapter(m2, 8).attach()
    lp1, mode = bits(m2.engine.arena.lp), m2.grad_mode
    with pytest.raises(RuntimeError, match="LoraAdapter"):
        FusedAdamW(m2)
    assert m2.grad_mode == mode and m2._lora is ad and torch.equal(bits(m2.engine.arena.lp), lp1)
    ema = ArenaEMA(m2, decay=0.99)
    for call in (lambda: ema.update(1), ema.swap):
        with pytest.raises(RuntimeError, match="LoraAdapter"):
            call()
    assert ema.flat is None and torch.equal(bits(m2.engine.arena.lp), lp1)


def test_state_dict_round_trip_on_the_device():
    m = build()
    ad = random_adapter(m, 10)
    sd = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in ad.state_dict().items()}
    twin = LoraAdapter(m, rank=RANK, seed=99)
    twin.load_state_dict(sd)
    assert twin.alpha == ALPHA and all(torch.equal(bits(a), bits(b)) for a, b in zip(twin.parameters(), ad.parameters()))
    inp = inputs()
    ad.attach()
    out = forward(m, inp)
    twin.attach()
    assert torch.equal(bits(forward(m, inp)), bits(out))
    with pytest.raises(ValueError, match="another adapter or model"):
        LoraAdapter(m, rank=RANK // 2).load_state_dict(sd)
