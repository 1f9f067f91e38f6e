"""GPU: AdamW with bf16 moments (mode_adamw_step_lp, optim.FusedAdamW / FlatAdamW with moment_dtype="bf16").  Everything is exact: the weights, the
bf16 shadow and the EMA must carry the bits of the fp32 kernel run on the expanded moments, and the stored moments the bits of the numpy reference's
stochastic rounding (tests/adamw_lp_refs.py) of that kernel's fp32 moments."""
import functools
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adamw_lp_refs as R  # noqa: E402
import mode_diffusion_policy_amd as M  # noqa: E402
from hip_helpers import Guarded, stream  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd.optim import ArenaEMA, FlatAdamW, FusedAdamW, GradClip  # noqa: E402
from oracle import mode_oracle as O  # noqa: E402
from oracle.weights import make_inputs, make_state_dict  # noqa: E402

HP = (1e-3, 0.9, 0.95, 1e-8, 0.05)                                          # lr, beta1, beta2, eps, weight_decay
SCALE = 1.37251                                                             # > 1: a gradient can then carry a moment into the last bf16 ulp below Inf
BAD_ARG = -1


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


def bf16_dev(b):
    """uint16 bits -> bfloat16 device tensor."""
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16).copy()).cuda().view(torch.bfloat16)


def u16(t):
    """bfloat16 / int16 tensor -> uint16 numpy bits."""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)


def expanded(t):
    """A bf16 moment tensor as the fp32 values it denotes (exact)."""
    return (t.detach().contiguous().view(torch.int16).to(torch.int32) << 16).view(torch.float32)


def lp_step(lib, p, g, m, v, n, elem_base, step, seed, scale, lp=None, ema=None, rate=0.0, st=None, hp=HP):
    return lib.mode_adamw_step_lp(p, g, m, v, n, elem_base, *hp, step, seed, scale, lp, ema, rate, st, stream())


# ------------------------------------------------------------------------------------------------------------ one launch through ctypes
@functools.lru_cache(maxsize=None)
def launch_inputs(n):
    """Host inputs of one launch, built once per size: fp32 p / g / ema and bf16 bits of m / v with the special values in front."""
    gen = torch.Generator().manual_seed(n)
    p, g, e = (torch.randn(n, generator=gen) for _ in range(3))
    m = R.rne_bf16(R.f32_bits((torch.randn(n, generator=gen) * 0.1).numpy()))                  # both signs
    v = R.rne_bf16(R.f32_bits((torch.rand(n, generator=gen) * 1e-3).numpy()))
    # (m bits, v bits, g): negative m, zeros of both signs, denormals, the bf16 maximum (g chosen so that the new moment lands in the last ulp below Inf:
    #  the rounding must truncate there), Inf and NaN moments
    special = [(0xBF80, 0x3A83, 0.5), (0x0000, 0x0000, 0.0), (0x8000, 0x0000, 0.0), (0x0001, 0x0003, 1e-30), (0x807F, 0x0040, -1e-25),
               (0x7F7F, 0x3A83, 3.395e38 / SCALE), (0xFF7F, 0x3A83, -3.395e38 / SCALE), (0x3C00, 0x7F7F, 1.87e19 / SCALE), (0x7F7F, 0x7F7F, 0.0),
               (0x7F80, 0x3A83, 0.25), (0xFF80, 0x7F80, 0.25), (0x7FC0, 0x3A83, 0.25), (0x3C00, 0x7FC1, 0.25), (0xFFFF, 0x3A83, 0.25),
               (0x3C00, 0x3A83, float("inf")), (0xBC00, 0x3A83, float("-inf"))]       # (an Inf moment meets inf - inf and leaves as NaN; an Inf gradient makes Inf moments)
    g = g.clone()
    order = [0, 3, 5, 9] if n == 4 else range(len(special))
    for i, k in enumerate(order):
        m[i], v[i], g[i] = special[k][0], special[k][1], special[k][2]
    return dict(p=p, g=g, e=e, m=m, v=v)


def fresh(n, host):
    out = {}
    for k in ("p", "e"):
        out[k] = Guarded(1, n); out[k].t.copy_(host[k].cuda().view(1, n))
    for k in ("m", "v"):
        out[k] = Guarded(1, n, torch.bfloat16, fill=0.0); out[k].t.copy_(bf16_dev(host[k]).view(1, n))
    out["lp"] = Guarded(1, n, torch.bfloat16, fill=0.0)
    return out


def fp32_reference(lib, n, host, step, scale, rate=0.25):
    """mode_adamw_step on the expanded moments: the bits of p / lp / ema the bf16-moment launch must reproduce, and this step's unrounded m / v."""
    p, e = host["p"].cuda(), host["e"].cuda()
    m, v = expanded(bf16_dev(host["m"])), expanded(bf16_dev(host["v"]))
    lp = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    L.check(lib.mode_adamw_step(p.data_ptr(), host["g"].cuda().data_ptr(), m.data_ptr(), v.data_ptr(), n, *HP, step, scale, lp.data_ptr(), e.data_ptr(), rate,
                                stream()), "adamw_step")
    torch.cuda.synchronize()
    return dict(p=bits(p), lp=bits(lp), ema=bits(e), m=m.cpu().numpy(), v=v.cpu().numpy())


def check_against(bufs, want):
    for k in ("p", "m", "v", "e", "lp"):
        assert bufs[k].intact(), k
    assert torch.equal(bits(bufs["p"].t).reshape(-1), want["p"]) and torch.equal(bits(bufs["lp"].t).reshape(-1), want["lp"])
    assert torch.equal(bits(bufs["e"].t).reshape(-1), want["ema"])
    for k in ("m", "v"):
        got = u16(bufs[k].t)
        bad = np.nonzero(got != want[k])[0]
        assert bad.size == 0, (k, bad[:8], got[bad[:8]], want[k][bad[:8]])


@pytest.mark.parametrize("mode", ["grad_scale", "clip_state"])
@pytest.mark.parametrize("n", [4, 1020, 65540])
def test_one_launch_is_the_fp32_kernel_with_its_moments_rounded_by_the_reference(n, mode):
    lib = L.load()
    host = launch_inputs(n)
    step, seed, base = 3, 0x1234ABCD, 4096
    st = torch.zeros(8, dtype=torch.int32, device="cuda")
    st.view(torch.float32)[2] = SCALE
    scale = float(st.view(torch.float32)[2])                                              # the fp32 value both paths multiply by
    ref = fp32_reference(lib, n, host, step, scale)
    want = R.expected_step(ref, seed, step, base)
    if n > 4:                                                                             # the inputs do reach the clamp: an unrounded moment in the last ulp below Inf
        for k in ("m", "v"):
            u = R.f32_bits(ref[k])
            assert np.any(((u & 0x7FFF0000) == 0x7F7F0000) & ((u & 0xFFFF) != 0)), k
        assert np.any(np.isnan(ref["m"])) and np.any(np.isinf(ref["m"])) and np.any(np.isinf(ref["v"]))
    g = host["g"].cuda()
    a = fresh(n, host)
    args = (a["p"].t.data_ptr(), g.data_ptr(), a["m"].t.data_ptr(), a["v"].t.data_ptr(), n, base, step, seed)
    if mode == "grad_scale":
        L.check(lp_step(lib, *args, scale, a["lp"].t.data_ptr(), a["e"].t.data_ptr(), 0.25, None), "adamw_step_lp")
    else:
        L.check(lp_step(lib, *args, 77.0, a["lp"].t.data_ptr(), a["e"].t.data_ptr(), 0.25, st.data_ptr()), "adamw_step_lp")   # the state overrides grad_scale
    torch.cuda.synchronize()
    check_against(a, want)
    assert np.any(u16(a["m"].t) != host["m"]) and np.any(u16(a["v"].t) != host["v"])
    # a skipped step: the launch returns before its first store
    st[4] = 1
    c, untouched = fresh(n, host), fresh(n, host)
    L.check(lp_step(lib, c["p"].t.data_ptr(), g.data_ptr(), c["m"].t.data_ptr(), c["v"].t.data_ptr(), n, base, step, seed, scale, c["lp"].t.data_ptr(),
                    c["e"].t.data_ptr(), 0.25, st.data_ptr()), "adamw_step_lp")
    torch.cuda.synchronize()
    for k in ("p", "m", "v", "e", "lp"):
        assert c[k].intact() and torch.equal(bits(c[k].t), bits(untouched[k].t)), k


def run_cut(lib, n, host, cuts, base, step, seed, blocks=0):
    """The range [0, n) as launches over [cuts[i], cuts[i + 1]) (in the given order), each with its own elem_base; returns the Guarded buffers."""
    g = host["g"].cuda()
    a = fresh(n, host)
    assert lib.mode_set_option(b"adamw_blocks", blocks) == 0
    try:
        for lo, hi in cuts:
            L.check(lp_step(lib, a["p"].t.data_ptr() + 4 * lo, g.data_ptr() + 4 * lo, a["m"].t.data_ptr() + 2 * lo, a["v"].t.data_ptr() + 2 * lo, hi - lo,
                            base + lo, step, seed, SCALE, a["lp"].t.data_ptr() + 2 * lo, a["e"].t.data_ptr() + 4 * lo, 0.25, None), "adamw_step_lp")
        torch.cuda.synchronize()
    finally:
        lib.mode_set_option(b"adamw_blocks", 0)
    return a


@pytest.mark.parametrize("n", [1020, 65540])
def test_bits_do_not_depend_on_the_grid_or_on_how_the_range_is_cut(n):
    lib = L.load()
    host = launch_inputs(n)
    step, seed = 5, 7
    base = (1 << 32) - 512                                                                 # the element index crosses 2^32 inside the range
    whole = run_cut(lib, n, host, [(0, n)], base, step, seed)
    ref = fp32_reference(lib, n, host, step, float(np.float32(SCALE)))
    check_against(whole, R.expected_step(ref, seed, step, base))
    rng = np.random.default_rng(n)
    pts = sorted(set((rng.integers(1, n // 4, 5) * 4).tolist()))
    cuts = list(zip([0] + pts, pts + [n]))
    variants = {"cut": run_cut(lib, n, host, cuts, base, step, seed), "cut, reversed": run_cut(lib, n, host, cuts[::-1], base, step, seed),
                "4 at a time": run_cut(lib, 1020, launch_inputs(1020), [(i, i + 4) for i in range(0, 1020, 4)], base, step, seed) if n == 1020 else None}
    for blocks in (1, 7, 0):
        variants[f"adamw_blocks={blocks}"] = run_cut(lib, n, host, [(0, n)], base, step, seed, blocks)
    for name, got in variants.items():
        if got is None:
            continue
        for k in ("p", "m", "v", "e", "lp"):
            assert got[k].intact() and torch.equal(bits(got[k].t), bits(whole[k].t)), (name, k)
    # the base is part of the definition: the same launches with another elem_base store other moments
    other = run_cut(lib, n, host, [(0, n)], base + 4, step, seed)
    assert not torch.equal(bits(other["m"].t), bits(whole["m"].t)) and torch.equal(bits(other["p"].t), bits(whole["p"].t))


def test_same_seed_and_step_repeat_and_other_steps_or_seeds_change_only_the_stored_moments():
    lib = L.load()
    n = 65540
    host = launch_inputs(n)
    # steps 1000 / 1001: both bias corrections are exactly 1.0 in fp64 (0.9^1000, 0.95^1000 < 2^-53), so the step changes nothing but the rounding bits
    assert 1.0 - 0.9 ** 1000 == 1.0 and 1.0 - 0.95 ** 1000 == 1.0
    a, b = run_cut(lib, n, host, [(0, n)], 0, 1000, 11), run_cut(lib, n, host, [(0, n)], 0, 1000, 11)
    for k in ("p", "m", "v", "e", "lp"):
        assert torch.equal(bits(a[k].t), bits(b[k].t)), k
    for step, seed in ((1001, 11), (1000, 12)):
        c = run_cut(lib, n, host, [(0, n)], 0, step, seed)
        assert not torch.equal(bits(c["m"].t), bits(a["m"].t)) and not torch.equal(bits(c["v"].t), bits(a["v"].t)), (step, seed)
        for k in ("p", "e", "lp"):
            assert torch.equal(bits(c[k].t), bits(a[k].t)), (step, seed, k)                # no weight sees a rounded moment


def test_second_moment_decays_on_the_device_bit_equal_to_the_reference():
    lib = L.load()
    beta2, steps, n = 0.999, 200, 65536
    b0, v0, want = R.decay_case(n, beta2, steps, 0)
    p, g = torch.ones(n, device="cuda"), torch.zeros(n, device="cuda")
    m, v = torch.zeros(n, dtype=torch.bfloat16, device="cuda"), bf16_dev(b0)
    for step in range(1, steps + 1):
        L.check(lp_step(lib, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 0, step, 0, 1.0, hp=(1e-3, 0.9, beta2, 1e-8, 0.0)), "adamw_step_lp")
    torch.cuda.synchronize()
    got = u16(v)
    assert np.array_equal(got, want) and not np.any(u16(m))
    ratio = R.expand(got).astype(np.float64) / v0.astype(np.float64)
    err = ratio.mean() / 0.999 ** steps - 1.0
    print(f"device: mean v_200 / v_0 = {ratio.mean():.6f}, relative error {err:+.2e}, per-element spread {ratio.std():.4f}")
    assert abs(err) < 1e-3
    assert bool((p == 1.0).all())                                                          # m = 0, no decay: the weights never moved


def test_bad_arguments_are_refused_and_nothing_is_launched():
    lib = L.load()
    n = 1020
    host = launch_inputs(n)
    a, untouched = fresh(n, host), fresh(n, host)
    g = host["g"].cuda()
    st = torch.zeros(8, dtype=torch.int32, device="cuda")
    P, G, Mo, V, LP, E = a["p"].t.data_ptr(), g.data_ptr(), a["m"].t.data_ptr(), a["v"].t.data_ptr(), a["lp"].t.data_ptr(), a["e"].t.data_ptr()

    def call(p=P, g_=G, m=Mo, v=V, n_=n, base=0, step=3, lp=LP, st_=None):
        return lp_step(lib, p, g_, m, v, n_, base, step, 5, 1.0, lp, E, 0.25, st_)
    cases = dict(n_mod_4=call(n_=n - 2), n_negative=call(n_=-4), p_null=call(p=None), g_null=call(g_=None), m_null=call(m=None), v_null=call(v=None),
                 p_unaligned=call(p=P + 4), g_unaligned=call(g_=G + 8), m_unaligned=call(m=Mo + 2), m_unaligned4=call(m=Mo + 4), v_unaligned=call(v=V + 4),
                 lp_unaligned=call(lp=LP + 4), base_negative=call(base=-4), base_mod_4=call(base=6), step_zero=call(step=0), st_unaligned=call(st_=st.data_ptr() + 2))
    torch.cuda.synchronize()
    for name, rc in cases.items():
        assert rc == BAD_ARG, (name, rc)
    for k in ("p", "m", "v", "e", "lp"):
        assert a[k].intact() and torch.equal(bits(a[k].t), bits(untouched[k].t)), k
    assert call(n_=0) == 0 and call(n_=0, p=None, m=None) == 0                             # an empty range is fine and launches nothing
    torch.cuda.synchronize()
    assert torch.equal(bits(a["p"].t), bits(untouched["p"].t))


# ------------------------------------------------------------------------------------------------------------ FusedAdamW (2 layers, embed_dim 128, B = 8)
CFG = O.DiTConfig(obs_dim=64, goal_dim=32, action_dim=7, embed_dim=128, n_layers=2, n_heads=4, action_seq_len=10, num_experts=4, top_k=2)
KW = dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)


def _setup(seed, freeze=True):
    cfg = CFG
    m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cuda", goal_conditioned=True, action_dim=7, embed_dim=cfg.embed_dim, embed_pdrob=0,
                  attn_pdrop=0.0, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1, obs_seq_len=1, action_seq_len=10, mlp_pdrop=0.0, goal_drop=0.0,
                  num_experts=cfg.num_experts, top_k=cfg.top_k, use_argmax=True, compute_dtype="bf16")
    m.load_state_dict(make_state_dict(cfg, seed))
    m = m.to("cuda").train()
    if freeze:
        m.freeze_router()
    inp = {k: v.cuda() for k, v in make_inputs(cfg, 8, 3).items()}
    den = M.GCDenoiser(m, 0.5).train()
    sig = torch.full((8,), 0.9, device="cuda")

    def backward():
        loss, _ = den.loss({"state_images": inp["state_images"]}, inp["actions"], inp["goals"], inp["noise"], sig)
        loss.backward()
    return m, backward


def _state(m, opt, ema=None):
    ar = m.engine.arena
    out = dict(flat=bits(ar.flat), lp=bits(ar.lp), m=bits(opt.exp_avg), v=bits(opt.exp_avg_sq))
    if ema is not None:
        out["ema"] = bits(ema.flat)
    return out


def _assert_twin_step(lp_m, lp_v, twin_m, twin_v, seed, step, what):
    """The bf16 optimizer's stored moments are the reference's rounding of the fp32 twin's moments of this step (element 0 = start of the buffer)."""
    wm, wv = R.round_moments(twin_m.cpu().numpy(), twin_v.cpu().numpy(), seed, step, 0)
    for k, got, want in (("exp_avg", u16(lp_m), wm), ("exp_avg_sq", u16(lp_v), wv)):
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, k, bad[:8], got[bad[:8]], want[bad[:8]])


@functools.lru_cache(maxsize=None)
def _twin_run(overlap):
    """Three clipped steps (frozen router, EMA) of a bf16-moment optimizer next to an fp32 twin that is re-seeded every step from the expanded bf16
    moments; then a step with a non-finite gradient.  Returns the final state bits."""
    seed = 0xC0FFEE
    ma, bwd_a = _setup(11)
    mb, bwd_b = _setup(11)
    clip = GradClip(max_norm=0.05, skip_nonfinite=True)
    oa = FusedAdamW(ma, clip=clip, moment_dtype="bf16", round_seed=seed, **KW)
    ob = FusedAdamW(mb, **KW)
    assert oa.exp_avg.dtype == oa.exp_avg_sq.dtype == torch.bfloat16 and oa.exp_avg.element_size() == 2 and ob.exp_avg.element_size() == 4
    assert oa.exp_avg.numel() == ob.exp_avg.numel()
    ea, eb = ArenaEMA(ma, decay=0.99, min_value=0.5), ArenaEMA(mb, decay=0.99, min_value=0.5)
    for step in range(1, 4):
        ob.exp_avg.copy_(expanded(oa.exp_avg)); ob.exp_avg_sq.copy_(expanded(oa.exp_avg_sq))
        bwd_a(); bwd_b()
        oa.step(overlap=overlap, ema=ea)
        scale = float(clip.scale)
        ob.step(grad_scale=scale, overlap=overlap, ema=eb)
        torch.cuda.synchronize()
        sa, sb = _state(ma, oa, ea), _state(mb, ob, eb)
        for k in ("flat", "lp", "ema"):
            assert torch.equal(sa[k], sb[k]), (step, k)                                   # weights, shadow and EMA never see a rounded moment
        _assert_twin_step(oa.exp_avg, oa.exp_avg_sq, ob.exp_avg, ob.exp_avg_sq, seed, step, f"step {step}")
        assert int(clip.skipped) == 0 and 0.0 < scale
        print(f"step {step} overlap {overlap}: scale {scale!r}, coef {float(clip.coef)!r}")
    assert bool((oa.exp_avg != 0).any()) and bool((oa.exp_avg_sq != 0).any())
    ar = ma.engine.arena
    assert oa._frozen_ranges()
    for rlo, rhi in oa._frozen_ranges():                                                  # the frozen router: never updated, its moments stay zero
        assert not bool(oa.exp_avg[rlo:rhi].any()) and not bool(oa.exp_avg_sq[rlo:rhi].any())
    # a non-finite gradient: the step is skipped, nothing changes - the bf16 moments keep their bits
    before = _state(ma, oa, ea)
    bwd_a()
    ar.grad[ar.offset("l0.w1") + 1234] = float("inf")
    oa.step(overlap=overlap, ema=ea)
    torch.cuda.synchronize()
    after = _state(ma, oa, ea)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert int(clip.skipped) == 1 and oa.step_count == 4
    return before


@pytest.mark.parametrize("overlap", [False, True])
def test_fused_adamw_bf16_moments_match_the_reseeded_fp32_twin_step_by_step(overlap):
    _twin_run(overlap)


def test_fused_adamw_bf16_moments_overlap_is_bit_identical_to_serial():
    a, b = _twin_run(False), _twin_run(True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_checkpoint_round_trip_continues_bit_identically_and_loads_across_dtypes():
    m, bwd = _setup(21, freeze=False)
    opt = FusedAdamW(m, moment_dtype="bf16", round_seed=99, **KW)
    ar, eng = m.engine.arena, m.engine
    for _ in range(2):
        bwd(); opt.step()
    sd = opt.state_dict()
    assert sd["moment_dtype"] == "bf16" and sd["round_seed"] == 99 and sd["exp_avg"].dtype == torch.bfloat16 and sd["step"] == 2
    saved = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
    flat, lp = ar.flat.clone(), ar.lp.clone()
    bwd(); opt.step()
    torch.cuda.synchronize()
    want = _state(m, opt)
    # back to the checkpoint through reset_state() (moments zeroed in place, in their dtype) and load_state_dict()
    opt.reset_state()
    assert opt.step_count == 0 and opt.exp_avg.dtype == torch.bfloat16 and not bool(opt.exp_avg.any()) and not bool(opt.exp_avg_sq.any())
    opt.round_seed = 5
    opt.load_state_dict(saved)
    assert opt.round_seed == 99 and opt.step_count == 2
    ar.flat.copy_(flat); ar.lp.copy_(lp); eng.weights_updated(lp_synced=True)
    bwd(); opt.step()
    torch.cuda.synchronize()
    got = _state(m, opt)
    for k in want:
        assert torch.equal(want[k], got[k]), k
    # a bf16 checkpoint into an fp32 optimizer: exact; an fp32 checkpoint (with or without the key) into a bf16 one: round-to-nearest-even, once
    m2, bwd2 = _setup(21, freeze=False)
    o32 = FusedAdamW(m2, **KW)
    o32.load_state_dict(opt.state_dict())
    assert o32.exp_avg.dtype == torch.float32 and torch.equal(o32.exp_avg, expanded(opt.exp_avg)) and torch.equal(o32.exp_avg_sq, expanded(opt.exp_avg_sq))
    assert o32.step_count == opt.step_count and o32.state_dict()["moment_dtype"] == "fp32"
    bwd2(); o32.step()
    torch.cuda.synchronize()
    sd32 = o32.state_dict()
    for drop in (False, True):
        d = {k: v for k, v in sd32.items() if not (drop and k in ("moment_dtype", "round_seed"))}
        opt.round_seed = 99
        opt.load_state_dict(d)
        assert opt.exp_avg.dtype == torch.bfloat16 and opt.round_seed == 99 and opt.step_count == o32.step_count
        for got_, src in ((opt.exp_avg, o32.exp_avg), (opt.exp_avg_sq, o32.exp_avg_sq)):
            assert np.array_equal(u16(got_), R.rne_bf16(R.f32_bits(src.cpu().numpy())))
    with pytest.raises(ValueError, match="moment_dtype"):
        opt.load_state_dict(dict(sd32, moment_dtype="fp16"))


def test_fuse_expert_step_and_zero1_are_refused_before_anything_changes():
    m, bwd = _setup(31, freeze=False)
    with pytest.raises(NotImplementedError, match="fuse_expert_step"):
        FusedAdamW(m, fuse_expert_step=True, moment_dtype="bf16", **KW)
    with pytest.raises(ValueError, match="moment_dtype"):
        FusedAdamW(m, moment_dtype="fp16", **KW)
    opt = FusedAdamW(m, moment_dtype="bf16", **KW)
    bwd(); opt.step()
    torch.cuda.synchronize()
    before = _state(m, opt)
    with pytest.raises(NotImplementedError, match="fuse_expert_step"):
        opt.set_fuse_expert_step(True)
    assert not opt.fuse_expert_step and getattr(m, "_fused_optimizer", None) is None
    from mode_diffusion_policy_amd.ddp import ArenaGradReducer
    red = ArenaGradReducer.for_model(m)
    bwd()
    for z in ("fp32", "bf16"):
        with pytest.raises(NotImplementedError, match="ZeRO-1"):
            opt.step(reducer=red, zero1=z)
    torch.cuda.synchronize()
    after = _state(m, opt)
    assert opt.step_count == 1
    for k in before:
        assert torch.equal(before[k], after[k]), k
    opt.step(reducer=red)                                                                  # a plain reducer is fine
    torch.cuda.synchronize()
    assert opt.step_count == 2 and not torch.equal(bits(m.engine.arena.flat), before["flat"])


# ------------------------------------------------------------------------------------------------------------ FlatAdamW
GROUPS = [[(5,), (1000,), (7,), (8, 4, 3, 3), (3,)], [(1,), (130,)]]                         # group 0, tensor 2 never gets a gradient
NO_GRAD = (0, 2)


def _flat_groups(seed):
    gen = torch.Generator().manual_seed(seed)
    groups = []
    for gi, shapes in enumerate(GROUPS):
        ps = []
        for s in shapes:
            t = torch.randn(s, generator=gen).cuda()
            ps.append(torch.nn.Parameter(t.contiguous(memory_format=torch.channels_last) if len(s) == 4 else t))
        groups.append(dict(params=ps, weight_decay=0.05 if gi == 0 else 0.0))
    return groups


def _set_flat_grads(groups_list, step, scale=1.0):
    gen = torch.Generator().manual_seed(1000 + step)
    for gi, shapes in enumerate(GROUPS):
        for pi, s in enumerate(shapes):
            g = (torch.randn(s, generator=gen) * scale).cuda()
            g = g.contiguous(memory_format=torch.channels_last) if len(s) == 4 else g
            for groups in groups_list:
                groups[gi]["params"][pi].grad = None if (gi, pi) == NO_GRAD else g.clone()


def _flat_twin_check(fa, fb, seed, step):
    for gi, (a, b) in enumerate(zip(fa._flat, fb._flat)):
        assert torch.equal(bits(a["flat"]), bits(b["flat"])), (step, gi)
        _assert_twin_step(a["exp_avg"], a["exp_avg_sq"], b["exp_avg"], b["exp_avg_sq"], seed, step, f"step {step} group {gi}")


def _flat_reseed(fa, fb):
    for a, b in zip(fa._flat, fb._flat):
        b["exp_avg"].copy_(expanded(a["exp_avg"])); b["exp_avg_sq"].copy_(expanded(a["exp_avg_sq"]))


def test_flat_adamw_bf16_moments_match_the_reseeded_fp32_twin():
    seed = 77
    ga, gb = _flat_groups(5), _flat_groups(5)
    fa = FlatAdamW(ga, lr=1e-2, moment_dtype="bf16", round_seed=seed)                       # default betas: beta2 = 0.999
    fb = FlatAdamW(gb, lr=1e-2)
    assert all(f["exp_avg"].dtype == torch.bfloat16 and f["exp_avg_sq"].element_size() == 2 for f in fa._flat) and len(fa._flat) == 2
    untouched = ga[0]["params"][2].detach().clone()
    for step in range(1, 4):
        _flat_reseed(fa, fb)
        _set_flat_grads([ga, gb], step)
        fa.step(grad_scale=0.5); fb.step(grad_scale=0.5)
        torch.cuda.synchronize()
        _flat_twin_check(fa, fb, seed, step)
    lo, hi = fa._flat[0]["spans"][2]
    assert torch.equal(ga[0]["params"][2].detach(), untouched) and not bool(fa._flat[0]["exp_avg_sq"][lo:hi].any())   # skipped like torch skips it
    assert bool(fa._flat[0]["exp_avg_sq"][hi:].any()) and bool(fa._flat[1]["exp_avg_sq"].any())
    sd = fa.state_dict()
    assert sd["moment_dtype"] == "bf16" and sd["round_seed"] == seed and all(t.dtype == torch.bfloat16 for t in sd["exp_avg"])
    fb.load_state_dict(sd)                                                                  # bf16 -> fp32: exact
    assert all(torch.equal(b["exp_avg_sq"], expanded(a["exp_avg_sq"])) for a, b in zip(fa._flat, fb._flat)) and fb.step_count == 3


def test_joint_clip_over_bf16_fused_and_flat_adamw():
    seed = 31337
    ma, bwd_a = _setup(61)
    mb, bwd_b = _setup(61)
    clip = GradClip(max_norm=0.05)
    oa, ob = FusedAdamW(ma, clip=clip, moment_dtype="bf16", round_seed=seed, **KW), FusedAdamW(mb, **KW)
    ga, gb = _flat_groups(9), _flat_groups(9)
    fa, fb = FlatAdamW(ga, lr=1e-2, clip=clip, moment_dtype="bf16", round_seed=seed), FlatAdamW(gb, lr=1e-2)
    assert clip.joint
    for step in range(1, 3):
        ob.exp_avg.copy_(expanded(oa.exp_avg)); ob.exp_avg_sq.copy_(expanded(oa.exp_avg_sq))
        _flat_reseed(fa, fb)
        bwd_a(); bwd_b()
        _set_flat_grads([ga, gb], step, scale=1e-2)
        clip.measure()
        scale = float(clip.scale)
        oa.step(); fa.step()
        ob.step(grad_scale=scale); fb.step(grad_scale=scale)
        torch.cuda.synchronize()
        sa, sb = _state(ma, oa), _state(mb, ob)
        assert torch.equal(sa["flat"], sb["flat"]) and torch.equal(sa["lp"], sb["lp"]), step
        _assert_twin_step(oa.exp_avg, oa.exp_avg_sq, ob.exp_avg, ob.exp_avg_sq, seed, step, f"fused, step {step}")
        _flat_twin_check(fa, fb, seed, step)
        assert float(clip.coef) <= 1.0 and int(clip.skipped) == 0


# ------------------------------------------------------------------------------------------------------------ no host sync, flat memory
def _flat_memory(fn, warm=3, reps=20, slack=1 << 20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        seen = []
        for _ in range(reps):
            fn()
            torch.cuda.synchronize()
            seen.append(torch.cuda.memory_allocated())
    finally:
        if was:
            gc.enable()
    assert max(seen) <= base + slack, (base, seen)


@pytest.mark.parametrize("overlap", [False, True])
def test_steps_never_sync_the_host_and_hold_no_memory_over_20_steps(overlap):
    m, bwd = _setup(71)
    opt = FusedAdamW(m, clip=GradClip(max_norm=0.05), moment_dtype="bf16", **KW)
    ema = ArenaEMA(m, decay=0.99, min_value=0.5)
    groups = _flat_groups(3)
    fl = FlatAdamW(groups, lr=1e-3, clip=GradClip(max_norm=0.05), moment_dtype="bf16")
    plain = FlatAdamW(_flat_groups(4), lr=1e-3, moment_dtype="bf16")                        # and without a clip state
    _set_flat_grads([groups, plain.param_groups], 0)
    grads = [[p.grad for p in g["params"]] for g in groups]

    def one(guard=True):
        bwd()
        for g, gs in zip(groups, grads):
            for p, gr in zip(g["params"], gs):
                p.grad = gr
        torch.cuda.set_sync_debug_mode("error" if guard else 0)
        try:
            opt.step(overlap=overlap, ema=ema)
            fl.step()
            plain.step(grad_scale=0.5)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    one(guard=False)                                                                        # (the chunk tables are built and uploaded here, once)
    _flat_memory(one)
    assert int(opt.clip.skipped) == 0 and int(fl.clip.skipped) == 0 and opt.step_count >= 24
