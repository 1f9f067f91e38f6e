"""GPU: device-side gradient norms, global-norm clipping and the non-finite-safe step (csrc/grad_norm.hip, mode_adamw_step_clipped, optim.GradClip)
against the fp64 reference and the DERIVED bound of tests/grad_norm_refs.py - the kernels on synthetic flat buffers through ctypes, then FusedAdamW /
FlatAdamW at the c1e4 configuration, B = 8."""
import ctypes as C
import functools
import gc
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import grad_norm_refs as R  # noqa: E402
import mode_diffusion_policy_amd as M  # noqa: E402
from hip_helpers import Guarded, stream  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd.optim import ArenaEMA, FlatAdamW, FusedAdamW, GradClip, build_chunk_table  # noqa: E402
from oracle.weights import get_config, make_inputs, make_state_dict  # noqa: E402

CH = L.MODE_GRAD_CHUNK
U = R.U


def rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


def build_train(cfgname, seed, dtype, **over):
    cfg = get_config(cfgname)
    kw = dict(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cuda", goal_conditioned=True, action_dim=7, embed_dim=cfg.embed_dim,
              embed_pdrob=0, attn_pdrop=0.0, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1, obs_seq_len=1, action_seq_len=10,
              mlp_pdrop=0.0, goal_drop=0.0, num_experts=cfg.num_experts, top_k=cfg.top_k, use_argmax=True, compute_dtype=dtype)
    kw.update(over)
    m = M.MoDeDiT(**kw)
    sd = make_state_dict(cfg, seed)
    m.load_state_dict(sd)
    return cfg, sd, m.to("cuda").train()


# ------------------------------------------------------------------------------------------------------------ synthetic buffers through ctypes
LENGTHS = [0, 1, 3, 4, 5, 255, 1023, CH - 1, CH, CH + 1, 2 * CH + 7]
ZERO_T = len(LENGTHS)                                                     # one more tensor, all zeros (CH + 5 elements)


class Synth:
    """A flat fp32 buffer holding the test tensors at offsets that are 16-byte but not 256-byte aligned; every gap is NaN, so a read outside
    [lo, lo + n) of any chunk poisons a partial.  Built once; the reference sums come from the same bits."""

    def __init__(self):
        sizes = LENGTHS + [CH + 5]
        spans, o = [], 4
        for k in sizes:
            if o % 64 == 0:
                o += 4
            spans.append((o, k, True))
            o += (k + 3) // 4 * 4 + 4
        host = torch.full((o + 64,), float("nan"))
        self.tensors = []
        for i, (lo, k, _) in enumerate(spans):
            host[lo: lo + k] = 0.0 if i == ZERO_T else R.make_values(k, 100 + i)
            self.tensors.append(host[lo: lo + k].clone())
        R.assert_normal_squares(self.tensors)
        assert all(lo % 4 == 0 and lo % 64 != 0 for lo, _, _ in spans)
        self.spans, self.sizes, self.host = spans, sizes, host
        self.tab = build_chunk_table(spans)
        self.n_chunks, self.n_tensors, self.numel = len(self.tab["lo"]), len(sizes), sum(sizes)
        self.ref_sq = R.ref_tensor_sq(self.tensors)
        self.g = host.cuda()
        assert self.g.data_ptr() % 256 == 0
        self.chunks, self.begin = chunk_dev(self.tab), torch.tensor(self.tab["begin"], dtype=torch.int32, device="cuda")


def chunk_dev(tab):
    arr = np.zeros(max(1, len(tab["lo"])), dtype=np.dtype([("lo", "<i8"), ("n", "<i4"), ("tensor", "<i4")]))
    k = len(tab["lo"])
    arr["lo"][:k], arr["n"][:k], arr["tensor"][:k] = tab["lo"], tab["n"], tab["tensor"]
    assert arr.itemsize == C.sizeof(L.ModeGradChunk) == 16
    return torch.from_numpy(arr.view(np.uint8)).cuda()


@functools.lru_cache(maxsize=None)
def synth():
    return Synth()


def sumsq(g, chunks, n_chunks, ranges):
    part = Guarded(1, max(1, n_chunks))
    for first, count in ranges:
        L.check(L.load().mode_grad_sumsq(g.data_ptr(), chunks.data_ptr(), first, count, part.t.data_ptr(), stream()), "grad_sumsq")
    torch.cuda.synchronize()
    assert part.intact()
    return part


def finish(part, begin, n_tensors, max_norm, grad_scale, skip_nonfinite, st=None):
    """mode_grad_clip_finish into Guarded outputs; returns (tensor_sq [n] cpu, state dict, the Guarded state for a further call)."""
    tsq = Guarded(1, max(1, n_tensors))
    if st is None:
        st = Guarded(1, 8, fill=0.0)
    assert C.sizeof(L.ModeGradClipState) == 32
    L.check(L.load().mode_grad_clip_finish(part.t.data_ptr(), begin.data_ptr(), n_tensors, float(max_norm), float(grad_scale), int(skip_nonfinite),
                                           tsq.t.data_ptr(), st.t.data_ptr(), stream()), "grad_clip_finish")
    torch.cuda.synchronize()
    assert tsq.intact() and st.intact()
    f, i = st.t.reshape(-1).cpu(), st.t.reshape(-1).view(torch.int32).cpu()
    state = dict(total_norm=float(f[0]), coef=float(f[1]), scale=float(f[2]), nonfinite=int(i[3]), skip=int(i[4]), skipped=int(i[5]),
                 scale_bits=int(i[2]), coef_bits=int(i[1]))
    return tsq.t.reshape(-1)[:n_tensors].cpu(), state, st


def f32_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


def test_stage1_per_tensor_sums_on_a_synthetic_buffer():
    s = synth()
    part = sumsq(s.g, s.chunks, s.n_chunks, [(0, s.n_chunks)])
    tsq, st, _ = finish(part, s.begin, s.n_tensors, 0.0, 1.0, 1)
    assert bool(torch.isfinite(part.t).all())                                            # no chunk read a NaN gap: nothing outside [lo, lo + n)
    for t, (want, k) in enumerate(zip(s.ref_sq, s.sizes)):
        got = float(tsq[t])
        print(f"tensor {t} n={k}: device {got!r} fp64 {want!r} err {abs(got - want):.3e} bound {R.bound_tensor_sq(want, k):.3e}")
        assert abs(got - want) <= R.bound_tensor_sq(want, k), (t, k, got, want)
    assert float(tsq[0]) == 0.0 and float(tsq[ZERO_T]) == 0.0 and bits(tsq)[ZERO_T] == 0  # empty and all-zero tensors: exactly +0.0
    total = R.ref_clip(s.ref_sq)[0]
    got = float(np.float64(np.float32(st["total_norm"])) ** 2)
    print(f"total: device norm^2 {got!r} fp64 {total!r} err {abs(got - total):.3e} bound {R.bound_total(total, s.n_chunks, s.numel):.3e}")
    assert abs(got - total) <= R.bound_total(total, s.n_chunks, s.numel)
    assert abs(st["total_norm"] - total ** 0.5) <= R.bound_norm(total ** 0.5, s.n_chunks, s.numel)
    # two runs: identical bits; one launch over the table == two launches over its halves (any split, either order)
    again = sumsq(s.g, s.chunks, s.n_chunks, [(0, s.n_chunks)])
    assert torch.equal(bits(again.t), bits(part.t))
    h = s.n_chunks // 2
    halves = sumsq(s.g, s.chunks, s.n_chunks, [(h, s.n_chunks - h), (0, h)])
    assert torch.equal(bits(halves.t), bits(part.t))
    tsq2, st2, _ = finish(halves, s.begin, s.n_tensors, 0.0, 1.0, 1)
    assert torch.equal(bits(tsq2), bits(tsq)) and f32_bits(st2["total_norm"]) == f32_bits(st["total_norm"])
    # an empty range launches nothing; bad arguments are refused on the host
    lib = L.load()
    assert lib.mode_grad_sumsq(s.g.data_ptr(), s.chunks.data_ptr(), 0, 0, part.t.data_ptr(), stream()) == 0
    assert lib.mode_grad_sumsq(s.g.data_ptr() + 4, s.chunks.data_ptr(), 0, 1, part.t.data_ptr(), stream()) == -1
    assert lib.mode_grad_sumsq(s.g.data_ptr(), s.chunks.data_ptr(), -1, 1, part.t.data_ptr(), stream()) == -1


def test_finish_clip_coefficient_scale_and_nonfinite_flags():
    s = synth()
    part = sumsq(s.g, s.chunks, s.n_chunks, [(0, s.n_chunks)])
    total, norm, _, _ = R.ref_clip(s.ref_sq)
    # below max_norm: coef exactly 1, scale has grad_scale's bits
    for gs in (1.0, 0.5, 0.3):
        _, st, _ = finish(part, s.begin, s.n_tensors, float(np.float32(2.0 * norm)), gs, 1)
        assert st["coef"] == 1.0 and st["scale_bits"] == f32_bits(gs) and st["nonfinite"] == st["skip"] == st["skipped"] == 0
        want = R.ref_clip(s.ref_sq, None, float(np.float32(gs)))[1]
        assert abs(st["total_norm"] - want) <= R.bound_norm(want, s.n_chunks, s.numel)
    # above max_norm (clipping active), also with grad_scale = 0.5: total_norm is the norm of the SCALED gradient
    for gs in (1.0, 0.5):
        mx = float(np.float32(0.5 * gs * norm))
        _, st, _ = finish(part, s.begin, s.n_tensors, mx, gs, 1)
        _, rnorm, rcoef, rscale = R.ref_clip(s.ref_sq, mx, gs)
        print(f"gs {gs}: norm {st['total_norm']!r} / {rnorm!r}, coef {st['coef']!r} / {rcoef!r} (bound {R.rel_coef(s.n_chunks) * rcoef:.3e}), scale {st['scale']!r} / {rscale!r}")
        assert rcoef < 1.0 and abs(st["total_norm"] - rnorm) <= R.bound_norm(rnorm, s.n_chunks, s.numel)
        assert abs(st["coef"] - rcoef) <= R.rel_coef(s.n_chunks) * rcoef
        assert abs(st["scale"] - rscale) <= R.rel_scale(s.n_chunks) * abs(rscale)
    # measure only
    _, st, _ = finish(part, s.begin, s.n_tensors, 0.0, 1.0, 1)
    assert st["coef"] == 1.0 and st["scale_bits"] == f32_bits(1.0) and abs(st["total_norm"] - norm) <= R.bound_norm(norm, s.n_chunks, s.numel)
    # one inf / one nan element: nonfinite; with skip_nonfinite also skip, and `skipped` counts; a finite gradient afterwards clears the flags only
    lo = s.spans[7][0]
    for bad in (float("inf"), float("nan")):
        g = s.g.clone()
        g[lo + 17] = bad
        pb = sumsq(g, s.chunks, s.n_chunks, [(0, s.n_chunks)])
        _, st, dev = finish(pb, s.begin, s.n_tensors, 1.0, 1.0, 1)
        assert st["nonfinite"] == 1 and st["skip"] == 1 and st["skipped"] == 1
        _, st, dev = finish(pb, s.begin, s.n_tensors, 1.0, 1.0, 1, st=dev)
        assert st["skip"] == 1 and st["skipped"] == 2
        _, st, dev = finish(pb, s.begin, s.n_tensors, 1.0, 1.0, 0, st=dev)
        assert st["nonfinite"] == 1 and st["skip"] == 0 and st["skipped"] == 2           # skip_nonfinite off: flagged, not skipped
        _, st, dev = finish(part, s.begin, s.n_tensors, 1.0, 1.0, 1, st=dev)
        assert st["nonfinite"] == 0 and st["skip"] == 0 and st["skipped"] == 2


@pytest.mark.parametrize("n", [4, 1020, 65540])
def test_adamw_step_clipped_is_adamw_step_with_the_state_scale(n):
    lib = L.load()
    gen = torch.Generator().manual_seed(n)
    host = {k: torch.randn(n, generator=gen) for k in ("p", "g", "m", "e")}
    host["v"] = torch.rand(n, generator=gen) * 1e-3
    st = torch.zeros(8, dtype=torch.int32, device="cuda")
    st.view(torch.float32)[2] = 0.37251
    scale = float(st.view(torch.float32)[2])                                             # the state's scale read back
    hp = (1e-3, 0.9, 0.95, 1e-8, 0.05, 3)

    def fresh():
        out = {}
        for k in ("p", "m", "v", "e"):
            out[k] = Guarded(1, n); out[k].t.copy_(host[k].cuda().view(1, n))
        out["lp"] = Guarded(1, n, torch.bfloat16, fill=0.0)
        return out

    g = host["g"].cuda()
    a, b, c = fresh(), fresh(), fresh()
    L.check(lib.mode_adamw_step(a["p"].t.data_ptr(), g.data_ptr(), a["m"].t.data_ptr(), a["v"].t.data_ptr(), n, *hp, scale, a["lp"].t.data_ptr(),
                                a["e"].t.data_ptr(), 0.25, stream()), "adamw_step")
    L.check(lib.mode_adamw_step_clipped(b["p"].t.data_ptr(), g.data_ptr(), b["m"].t.data_ptr(), b["v"].t.data_ptr(), n, *hp, b["lp"].t.data_ptr(),
                                        b["e"].t.data_ptr(), 0.25, st.data_ptr(), stream()), "adamw_step_clipped")
    st[4] = 1                                                                            # skip
    L.check(lib.mode_adamw_step_clipped(c["p"].t.data_ptr(), g.data_ptr(), c["m"].t.data_ptr(), c["v"].t.data_ptr(), n, *hp, c["lp"].t.data_ptr(),
                                        c["e"].t.data_ptr(), 0.25, st.data_ptr(), stream()), "adamw_step_clipped")
    torch.cuda.synchronize()
    untouched = fresh()
    for k in ("p", "m", "v", "e", "lp"):
        assert a[k].intact() and b[k].intact() and c[k].intact()
        assert torch.equal(bits(a[k].t), bits(b[k].t)), k                                # same bits as mode_adamw_step with that scale
        assert torch.equal(bits(c[k].t), bits(untouched[k].t)), k                        # skip: nothing stored
    assert not torch.equal(bits(a["p"].t), bits(untouched["p"].t)) and not torch.equal(bits(a["lp"].t), bits(untouched["lp"].t))
    assert lib.mode_adamw_step_clipped(b["p"].t.data_ptr(), g.data_ptr(), b["m"].t.data_ptr(), b["v"].t.data_ptr(), n, *hp, None, None, 0.0, None,
                                       stream()) == -1                                   # no state: refused


# ------------------------------------------------------------------------------------------------------------ model level (c1e4, B = 8)
def _setup(seed, **kw):
    cfg, sd, m = build_train("c1e4", seed, "bf16")
    inp = {k: v.cuda() for k, v in make_inputs(cfg, 8, 3).items()}
    den = M.GCDenoiser(m, 0.5).train()
    sig = torch.full((8,), 0.9, device="cuda")

    def backward():
        loss, _ = den.loss({"state_images": inp["state_images"]}, inp["actions"], inp["goals"], inp["noise"], sig)
        loss.backward()
        return loss
    return cfg, sd, m, backward


def _arena_state(m, opt, ema):
    ar = m.engine.arena
    return dict(flat=bits(ar.flat), m=bits(opt.exp_avg), v=bits(opt.exp_avg_sq), lp=bits(ar.lp), ema=bits(ema.flat))


def _grad_names(m):
    """[(name, gradient view)] of every tensor the optimizer updates: requires_grad and not the arena's dead parameter."""
    gv = m.engine.arena.g_by_name
    return [(n, gv[n]) for n, p in m.named_parameters() if p.requires_grad and n != "gripper_embed.weight"]


def _moment_view(m, flat, p):
    off = (p.data_ptr() - m.engine.arena.flat.data_ptr()) // 4
    return flat[off: off + p.numel()].view(p.shape)


@functools.lru_cache(maxsize=None)
def _clipped_run(overlap):
    """Three clipped steps of a c1e4 model with ArenaEMA; checks (a) - (c) on the way and returns the final state bits for (d)."""
    from mode_diffusion_policy_amd.ddp import optimizer_param_groups
    _, _, ma, bwd_a = _setup(11)
    _, _, mb, bwd_b = _setup(11)
    clip = GradClip(max_norm=1.0, skip_nonfinite=True)
    oa = FusedAdamW(ma, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05, clip=clip)
    ob = FusedAdamW(mb, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)
    assert oa.clip is clip and ob.clip is None
    ea, eb = ArenaEMA(ma, decay=0.99, min_value=0.5), ArenaEMA(mb, decay=0.99, min_value=0.5)
    ref = {n: p.detach().clone().requires_grad_(True) for n, p in ma.named_parameters()}

    class _Holder(torch.nn.Module):
        def named_parameters(self_inner, *a, **k):
            return iter(ref.items())
    topt = torch.optim.AdamW(optimizer_param_groups(_Holder(), 0.05), lr=1e-3, betas=(0.9, 0.95))
    for step in range(3):
        bwd_a(); bwd_b()
        named = _grad_names(ma)
        sq = R.ref_tensor_sq([g for _, g in named])
        numel = sum(g.numel() for _, g in named)
        chunks = sum(R.n_chunks(g.numel()) for _, g in named)
        if step == 0:
            clip.max_norm = float(np.float32(0.5 * R.ref_clip(sq)[1]))                   # half the first step's fp64 norm: clipping is active
        _, rnorm, rcoef, rscale = R.ref_clip(sq, clip.max_norm)
        for n, p in ma.named_parameters():
            ref[n].grad = None if p.grad is None else (p.grad.detach().double() * rcoef).float()
        oa.step(overlap=overlap, ema=ea)
        scale = float(clip.scale)
        ob.step(grad_scale=scale, overlap=overlap, ema=eb)
        topt.step()
        torch.cuda.synchronize()
        # (a) bit-identical to the twin stepping with the clip's scale as a host float
        sa, sb = _arena_state(ma, oa, ea), _arena_state(mb, ob, eb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (step, k)
        # (c) the per-tensor log and the total
        assert clip.names == [n for n, _ in sorted(named, key=lambda x: x[1].data_ptr())] and "gripper_embed.weight" not in clip.names
        tsq = dict(zip(clip.names, clip.tensor_sq.cpu().tolist()))
        for (n, g), want in zip(named, sq):
            assert abs(tsq[n] - want) <= R.bound_tensor_sq(want, g.numel()), (step, n, tsq[n], want)
            if want == 0.0:
                assert tsq[n] == 0.0, n                                                  # un-routed experts: exactly zero
        assert rcoef < 1.0 and abs(float(clip.total_norm) - rnorm) <= R.bound_norm(rnorm, chunks, numel), (float(clip.total_norm), rnorm)
        assert abs(scale - rscale) <= R.rel_scale(chunks) * rscale
        assert int(clip.nonfinite) == 0 and int(clip.skipped) == 0
        # (b) torch.optim.AdamW on the gradients scaled by the fp64 coefficient
        tol_m = R.rel_norm(chunks) + 4 * U
        worst = [0.0, 0.0]
        for n, p in ma.named_parameters():
            assert rel(p.detach(), ref[n].detach()) < 2e-6, (step, n)
            if ref[n].grad is None:
                continue
            stt = topt.state[ref[n]]
            e1, e2 = rel(_moment_view(ma, oa.exp_avg, p), stt["exp_avg"]), rel(_moment_view(ma, oa.exp_avg_sq, p), stt["exp_avg_sq"])
            worst = [max(worst[0], e1), max(worst[1], e2)]
            assert e1 <= tol_m and e2 <= 2 * tol_m, (step, n, e1, e2, tol_m)
        print(f"step {step} overlap {overlap}: norm {float(clip.total_norm)!r} ref {rnorm!r}; worst exp_avg {worst[0]:.3e} exp_avg_sq {worst[1]:.3e} (tol {tol_m:.3e})")
    out = _arena_state(ma, oa, ea)
    out["clip"] = bits(clip._state[:5])
    out["tensor_sq"] = bits(clip.tensor_sq)
    return out


@pytest.mark.parametrize("overlap", [False, True])
def test_clipped_steps_match_the_scaled_twin_torch_adamw_and_the_per_tensor_log(overlap):
    _clipped_run(overlap)


def test_overlapped_clipped_steps_are_bit_identical_to_serial_ones():
    a, b = _clipped_run(False), _clipped_run(True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_frozen_router_is_absent_from_the_log_and_the_total():
    _, _, m, bwd = _setup(51)
    clip = GradClip()                                                                    # measure only: the reference's logging hook
    opt = FusedAdamW(m, lr=1e-3, clip=clip)
    bwd(); opt.step()
    assert any("router" in n for n in clip.names) and float(clip.coef) == 1.0
    table = clip._chunks
    bwd(); opt.step()
    assert clip._chunks is table                                                         # nothing changed: the table is not rebuilt per step
    m.freeze_router()
    bwd()
    gv = m.engine.arena.g_by_name
    named = [(n, gv[n]) for n, p in m.named_parameters() if p.requires_grad and n != "gripper_embed.weight"]
    sq = R.ref_tensor_sq([g for _, g in named])
    opt.step()
    assert clip._chunks is not table and len(clip.names) == len(named) == len(clip.tensor_sq)
    assert not any("router" in n for n in clip.names) and "gripper_embed.weight" not in clip.names
    numel, chunks = sum(g.numel() for _, g in named), sum(R.n_chunks(g.numel()) for _, g in named)
    rnorm = R.ref_clip(sq)[1]
    assert abs(float(clip.total_norm) - rnorm) <= R.bound_norm(rnorm, chunks, numel)


@pytest.mark.parametrize("overlap", [False, True])
def test_nonfinite_gradient_skips_the_step_and_leaves_every_buffer_untouched(overlap):
    _, _, m, bwd = _setup(23)
    clip = GradClip(max_norm=1.0, skip_nonfinite=True)
    opt = FusedAdamW(m, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05, clip=clip)
    ema = ArenaEMA(m, decay=0.99, min_value=0.5)
    bwd(); opt.step(overlap=overlap, ema=ema)                                            # an ordinary step first: moments, EMA and shadow exist
    torch.cuda.synchronize()
    before = _arena_state(m, opt, ema)
    bwd()
    ar = m.engine.arena
    ar.grad[ar.offset("l0.w1") + 12345] = float("inf")
    opt.step(overlap=overlap, ema=ema)
    torch.cuda.synchronize()
    after = _arena_state(m, opt, ema)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert int(clip.skipped) == 1 and int(clip.nonfinite) == 1 and opt.step_count == 2   # attempted steps are counted on the host
    bwd(); opt.step(overlap=overlap, ema=ema)
    torch.cuda.synchronize()
    assert int(clip.skipped) == 1 and int(clip.nonfinite) == 0
    assert not torch.equal(bits(ar.flat), before["flat"]) and bool(torch.isfinite(ar.flat).all())


def test_refusals_happen_before_anything_irreversible():
    _, _, m, bwd = _setup(31)
    with pytest.raises(NotImplementedError, match="fuse_expert_step"):
        FusedAdamW(m, lr=1e-3, fuse_expert_step=True, clip=GradClip(max_norm=1.0))
    clip = GradClip(max_norm=1.0)
    opt = FusedAdamW(m, lr=1e-3, clip=clip)
    with pytest.raises(NotImplementedError, match="fuse_expert_step"):
        opt.set_fuse_expert_step(True)
    assert not opt.fuse_expert_step and getattr(m, "_fused_optimizer", None) is None and clip._members == [opt]     # (no backward has run)

    class _Reducer:
        world, slices, average = 2, [], False
    with pytest.raises(NotImplementedError, match="ZeRO-1"):
        opt._validate_zero1(_Reducer(), "fp32", None)
    from mode_diffusion_policy_amd.ddp import ArenaGradReducer
    red = ArenaGradReducer.for_model(m)
    bwd()
    flat = bits(m.engine.arena.flat)
    with pytest.raises(NotImplementedError, match="ZeRO-1"):
        opt.step(reducer=red, zero1="fp32")
    assert opt.step_count == 0 and torch.equal(bits(m.engine.arena.flat), flat)
    with pytest.raises(ValueError):
        GradClip(max_norm=0.0)


# ------------------------------------------------------------------------------------------------------------ FlatAdamW, joint clip
FLAT_SHAPES = [(1,), (3,), (5,), (1000,), (8, 4, 3, 3), (7,)]                              # the 4-D weight is channels_last; the last one gets no gradient


def _flat_params(seed):
    gen = torch.Generator().manual_seed(seed)
    ps = []
    for s in FLAT_SHAPES:
        t = torch.randn(s, generator=gen).cuda()
        if len(s) == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        ps.append(torch.nn.Parameter(t))
    return ps


def _flat_grads(step, scale=1.0):
    out = []
    for i, s in enumerate(FLAT_SHAPES[:-1]):
        g = (R.make_values(int(torch.Size(s).numel()), 1000 + 10 * step + i, -4.0, 1.0) * scale).reshape(s).cuda()
        out.append(g.contiguous(memory_format=torch.channels_last) if len(s) == 4 else g)
    return out + [None]


def _flat_moment(opt, name, p, i):
    f = opt._flat[0]
    return torch.as_strided(f[name], p.shape, p.stride(), f["spans"][i][0])


def test_flat_adamw_clipped_matches_torch_adamw():
    ps, rs = _flat_params(5), _flat_params(5)
    clip = GradClip(max_norm=1.0)
    opt = FlatAdamW(ps, lr=1e-2, betas=(0.9, 0.95), weight_decay=0.05, clip=clip)
    topt = torch.optim.AdamW(rs, lr=1e-2, betas=(0.9, 0.95), weight_decay=0.05)
    assert opt.clip is clip
    last = ps[-1].detach().clone()
    for step in range(3):
        gs = _flat_grads(step)
        R.assert_normal_squares([g for g in gs if g is not None])
        sq = R.ref_tensor_sq([g for g in gs if g is not None])
        if step == 0:
            clip.max_norm = float(np.float32(0.5 * R.ref_clip(sq)[1]))
        _, rnorm, rcoef, rscale = R.ref_clip(sq, clip.max_norm)
        for p, r, g in zip(ps, rs, gs):
            p.grad = None if g is None else g.clone()
            r.grad = None if g is None else (g.double() * rcoef).float()
        opt.step(); topt.step()
        torch.cuda.synchronize()
        numel, chunks = sum(g.numel() for g in gs if g is not None), len(sq)
        assert clip.names == [f"g0.p{i}" for i in range(5)]                             # the tensor without a gradient is not measured
        for got, want, g in zip(clip.tensor_sq.cpu().tolist(), sq, gs):
            assert abs(got - want) <= R.bound_tensor_sq(want, g.numel())
        assert rcoef < 1.0 and abs(float(clip.total_norm) - rnorm) <= R.bound_norm(rnorm, chunks, numel)
        tol_m = R.rel_norm(chunks) + 4 * U
        for i, (p, r) in enumerate(zip(ps[:-1], rs[:-1])):
            assert rel(p.detach(), r.detach()) < 2e-6, (step, i)
            e1 = rel(_flat_moment(opt, "exp_avg", p, i), topt.state[r]["exp_avg"])
            e2 = rel(_flat_moment(opt, "exp_avg_sq", p, i), topt.state[r]["exp_avg_sq"])
            assert e1 <= tol_m and e2 <= 2 * tol_m, (step, i, e1, e2, tol_m)
        assert torch.equal(ps[-1].detach(), last)


def test_joint_clip_over_fused_and_flat_adamw_shares_one_scale():
    _, _, ma, bwd_a = _setup(61)
    _, _, mb, bwd_b = _setup(61)
    clip = GradClip(max_norm=1.0)
    oa, ob = FusedAdamW(ma, lr=1e-3, clip=clip), FusedAdamW(mb, lr=1e-3)
    pa, pb = _flat_params(9), _flat_params(9)
    fa, fb = FlatAdamW(pa, lr=1e-2, clip=clip), FlatAdamW(pb, lr=1e-2)
    assert clip.joint
    for step in range(2):
        bwd_a(); bwd_b()
        gs = _flat_grads(step, scale=1e-2)                                               # comparable to the model's gradient norm: both parts matter
        for p, q, g in zip(pa, pb, gs):
            p.grad = None if g is None else g.clone()
            q.grad = None if g is None else g.clone()
        named = _grad_names(ma)
        sq_m, sq_f = R.ref_tensor_sq([g for _, g in named]), R.ref_tensor_sq([g for g in gs if g is not None])
        if step == 0:
            with pytest.raises(RuntimeError, match="measure"):
                oa.step()                                                                # a joint clip needs a fresh measurement ...
            with pytest.raises(RuntimeError, match="measure"):
                fa.step()
            assert oa.step_count == 0 and fa.step_count == 0                             # ... and refuses before anything changed
            clip.max_norm = float(np.float32(0.5 * R.ref_clip(sq_m + sq_f)[1]))
        clip.measure()
        total, rnorm, rcoef, _ = R.ref_clip(sq_m + sq_f, clip.max_norm)
        numel = sum(g.numel() for _, g in named) + sum(g.numel() for g in gs if g is not None)
        chunks = sum(R.n_chunks(g.numel()) for _, g in named) + len(sq_f)
        got = float(np.float64(np.float32(float(clip.total_norm))) ** 2)
        assert abs(got - total) <= R.bound_total(total, chunks, numel), (got, total)     # total_norm^2 == fp64 sum of BOTH parts
        print(f"step {step}: model part {math.fsum(sq_m)!r} + flat part {math.fsum(sq_f)!r} = {total!r}; device norm^2 {got!r}")
        assert math.fsum(sq_f) > 0.0 and rcoef < 1.0
        assert len(clip.names) == len(sq_m) + len(sq_f) and clip.names[-5:] == [f"g0.p{i}" for i in range(5)]
        with pytest.raises(ValueError, match="measure"):
            oa.step(grad_scale=0.5)                                                      # another scale than measure()'s: refused, nothing consumed
        scale = float(clip.scale)
        oa.step(); fa.step()
        ob.step(grad_scale=scale); fb.step(grad_scale=scale)
        torch.cuda.synchronize()
        # both members' launches read the same scale bits: each is bit-identical to its twin stepping with that one host float
        assert torch.equal(bits(ma.engine.arena.flat), bits(mb.engine.arena.flat)) and torch.equal(bits(oa.exp_avg), bits(ob.exp_avg))
        assert torch.equal(bits(fa._flat[0]["flat"]), bits(fb._flat[0]["flat"])) and torch.equal(bits(fa._flat[0]["exp_avg_sq"]), bits(fb._flat[0]["exp_avg_sq"]))
        with pytest.raises(RuntimeError, match="measure"):
            fa.step()                                                                    # each measurement is consumed once per member


# ------------------------------------------------------------------------------------------------------------ world-2 data parallelism on ONE GPU
def _dp_clip_worker(rank, world, port, max_norm, outdir):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mode_diffusion_policy_amd.ddp import ArenaGradReducer
        torch.cuda.set_device(0)
        cfg, sd, m = build_train("c1e4", 210, "bf16")
        B = 16
        inp = {k: v.cuda() for k, v in make_inputs(cfg, B, 55).items()}
        sig = torch.full((B,), 0.9, device="cuda")
        sl = slice(rank * B // world, (rank + 1) * B // world)
        den = M.GCDenoiser(m, 0.5).train()
        clip = GradClip(max_norm=max_norm)
        opt = FusedAdamW(m, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05, clip=clip)
        red = ArenaGradReducer.for_model(m, mode="allreduce", comm_dtype=torch.float32)
        norms, scales = [], []
        for step in range(2):
            loss, _ = den.loss({"state_images": inp["state_images"][sl]}, inp["actions"][sl], inp["goals"][sl], inp["noise"][sl], sig[sl])
            loss.backward()
            opt.step(reducer=red, overlap=True)
            torch.cuda.synchronize()
            norms.append(float(clip.total_norm)); scales.append(bits(clip._state[2:3]))
        torch.save(dict(flat=m.engine.arena.flat.cpu(), norms=norms, scales=scales), os.path.join(outdir, f"c{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_data_parallel_world2_clips_the_averaged_gradient(tmp_path):
    import socket
    import torch.multiprocessing as mp
    # single process, whole batch: the fp64 norm of the mean-loss gradient
    cfg, sd, m = build_train("c1e4", 210, "bf16")
    B = 16
    inp = {k: v.cuda() for k, v in make_inputs(cfg, B, 55).items()}
    den = M.GCDenoiser(m, 0.5).train()
    FusedAdamW(m, lr=1e-3)                                                               # arena gradient mode
    loss, _ = den.loss({"state_images": inp["state_images"]}, inp["actions"], inp["goals"], inp["noise"], torch.full((B,), 0.9, device="cuda"))
    loss.backward()
    torch.cuda.synchronize()
    rnorm = R.ref_clip(R.ref_tensor_sq([g for _, g in _grad_names(m)]))[1]
    max_norm = float(np.float32(0.5 * rnorm))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_dp_clip_worker, args=(r, 2, port, max_norm, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    w = [torch.load(tmp_path / f"c{r}.pt") for r in range(2)]
    assert torch.equal(bits(w[0]["flat"]), bits(w[1]["flat"]))                           # both ranks end with the same weights, bit for bit
    for a, b in zip(w[0]["scales"], w[1]["scales"]):
        assert torch.equal(a, b)                                                         # ... having applied the same scale bits
    assert w[0]["norms"] == w[1]["norms"]
    assert abs(w[0]["norms"][0] - rnorm) <= 1e-2 * rnorm, (w[0]["norms"], rnorm)         # the norm of the AVERAGED gradient (grad_scale carries 1/world)
    assert not torch.equal(w[0]["flat"], m.engine.arena.flat.cpu())                      # (and they moved: the parent's model never stepped)


# ------------------------------------------------------------------------------------------------------------ no host sync, flat memory
def _flat(fn, warm=3, reps=8, slack=1 << 20):
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
def test_step_and_measure_never_sync_the_host_and_hold_no_memory(overlap):
    _, _, m, bwd = _setup(71)
    clip = GradClip(max_norm=0.05)
    opt = FusedAdamW(m, lr=1e-4, clip=clip)
    ema = ArenaEMA(m, decay=0.99, min_value=0.5)
    ps = _flat_params(3)
    solo = GradClip(max_norm=0.05)
    fl = FlatAdamW(ps, lr=1e-3, clip=solo)
    grads = _flat_grads(0)

    def single():
        bwd()
        for p, g in zip(ps, grads):
            p.grad = g
        torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step(overlap=overlap, ema=ema)
            fl.step()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    bwd(); opt.step(overlap=overlap, ema=ema)                                            # (the chunk tables are built and uploaded here, once)
    for p, g in zip(ps, grads):
        p.grad = g
    fl.step()
    _flat(single)
    # the same two optimizers as members of ONE clip: measure() + both steps
    _, _, m2, bwd2 = _setup(72)
    joint = GradClip(max_norm=0.05)
    o2 = FusedAdamW(m2, lr=1e-4, clip=joint)
    p2 = _flat_params(4)
    f2 = FlatAdamW(p2, lr=1e-3, clip=joint)

    def both():
        bwd2()
        for p, g in zip(p2, grads):
            p.grad = g
        torch.cuda.set_sync_debug_mode("error")
        try:
            joint.measure()
            o2.step(overlap=overlap)
            f2.step()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    bwd2()
    for p, g in zip(p2, grads):
        p.grad = g
    joint.measure(); o2.step(overlap=overlap); f2.step()                                 # (tables built and uploaded here, once)
    _flat(both)
    assert int(clip.skipped) == 0 and int(joint.skipped) == 0 and float(joint.coef) < 1.0
