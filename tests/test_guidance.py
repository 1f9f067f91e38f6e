"""Classifier-free guidance, the parts that need no GPU: GCDenoiser's ``guidance_scale`` argument, the generic path over a foreign inner model
(two inner calls, the second with ``uncond=True``, combined as D_u + w (D_c - D_u)), and the additions to the C ABI (new structs that wrap the old
ones, new exports, ABI version unchanged)."""
import ctypes as C
import os
import re

import pytest
import torch
from torch import nn

import mode_diffusion_policy_amd as M
from mode_diffusion_policy_amd import _lib as L
from mode_diffusion_policy_amd import gc_sampling, samplers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mode_hip.h")).read()
GUIDED = {"ModeEmbedGuidedDesc": ("mode_embed_tokens_guided_fwd", "ModeEmbedDesc"),
          "ModeHeadGuidedDesc": ("mode_head_ddim_guided_fwd", "ModeHeadDesc"),
          "ModeGuidedArgs": ("mode_dit_forward_guided", "ModeForwardArgs")}


class Stub(nn.Module):
    """A foreign inner model: linear in the action, the goal enters additively unless ``uncond``; records its calls."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, state, action, goal, sigma, uncond=False, gain=1.0):
        self.calls.append(dict(uncond=bool(uncond), gain=gain))
        g = torch.zeros_like(goal) if uncond else goal
        return gain * (0.5 * action + g.mean(-1, keepdim=True) + state["state_images"].mean())


def stub_inputs(B=3):
    g = torch.Generator().manual_seed(5)
    return ({"state_images": torch.randn(B, 2, 4, generator=g)}, torch.randn(B, 10, 7, generator=g), torch.randn(B, 1, 6, generator=g),
            torch.rand(B, generator=g) + 0.1)


def test_argument_validation():
    den = M.GCDenoiser(Stub(), 0.5)
    assert den.guidance_scale is None                                     # the default: unguided
    assert M.GCDenoiser(Stub(), 0.5, guidance_scale=2).guidance_scale == 2.0
    for w in (0, 1, -1.5, 2.5, 7):
        den.guidance_scale = w
        assert den.guidance_scale == float(w) and isinstance(den.guidance_scale, float)
    den.guidance_scale = None
    assert den.guidance_scale is None
    for bad in (float("nan"), float("inf"), -float("inf"), "2", [2.0], torch.tensor(2.0), True, 1 + 2j):
        with pytest.raises(ValueError):
            M.GCDenoiser(Stub(), 0.5, guidance_scale=bad)
        with pytest.raises(ValueError):
            den.guidance_scale = bad
        assert den.guidance_scale is None                                 # a refused value leaves the attribute as it was


def test_default_is_one_inner_call_as_before():
    st, x, goal, sig = stub_inputs()
    den = M.GCDenoiser(Stub(), 0.5)
    c_skip, c_out, c_in = [M.utils.append_dims(v, x.ndim) for v in den.get_scalings(sig)]
    out = den(st, x, goal, sig)
    assert den.inner_model.calls == [dict(uncond=False, gain=1.0)]
    assert torch.equal(out, Stub()(st, x * c_in, goal, sig) * c_out + x * c_skip)


@pytest.mark.parametrize("w", [0.0, 1.0, 2.5, -0.5])
def test_generic_path_combines_two_inner_calls(w):
    st, x, goal, sig = stub_inputs()
    den = M.GCDenoiser(Stub(), 0.5, guidance_scale=w)
    out = den(st, x, goal, sig, gain=2.0)
    assert den.inner_model.calls == [dict(uncond=False, gain=2.0), dict(uncond=True, gain=2.0)]   # second call unconditional; other keywords kept
    plain = M.GCDenoiser(Stub(), 0.5)
    d_c, d_u = plain(st, x, goal, sig, gain=2.0), plain(st, x, goal, sig, gain=2.0, uncond=True)
    assert not torch.equal(d_c, d_u)
    assert torch.equal(out, d_u + w * (d_c - d_u))                         # no special case for 0 or 1: the same expression


def test_samplers_inherit_guidance_on_the_generic_path():
    """A sampler over a guided denoiser with a foreign inner model takes its step loop; every step is two inner calls."""
    st, x, goal, _ = stub_inputs()
    sig = gc_sampling.get_sigmas_exponential(4, 1e-2, 1.0)
    den = M.GCDenoiser(Stub(), 0.5, guidance_scale=2.5)
    ref = M.GCDenoiser(Stub(), 0.5)
    guided = lambda s, a, g, sg, **kw: ref(s, a, g, sg, uncond=True) + 2.5 * (ref(s, a, g, sg) - ref(s, a, g, sg, uncond=True))
    for fn in (gc_sampling.sample_ddim, samplers.sample_heun, samplers.sample_dpmpp_2m):
        den.inner_model.calls.clear()
        out = fn(den, st, x, goal, sig, disable=True)
        assert [c["uncond"] for c in den.inner_model.calls[:4]] == [False, True, False, True], fn.__name__
        assert torch.allclose(out, fn(guided, st, x, goal, sig, disable=True), rtol=1e-6, atol=1e-6), fn.__name__


def test_loss_ignores_the_scale():
    st, x, goal, sig = stub_inputs()
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(6))
    a, b = M.GCDenoiser(Stub(), 0.5), M.GCDenoiser(Stub(), 0.5, guidance_scale=3.0)
    la, lb = a.loss(st, x, goal, noise, sig), b.loss(st, x, goal, noise, sig)
    assert torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1])
    assert b.inner_model.calls == [dict(uncond=False, gain=1.0)]


def _tiny_dit(**kw):
    with torch.device("meta"):                                             # no storage: these models only have to refuse
        return M.MoDeDiT(**{**dict(obs_dim=8, goal_dim=8, device="cuda", goal_conditioned=True, action_dim=7, embed_dim=64, embed_pdrob=0, attn_pdrop=0.0,
                                   n_layers=1, n_heads=2, goal_seq_len=1, obs_seq_len=1, action_seq_len=10, num_experts=4, top_k=2), **kw})


def test_hip_model_refuses_guidance_it_cannot_run_before_touching_the_device():
    st, x, goal, sig = {"state_images": torch.zeros(2, 2, 8)}, torch.zeros(2, 10, 7), torch.zeros(2, 1, 8), torch.ones(2)
    with pytest.raises(ValueError, match="eval"):                          # training mode with a scale set
        M.GCDenoiser(_tiny_dit().train(), 0.5, guidance_scale=2.0)(st, x, goal, sig)
    with pytest.raises(ValueError, match="top_k"):                         # shapes only the fallback row kernels take
        M.GCDenoiser(_tiny_dit(top_k=3).eval(), 0.5, guidance_scale=2.0)(st, x, goal, sig)
    with pytest.raises(ValueError, match="embed_dim"):
        M.GCDenoiser(_tiny_dit(embed_dim=4352).eval(), 0.5, guidance_scale=2.0)(st, x, goal, sig)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def _struct_body(name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S)
    assert m, f"{name} is not declared in include/mode_hip.h"
    return m.group(1)


@pytest.mark.parametrize("name", sorted(GUIDED))
def test_header_declares_the_guided_structs_and_exports(name):
    export, wrapped = GUIDED[name]
    body = _struct_body(name)
    assert re.match(r"\s*%s \w+;" % wrapped, body), f"{name} must wrap {wrapped} as its first member"
    assert re.search(r"\bint %s\(const %s\* \w+," % (export, name) if name != "ModeGuidedArgs" else r"\bint %s\(" % export, HEADER)
    assert export in L.PROTOTYPES
    if name != "ModeEmbedGuidedDesc":
        assert re.search(r"const float\* scale;", body), f"{name} carries the guidance scale as a device pointer"
    assert int(re.search(r"#define\s+MODE_HIP_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 13 == L.ABI_VERSION   # an addition, not a new ABI


@pytest.mark.parametrize("name", sorted(GUIDED))
def test_ctypes_mirrors_wrap_the_old_structs(name):
    cls, inner = getattr(L, name), getattr(L, GUIDED[name][1])
    first = cls._fields_[0]
    assert first[1] is inner and getattr(cls, first[0]).offset == 0 and getattr(cls, first[0]).size == C.sizeof(inner)
    if name != "ModeEmbedGuidedDesc":
        assert cls._fields_[1:] == [("scale", C.c_void_p)] and cls.scale.offset == C.sizeof(inner)


@pytest.mark.parametrize("name", sorted(GUIDED))
def test_ctypes_mirrors_agree_with_the_library(name):
    lib = L.load()
    assert lib.mode_hip_sizeof(name.encode()) == C.sizeof(getattr(L, name)) > 0
    assert lib.mode_hip_sizeof(GUIDED[name][1].encode()) == C.sizeof(getattr(L, GUIDED[name][1]))   # the wrapped struct keeps its layout
    assert hasattr(lib, GUIDED[name][0])


def test_guided_exports_refuse_before_any_launch():
    """Bad arguments and unsupported shapes come back as status codes before a pointer is followed (so this runs without a device)."""
    lib = L.load()
    BAD, UNSUPPORTED = -1, -2
    head = dict(B=2, T=14, D=256, A_len=10, A_dim=7, k=2, u=16, Y=16, y_dtype=L.MODE_BF16, y_splits=4, y_split_stride=0, pos=16, posw=16, g=16, eps=1e-6,
                w_out=16, b_out=16, x_a=16, scal=16, denoised=16)
    call = lambda scale=16, **over: lib.mode_head_ddim_guided_fwd(C.byref(L.ModeHeadGuidedDesc(head=L.ModeHeadDesc(**{**head, **over}), scale=scale)), None)
    assert lib.mode_head_ddim_guided_fwd(None, None) == BAD
    assert call(F=16) == BAD                                               # the raw network output has no guided form
    assert call(scale=None) == BAD and call(scal=None) == BAD and call(x_a=None) == BAD and call(u=None) == BAD
    assert call(D=4100) == UNSUPPORTED and call(k=3) == UNSUPPORTED and call(y_splits=16) == UNSUPPORTED and call(D=258) == UNSUPPORTED
    emb = dict(B=2, T=14, D=256, A_len=10, A_dim=7, n_img=2, use_noise_token=1, emb_t=16, goal_e=16, img_e=16, actions=16, w_act=16, pos=16, g=16, x=16, h=16)
    ecall = lambda **over: lib.mode_embed_tokens_guided_fwd(C.byref(L.ModeEmbedGuidedDesc(emb=L.ModeEmbedDesc(**{**emb, **over}))), None)
    assert lib.mode_embed_tokens_guided_fwd(None, None) == BAD and ecall(goal_e=None) == BAD and ecall(emb_t=None) == BAD
    assert ecall(D=4100) == UNSUPPORTED and ecall(T=13) == UNSUPPORTED
    assert lib.mode_dit_forward_guided(None, None, None, None, 0, None) == BAD
