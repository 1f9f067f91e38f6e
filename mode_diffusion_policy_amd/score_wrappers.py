"""Mirror of ``mode.models.edm_diffusion.score_wrappers.GCDenoiser`` (Karras/EDM preconditioner) on the HIP denoiser.

``forward`` fuses the three scalings into the HIP launch chain: ``c_in`` is applied while the action tokens are embedded and
``F*c_out + x*c_skip`` is the epilogue of the output-head kernel (reference: score_wrappers.py:65-80 = 3 extra elementwise
launches + temporaries per call).
"""
from __future__ import annotations

import math
import numbers

import torch
from torch import nn

from .modedit import MoDeDiT
from .utils import append_dims


def _instantiate(cfg):
    """Accept a ready module, or a Hydra/OmegaConf node / plain dict with ``_target_`` (the agent passes a DictConfig because
    it is built with ``_recursive_: false``; score_wrappers.py:28)."""
    if isinstance(cfg, nn.Module):
        return cfg
    try:
        import hydra
        return hydra.utils.instantiate(cfg)
    except ImportError:
        kw = {k: v for k, v in dict(cfg).items() if k not in ("_target_", "_recursive_")}
        return MoDeDiT(**kw)


class GCDenoiser(nn.Module):
    """``guidance_scale`` (settable): None = the plain denoiser, every path and result as without the argument.  A finite number w = classifier-free
    guidance at sampling time - the model is trained with goal dropout for exactly this -:
        D_w(x; sigma, obs, goal) = D_u + w (D_c - D_u),   D_c = D(x; sigma, obs, goal),   D_u = D(x; sigma, obs, 0)
    (no special case for w = 0 or 1).  Guidance acts on the goal token and, with ``use_goal_in_routing``, on the router input; both branches share
    the observation tokens, the latent, sigma and the EDM scalings.  On the HIP MoDeDiT both branches run in ONE chain at twice the batch and the
    combine is a step of the head kernel's epilogue, ahead of any solver update: ``forward``, the graphed denoiser and every fused sampler carry
    it, so do all samplers of ``samplers.py``.  Eval only; ``loss`` ignores it."""

    def __init__(self, inner_model, sigma_data=1.0, guidance_scale=None):
        super().__init__()
        self.inner_model = _instantiate(inner_model)
        self.sigma_data = sigma_data
        self.guidance_scale = guidance_scale

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @guidance_scale.setter
    def guidance_scale(self, w):
        if w is not None:
            if isinstance(w, bool) or not isinstance(w, numbers.Real) or not math.isfinite(w):
                raise ValueError(f"guidance_scale must be None or a finite number, got {w!r}")
            w = float(w)
        self._guidance_scale = w

    def get_scalings(self, sigma):
        """c_skip, c_out, c_in   (score_wrappers.py:31-43)."""
        c_skip = self.sigma_data ** 2 / (sigma ** 2 + self.sigma_data ** 2)
        c_out = sigma * self.sigma_data / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        c_in = 1 / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        return c_skip, c_out, c_in

    def loss(self, state, action, goal, noise, sigma, *, action_mask=None, sample_weight=None, **kwargs):
        """Score-matching loss (score_wrappers.py:45-63) -> (loss, model_output).  On a HIP MoDeDiT in training mode the scalings, the
        target, the MSE and their backward are two HIP launches around the training chain (training.edm_loss); the expression below is
        the generic path (eval-mode loss, extra kwargs).

        ``action_mask`` (B, W) and ``sample_weight`` (B,), both optional: the loss becomes the mean over the elements weighted by
        ``c[b, w] = sample_weight[b] * action_mask[b, w]`` (an absent factor is 1), ``sum(c * sq_err) / (A * sum(c))``, and 0 when every ``c`` is
        0 - padded steps of a window (``data.WindowStream(pad="hold")``) then train nothing.  Without them nothing changes."""
        m = self.inner_model
        if isinstance(m, MoDeDiT) and m.training and not kwargs and torch.is_grad_enabled():
            from .training import edm_loss
            if action_mask is None and sample_weight is None:
                return edm_loss(self, state, action, goal, noise, sigma)
            return edm_loss(self, state, action, goal, noise, sigma, action_mask=action_mask, sample_weight=sample_weight)
        c_skip, c_out, c_in = [append_dims(x, action.ndim) for x in self.get_scalings(sigma)]
        noised_input = action + noise * append_dims(sigma, action.ndim)
        model_output = self.inner_model(state, noised_input * c_in, goal, sigma, **kwargs)
        target = (action - c_skip * noised_input) / c_out
        if action_mask is None and sample_weight is None:
            return (model_output - target).pow(2).flatten(1).mean(), model_output
        if action.ndim != 3:
            raise ValueError(f"action_mask / sample_weight need an action chunk of shape (B, W, A), got {tuple(action.shape)}")
        c = torch.ones(action.shape[:2], dtype=model_output.dtype, device=model_output.device)
        if action_mask is not None:
            c = c * action_mask.to(c).clamp_min(0)
        if sample_weight is not None:
            c = c * sample_weight.to(c).clamp_min(0).unsqueeze(1)
        den = action.shape[2] * c.sum()
        resid = torch.where(c.unsqueeze(2) > 0, model_output - target, torch.zeros_like(model_output))     # an element with c = 0 trains nothing, finite or not
        return (c.unsqueeze(2) * resid.pow(2)).sum() / den.clamp_min(torch.finfo(c.dtype).tiny) * (den > 0), model_output

    def forward(self, state, action, goal, sigma, **kwargs):
        """D(x; sigma) = F(x*c_in)*c_out + x*c_skip   (score_wrappers.py:65-80)."""
        m, w = self.inner_model, self.guidance_scale
        if isinstance(m, MoDeDiT):
            if w is not None and m.training:
                raise ValueError("guidance_scale is set: classifier-free guidance is an inference-time combine, call .eval() first")
            if not m.training and not kwargs:
                return m.denoise(state, action, goal, sigma, self.sigma_data, guidance=w)
        c_skip, c_out, c_in = [append_dims(x, action.ndim) for x in self.get_scalings(sigma)]
        den = m(state, action * c_in, goal, sigma, **kwargs) * c_out + action * c_skip
        if w is None:
            return den
        den_u = m(state, action * c_in, goal, sigma, **{**kwargs, "uncond": True}) * c_out + action * c_skip   # any inner model: the reference's `uncond` flag
        return den_u + w * (den - den_u)

    def _fused_model(self, *schedules):
        """The HIP MoDeDiT when its fused routes apply - eval mode, no autograd, every schedule given a 1-d tensor -, else None."""
        m = self.inner_model
        ok = isinstance(m, MoDeDiT) and not m.training and not torch.is_grad_enabled() and all(torch.is_tensor(s) and s.dim() == 1 for s in schedules)
        return m if ok else None

    def denoise_uniform(self, state, action, goal, sigma):
        """D(x; sigma) for ONE noise level shared by the whole batch (what every k-diffusion style sampler asks for: ``sigma * ones``), as one
        hipGraph replay of the HIP chain (``MoDeDiT.denoise_graphed``).  Returns None when the fast path does not apply (training mode, token /
        goal routing, a foreign inner model) - the caller then takes ``forward``."""
        m = self._fused_model()
        return None if m is None else m.denoise_graphed(state, action, goal, sigma, self.sigma_data, guidance=self.guidance_scale)

    def first_order_ode_fused(self, state, action, goal, sigmas):
        """The whole deterministic first-order solve  x <- (s'/s) x + (1 - s'/s) D(x; s)  over ``sigmas`` as one hipGraph replay
        (``MoDeDiT.sample_ddim_fused``).  That update is both sample_ddim's (gc_sampling.py:922-951: exp(-t')/exp(-t) = s'/s, -expm1(-h) = 1 - s'/s)
        and, multiplied out, sample_euler's without churn (gc_sampling.py:165-211: x + (x - D)/s (s' - s)).  None when the fast path does not apply."""
        m = self._fused_model(sigmas)
        return None if m is None else m.sample_ddim_fused(state, action, goal, sigmas, self.sigma_data, guidance=self.guidance_scale)

    def dpmpp_2m_fused(self, state, action, goal, sigmas):
        """sample_dpmpp_2m (gc_sampling.py:700-734) as one hipGraph replay: the same chain as the first-order solve, the head kernel applying the step to the
        two-point extrapolation (1 + 1/(2r)) D - (1/(2r)) D_old of the denoised prediction.  None when the fast path does not apply."""
        m = self._fused_model(sigmas)
        return None if m is None else m.sample_ddim_fused(state, action, goal, sigmas, self.sigma_data, solver="dpmpp_2m", guidance=self.guidance_scale)

    def two_stage_fused(self, state, action, goal, sigmas, solver: str):
        """sample_heun / sample_dpm_2 / sample_dpmpp_2s without churn, clipping or callback as one hipGraph replay (``MoDeDiT.sample_two_stage_fused``:
        every stage's update is linear and runs inside the head kernel).  None when the fast path does not apply."""
        m = self._fused_model(sigmas)
        return None if m is None else m.sample_two_stage_fused(state, action, goal, sigmas, self.sigma_data, solver, guidance=self.guidance_scale)

    def get_params(self):
        return self.inner_model.parameters()
