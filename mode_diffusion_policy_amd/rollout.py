"""Inference-side harness around the HIP sampler: what ``MoDEAgent`` does between "perceptual
embeddings + goal embedding" and "action for this control step" — noise-schedule / sampler dispatch, the initial noise draw, action
chunking with replanning every ``multistep`` steps, routing pre-cache per noise level, and loading the denoiser's weights from a
published checkpoint.  The reference agent (mode/models/mode_agent.py) is a LightningModule that also owns the ResNet / CLIP encoders;
those producers are out of scope here, so this harness starts at their outputs and — unlike the reference's ``step`` which is B = 1
(``pred_action_seq[0, ...]``, mode_agent.py:630) — serves a BATCH of environments per call (BASELINE configs[4]: 32 envs).
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace
from typing import Dict, Optional

import numpy as np
import torch

from . import gc_sampling as gs
from ._checks import _checked_float, _checked_int
from .engine import graphs_enabled


def get_noise_schedule(n_sampling_steps: int, noise_schedule_type: str, sigma_min: float, sigma_max: float, device="cpu") -> torch.Tensor:
    """``MoDEAgent.get_noise_schedule`` (mode_agent.py:841-861): same names, same defaults (Karras rho = 7), same error."""
    if noise_schedule_type == "karras":
        return gs.get_sigmas_karras(n_sampling_steps, sigma_min, sigma_max, 7, device)
    if noise_schedule_type == "exponential":
        return gs.get_sigmas_exponential(n_sampling_steps, sigma_min, sigma_max, device)
    if noise_schedule_type == "vp":
        return gs.get_sigmas_vp(n_sampling_steps, device=device)
    if noise_schedule_type == "linear":
        return gs.get_sigmas_linear(n_sampling_steps, sigma_min, sigma_max, device=device)
    if noise_schedule_type == "cosine_beta":
        return gs.cosine_beta_schedule(n_sampling_steps, device=device)
    if noise_schedule_type == "ve":
        return gs.get_sigmas_ve(n_sampling_steps, sigma_min, sigma_max, device=device)
    if noise_schedule_type == "iddpm":
        return gs.get_iddpm_sigmas(n_sampling_steps, sigma_min, sigma_max, device=device)
    raise ValueError("Unknown noise schedule type")


def sample_loop(model, sigmas, x_t, state, goal, sampler_type: str = "ddim", extra_args: Optional[dict] = None, scaler=None):
    """``MoDEAgent.sample_loop`` (mode_agent.py:779-839): sampler names -> functions, ``s_churn`` / ``s_min`` / ``use_scaler`` taken from
    ``extra_args`` the way the agent does, ``ValueError`` for an unknown name."""
    extra_args = extra_args or {}
    s_churn = extra_args.get("s_churn", 0)
    s_min = extra_args.get("s_min", 0)
    sc = scaler if extra_args.get("use_scaler", False) else None
    reduced = {k: extra_args[k] for k in ("s_churn", "keep_last_actions")} if extra_args else {}
    table = {
        "lms": lambda: gs.sample_lms(model, state, x_t, goal, sigmas, scaler=sc, disable=True, extra_args=reduced),
        "heun": lambda: gs.sample_heun(model, state, x_t, goal, sigmas, scaler=sc, s_churn=s_churn, s_tmin=s_min, disable=True),
        "euler": lambda: gs.sample_euler(model, state, x_t, goal, sigmas, scaler=sc, disable=True),
        "ancestral": lambda: gs.sample_dpm_2_ancestral(model, state, x_t, goal, sigmas, scaler=sc, disable=True),
        "euler_ancestral": lambda: gs.sample_euler_ancestral(model, state, x_t, goal, sigmas, scaler=sc, disable=True),
        "dpm": lambda: gs.sample_dpm_2(model, state, x_t, goal, sigmas, disable=True),
        "dpm_adaptive": lambda: gs.sample_dpm_adaptive(model, state, x_t, goal, sigmas[-2].item(), sigmas[0].item(), disable=True),
        "dpm_fast": lambda: gs.sample_dpm_fast(model, state, x_t, goal, sigmas[-2].item(), sigmas[0].item(), len(sigmas), disable=True),
        "dpmpp_2s_ancestral": lambda: gs.sample_dpmpp_2s_ancestral(model, state, x_t, goal, sigmas, scaler=sc, disable=True),
        "dpmpp_2m": lambda: gs.sample_dpmpp_2m(model, state, x_t, goal, sigmas, scaler=sc, disable=True),
        "dpmpp_2m_sde": lambda: gs.sample_dpmpp_sde(model, state, x_t, goal, sigmas, scaler=sc, disable=True),
        "ddim": lambda: gs.sample_ddim(model, state, x_t, goal, sigmas, scaler=sc, disable=True),
        "dpmpp_2s": lambda: gs.sample_dpmpp_2s(model, state, x_t, goal, sigmas, scaler=sc, disable=True),
        "debugging": lambda: gs.sample_dpmpp_2_with_lms(model, state, x_t, goal, sigmas, scaler=sc, disable=True),
        "dpmpp_2_with_lms": lambda: gs.sample_dpmpp_2_with_lms(model, state, x_t, goal, sigmas, scaler=sc, disable=True),
    }
    if sampler_type not in table:
        raise ValueError("desired sampler type not found!")
    return table[sampler_type]()


# Samplers whose step loop depends on the schedule only (no data-dependent control flow, no host-side noise source): whole call capturable in a hipGraph.
# Not here: "ddim" and "euler" (without churn the same update: both take MoDeDiT's fused graph, samplers.sample_euler) and "dpmpp_2m" (the same chain with the
# two-point extrapolation inside the head kernel, samplers.sample_dpmpp_2m -> GCDenoiser.dpmpp_2m_fused), "heun" / "dpm" / "dpmpp_2s" (two-stage solvers: every
# stage's linear update inside the head kernel, GCDenoiser.two_stage_fused), "lms" / "dpmpp_2_with_lms"
# (host-side quadrature of the schedule), "dpmpp_2m_sde" (torchsde Brownian tree on the host), "dpm_adaptive" / "dpm_fast" (step sizes from error
# norms / host floats).
_GRAPHABLE_SAMPLERS = ("euler_ancestral", "ancestral", "dpmpp_2s_ancestral")


class ChunkedRolloutPolicy:
    """Action-chunking policy for a batch of environments: plan ``act_window_size`` actions with the sampler, emit one per control step,
    replan every ``multistep`` steps (``MoDEAgent.forward`` / ``step`` / ``denoise_actions`` / ``precompute_expert_for_inference``,
    mode_agent.py:584-644, 733-760).

    ``step(perceptual_emb, latent_goal)``: ``perceptual_emb = {'state_images': (B, 2, obs_dim)}`` (the encoders' output), ``latent_goal``
    (B, G) or (B, 1, G); returns the actions of this control step, (B, action_dim).  With the default DDIM sampler a replanning call is one
    hipGraph replay; the routing decisions of every noise level are resolved once (``precompute_experts_for_inference``) like the agent does
    on its first inference call.  Goal-routed (``use_goal_in_routing``) and token-routed (``cond_router=False``) denoisers replan in one replay
    as well: their routing depends on the observations and is resolved inside the graph for every sample, so the cache the agent fills from
    the FIRST environment's goal (``latent_goal[:1]``) never routes the others.

    With ``static_resnet`` / ``gripper_resnet`` (the agent's perceptual encoders, mode_agent.py:132-160) ``step`` also takes the environment's
    observation as the agent does - ``{'rgb_obs': {'rgb_static': (B, T, 3, H, W), 'rgb_gripper': ...}}`` - and embeds it on replanning steps
    (``MoDEAgent.forward``, mode_agent.py:598-603) through ``GraphedVisualEncoder``: one more hipGraph replay instead of ~640 eager launches.

    ``camera_transforms={'rgb_static': CameraTransform, 'rgb_gripper': CameraTransform}`` (needs the encoders; None, the default, changes nothing):
    ``rgb_obs`` then holds the cameras' own frames, uint8 ``(B, T, H, W, 3)`` at the cameras' resolution on the policy's device, and one launch
    (camera.py, csrc/frame_prep.hip) resizes, normalises and writes them straight into the encoder graph's input buffers."""

    def __init__(self, denoiser, num_sampling_steps: int = 10, sigma_min: float = 0.001, sigma_max: float = 80.0,
                 noise_scheduler: str = "exponential", sampler_type: str = "ddim", act_window_size: int = 10, multistep: int = 10,
                 action_dim: int = 7, generator: Optional[torch.Generator] = None, static_resnet=None, gripper_resnet=None,
                 encoder_autocast: Optional[torch.dtype] = torch.bfloat16, camera_transforms: Optional[dict] = None):
        self.camera_transforms = self._checked_transforms(camera_transforms, static_resnet is not None and gripper_resnet is not None)
        if multistep > act_window_size:
            raise ValueError("multistep cannot exceed the planned window")
        if (static_resnet is None) != (gripper_resnet is None):
            raise ValueError("give both perceptual encoders or neither")
        self.encoders = None
        if static_resnet is not None:
            from .perceptual_encoders import GraphedVisualEncoder
            self.encoders = GraphedVisualEncoder(static_resnet.eval(), gripper_resnet.eval(), encoder_autocast)
        self.model = denoiser
        self.num_sampling_steps, self.sigma_min, self.sigma_max = num_sampling_steps, sigma_min, sigma_max
        self.noise_scheduler, self.sampler_type = noise_scheduler, sampler_type
        self.act_window_size, self.multistep, self.action_dim = act_window_size, multistep, action_dim
        self.generator = generator
        self.need_precompute_experts_for_inference = True
        self.reset()

    _CAMERAS = ("rgb_static", "rgb_gripper")

    @classmethod
    def _checked_transforms(cls, camera_transforms, have_encoders: bool):
        """``camera_transforms=`` of the constructor: None, or a dict of one CameraTransform per camera of a policy that owns the encoders."""
        if camera_transforms is None:
            return None
        from .camera import CameraTransform
        if not isinstance(camera_transforms, dict) or set(camera_transforms) != set(cls._CAMERAS):
            raise ValueError(f"camera_transforms must be a dict with exactly the keys {list(cls._CAMERAS)}, got "
                             f"{sorted(camera_transforms) if isinstance(camera_transforms, dict) else type(camera_transforms).__name__}")
        for name in cls._CAMERAS:
            if not isinstance(camera_transforms[name], CameraTransform):
                raise ValueError(f"camera_transforms[{name!r}] must be a CameraTransform, got {type(camera_transforms[name]).__name__}")
        if not have_encoders:
            raise ValueError("camera_transforms feed the policy's perceptual encoders: pass static_resnet / gripper_resnet as well")
        return dict(camera_transforms)

    def _frames_device(self) -> torch.device:
        return next(self.model.inner_model.parameters()).device

    def _check_u8_frames(self, rgb, n: Optional[int] = None):
        """The raw observation's contract of a policy built with ``camera_transforms``: both cameras, uint8 (n, T, H, W, 3) each with one T,
        2 T = n_img_tokens, on the policy's device, at most 8 source pixels per output pixel; a row's frames one contiguous block (made so here)."""
        from .camera import check_frames_u8

        def camera(name, f):
            if torch.is_tensor(f) and f.dtype != torch.uint8:
                raise ValueError(f"{name}: a policy built with camera_transforms takes the camera's uint8 (n, T, H, W, 3) frames, got {f.dtype} "
                                 f"{tuple(f.shape)}; float frames go to a policy without camera_transforms")
            if not torch.is_tensor(f) or f.dim() != 5 or (n is not None and f.shape[0] != n):
                raise ValueError(f"{name} must be uint8 ({'n' if n is None else n}, T, H, W, 3) (one row per environment), got {tuple(getattr(f, 'shape', ()))}")
            f = check_frames_u8(f, name, self._frames_device())
            self.camera_transforms[name].check_source(f.shape[2], f.shape[3], name)
            return f
        return self._check_cameras(rgb, camera, "rows and number of frames T", lambda f: tuple(f.shape[:2]))

    def _check_cameras(self, rgb, camera, same: str, key):
        """What every raw observation has to meet: exactly the two cameras, each passing ``camera(name, frames) -> frames`` (the caller's own
        contract), both with one ``key(frames)`` - named ``same`` in the refusal - and 2 T = n_img_tokens.  Returns the two checked tensors."""
        if not isinstance(rgb, dict) or set(rgb) != set(self._CAMERAS):
            raise ValueError(f"rgb_obs must hold exactly the cameras {list(self._CAMERAS)}, got {sorted(rgb) if isinstance(rgb, dict) else type(rgb).__name__}")
        out = tuple(camera(name, rgb[name]) for name in self._CAMERAS)
        if key(out[1]) != key(out[0]):
            raise ValueError(f"both cameras must carry the same {same}, got {key(out[0])} and {key(out[1])}")
        T, n_img = out[0].shape[1], self.model.inner_model.n_img_tokens
        if 2 * T != n_img:
            raise ValueError(f"2 * T frames (T = {T}) must equal the model's n_img_tokens = {n_img}")
        return out

    def _transform_pair(self):
        return tuple(self.camera_transforms[name] for name in self._CAMERAS)

    def reset(self) -> None:
        """Start of an episode (the reference agent's ``reset``): replan at the next ``step``."""
        self.rollout_step_counter = 0
        self.pred_action_seq: Optional[torch.Tensor] = None

    def _schedule(self, dev) -> torch.Tensor:
        """The noise schedule of this policy, built once per device: handing the sampler the SAME tensor every call lets it recognise the
        schedule (pointer + version) without comparing values."""
        cached = getattr(self, "_sigmas", None)
        if cached is None or cached.device != torch.device(dev):
            cached = self._sigmas = get_noise_schedule(self.num_sampling_steps, self.noise_scheduler, self.sigma_min, self.sigma_max, dev)
        return cached

    def precompute_expert_for_inference(self, goal=None) -> None:
        inner = self.model.inner_model
        dev = next(inner.parameters()).device
        for sigma in self._schedule(dev)[:-1]:
            inner.precompute_experts_for_inference(sigma, goal)

    @torch.no_grad()
    def denoise_actions(self, perceptual_emb: Dict[str, torch.Tensor], latent_goal: torch.Tensor, extra_args: Optional[dict] = None,
                        x: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``x``: the initial latent, (B, act_window_size, action_dim) already at ``sigma_max`` (``validation.Validator`` plans from a window's own
        noise); None, the default, draws it from the policy's generator."""
        self.model.eval()
        dev = perceptual_emb["state_images"].device
        if latent_goal.dim() < perceptual_emb["state_images"].dim():
            latent_goal = latent_goal.unsqueeze(1)
        if self.need_precompute_experts_for_inference:
            self.precompute_expert_for_inference(latent_goal[:1] if self.model.inner_model.use_goal_in_routing else None)
            self.need_precompute_experts_for_inference = False
        sigmas = self._schedule(dev)
        if x is None:
            x = torch.randn((len(latent_goal), self.act_window_size, self.action_dim), device=dev, generator=self.generator) * self.sigma_max
        elif tuple(x.shape) != (len(latent_goal), self.act_window_size, self.action_dim):
            raise ValueError(f"x must be {(len(latent_goal), self.act_window_size, self.action_dim)}, got {tuple(x.shape)}")
        if self.sampler_type in _GRAPHABLE_SAMPLERS and not extra_args:
            out = self._sample_graphed(sigmas, x, perceptual_emb, latent_goal)
            if out is not None:
                return out
        return sample_loop(self.model, sigmas, x, perceptual_emb, latent_goal, self.sampler_type, extra_args)

    def _sample_graphed(self, sigmas, x, perceptual_emb, latent_goal):
        """The whole sampler call (every denoiser call, every update of the recurrence, the samplers' own noise draws) as ONE hipGraph replay - what the
        fused DDIM path does for ``ddim`` and ``euler``, for the samplers whose control flow does not depend on the data (heun, dpm-solver(++) ...: the step
        loop only branches on which levels of the SCHEDULE are zero).  Captured once per (sampler, batch, weights storage); the ancestral samplers' noise
        comes from torch's default generator, which hipGraph capture advances per replay.  Goal and token routing are captured too: every denoiser call
        of the chunk routes its own samples / tokens inside the graph.  None = not applicable (training mode, MODE_HIP_GRAPH=0): the caller takes the
        step-by-step path."""
        from . import samplers as S
        from .modedit import MoDeDiT
        den = self.model
        inner = getattr(den, "inner_model", None)
        if not isinstance(inner, MoDeDiT) or inner.training or len(x) == 0 or not graphs_enabled():
            return None
        guidance = inner._guidance(getattr(den, "guidance_scale", None))   # classifier-free guidance: the device scalar every denoiser call of the chunk reads
        eng = inner.engine
        img, gl, x = inner._inputs(eng, perceptual_emb, x, latent_goal)
        B, guided = x.shape[0], guidance is not None
        cache = self.__dict__.setdefault("_chunk_graphs", {})
        key = (self.sampler_type, id(sigmas), sigmas._version) + inner._graph_key(eng, B, den.sigma_data, guided)
        ent = cache.get(key)
        if ent is None:
            def chunk(ent):                                                  # the observations are embedded INSIDE the graph, once per replay
                state, goal3 = {"state_images": ent["img"].view(B, inner.n_img_tokens, -1)}, ent["goals"].view(B, 1, -1)
                eng.embed_obs(ent["img"], ent["goals"], out=(ent["img_e"], ent["goal_e"]))
                cc = dict(inner=inner, sigma_data=float(den.sigma_data), obs_emb=(ent["img_e"], ent["goal_e"]), metas=[], guidance=guidance)
                S._set_chunk_capture(cc)
                try:
                    return sample_loop(den, sigmas, ent["x"], state, goal3, self.sampler_type, None), cc["metas"]
                finally:
                    S._set_chunk_capture(None)
            # (the warm-up also does the schedule's host-side reads)
            ent, res = inner._capture_entry(eng, cache, key, 4, img, gl, x, guided, chunk, sig=sigmas)
            ent["out"], ent["metas"] = res
        ent["x"].copy_(x); ent["img"].copy_(img); ent["goals"].copy_(gl)
        ent["graph"].replay()
        # expert-usage counters of every denoiser call, as the step-by-step path keeps them
        inner._account_calls(eng, ent["metas"], inner._internal_batch(B, guided))
        return ent["out"].clone()

    @torch.no_grad()
    def embed(self, obs: Dict, latent_goal: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Raw camera observation -> ``perceptual_emb`` (``MoDEAgent.embed_visual_obs``, mode_agent.py:548-567); embedded observations pass through."""
        if "state_images" in obs:
            return obs
        if self.encoders is None:
            raise ValueError("raw observations ('rgb_obs') need the policy's perceptual encoders: pass static_resnet / gripper_resnet")
        rgb = obs["rgb_obs"]
        goal = latent_goal.reshape(latent_goal.shape[0], -1)
        if self.camera_transforms is not None:
            s, g = self._check_u8_frames(rgb)
            emb = self.encoders(s, g, goal, camera_transforms=self._transform_pair())
        else:
            emb = self.encoders(rgb["rgb_static"], rgb["rgb_gripper"], goal)
        return {"state_images": emb["state_images"].to(torch.float32)}

    @torch.no_grad()
    def step(self, perceptual_emb: Dict, latent_goal: torch.Tensor) -> torch.Tensor:
        if self.rollout_step_counter % self.multistep == 0:
            self.pred_action_seq = self.denoise_actions(self.embed(perceptual_emb, latent_goal), latent_goal)
        current = self.pred_action_seq[:, self.rollout_step_counter]
        self.rollout_step_counter += 1
        if self.rollout_step_counter == self.multistep:
            self.rollout_step_counter = 0
        return current


# VectorEnvPolicy's samplers: the deterministic ones whose whole call is one captured chunk of MoDeDiT._sample_chunk (sampler_type -> its solver there;
# "euler" without churn is the DDIM update, see samplers.sample_euler).  The others draw in-loop noise from torch's global generator, which would tie an
# environment's actions to which other environments replan with it.
_VECTOR_SAMPLERS = {"ddim": "ddim", "euler": "ddim", "dpmpp_2m": "dpmpp_2m", "heun": "heun", "dpm": "dpm_2", "dpmpp_2s": "dpmpp_2s"}


def _u32_as_i32(values) -> torch.Tensor:
    """Host int32 tensor holding the uint32 bit patterns of ``values`` (each taken modulo 2^32)."""
    return torch.from_numpy(np.asarray([int(v) & 0xFFFFFFFF for v in values], dtype=np.uint32).view(np.int32).copy())


def _buckets(num_envs: int):
    """Batch sizes a replanning chunk runs at: the powers of two up to ``num_envs``, and ``num_envs``."""
    return sorted({1 << i for i in range(num_envs.bit_length()) if 1 << i <= num_envs} | {num_envs})


def ensemble_weights(m: float, depth: int) -> np.ndarray:
    """The weight table of temporal ensembling, ``w_i = exp(-m i)`` for the i-th oldest live plan (ACT's rule): the fp64 exponential rounded to
    fp32, ``depth`` entries.  The kernel reads this table and evaluates no transcendental itself."""
    return np.exp(-float(m) * np.arange(depth, dtype=np.float64)).astype(np.float32)


def coherence_weights(rho: float, length: int) -> np.ndarray:
    """The weight table of candidate selection (``VectorEnvPolicy(candidates=N, coherence_decay=rho)``), ``w_i = rho ** i`` for the i-th coming
    step: the fp64 power rounded to fp32, ``length`` entries.  The kernel reads this table and evaluates no transcendental itself."""
    return (float(rho) ** np.arange(length, dtype=np.float64)).astype(np.float32)


def _env_latents(what: str, seeds, draws, dev, shape, *tail) -> torch.Tensor:
    """One row per (seed, draw) from the single-row gather ``mode_<what>`` without observations: ``shape`` fp32 on ``dev``."""
    from . import _lib as L
    from .engine import _stream
    n = len(seeds)
    s, d = _u32_as_i32(seeds).to(dev), _u32_as_i32(draws).to(dev)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    x = torch.empty(shape, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(getattr(L.load(), "mode_" + what)(rows.data_ptr(), n, n, s.data_ptr(), d.data_ptr(), None, 0, None, 0, None, None, x.data_ptr(), *tail,
                                                  _stream()), what)
    return x


@torch.no_grad()
def env_noise(seeds, draws, act_window_size: int, action_dim: int, sigma_max: float, device="cuda") -> torch.Tensor:
    """The initial latents ``VectorEnvPolicy`` plans from: row i = draw ``draws[i]`` of the noise stream with seed ``seeds[i]`` times ``sigma_max``,
    (len(seeds), act_window_size, action_dim) fp32 on ``device``.  The stream is counter-based (formula: include/mode_hip.h, ABI 13), so any
    environment's replan can be reproduced from its seed and draw index alone."""
    seeds, draws = list(seeds), list(draws)
    if not seeds or len(seeds) != len(draws):
        raise ValueError("env_noise: one draw index per seed, at least one")
    return _env_latents("env_gather_noise", seeds, draws, torch.device(device), (len(seeds), act_window_size, action_dim),
                        act_window_size * action_dim, float(sigma_max))


@torch.no_grad()
def env_warm_latents(plans: torch.Tensor, seeds, draws, shift: int, sigma_start: float) -> torch.Tensor:
    """The initial latents of a warm-started replan (``VectorEnvPolicy(warm_start=k)``): row i is ``plans[i]`` advanced by ``shift`` rows, its last
    row held beyond the end, plus ``sigma_start`` times draw ``draws[i]`` of the noise stream with seed ``seeds[i]`` - the stream element
    ``env_noise`` scales by ``sigma_max``:  ``x0[i, w, a] = plans[i, min(w + shift, W - 1), a] + sigma_start * z_i[w, a]`` (fp32; formula:
    include/mode_hip.h).  ``plans`` (n, W, A) on a ROCm device, 1 <= shift < W, sigma_start finite and >= 0; returns (n, W, A) fp32 there."""
    seeds, draws = list(seeds), list(draws)
    if not torch.is_tensor(plans) or plans.dim() != 3 or plans.shape[0] == 0:
        raise ValueError(f"env_warm_latents: plans must be a (n, W, A) tensor, got {tuple(getattr(plans, 'shape', ()))}")
    n, W, A = plans.shape
    if len(seeds) != n or len(draws) != n:
        raise ValueError("env_warm_latents: one seed and one draw index per plan")
    if plans.device.type != "cuda":
        raise ValueError("env_warm_latents: plans must be on a ROCm device")
    old = plans.to(torch.float32).contiguous()
    return _env_latents("env_gather_warm", seeds, draws, plans.device, (n, W, A), old.data_ptr(), W, A, int(shift), float(sigma_start))


def _mask_words(mask: np.ndarray, nw: int) -> np.ndarray:
    """A host bool vector as ``nw`` little-endian uint32 words, bit b % 32 of word b // 32 = entry b (the control block's bitmasks)."""
    bits = np.packbits(mask, bitorder="little")
    return np.pad(bits, (0, 4 * nw - bits.size)).view("<u4")


def _select_desc(contrast: Optional[dict] = None, **common):
    """``ModeEnvSelectDesc`` from the fields both selections share; with ``contrast`` - ``lambda_``, ``bc``, ``fc``, ``M`` and ``K`` -
    ``ModeEnvBidDesc``.  A tensor stands for its address."""
    from . import _lib as L
    fields = {k: v.data_ptr() if torch.is_tensor(v) else v for k, v in {**common, **(contrast or {})}.items()}
    return (L.ModeEnvBidDesc if contrast else L.ModeEnvSelectDesc)(**fields)


def _candidate_dims(name: str, dims: str, chunk):
    if not torch.is_tensor(chunk) or chunk.dim() != 4 or chunk.numel() == 0:
        raise ValueError(f"{name}: chunk must be a non-empty {dims} tensor, got {tuple(getattr(chunk, 'shape', ()))}")
    return chunk.shape


def _select_rows(name: str, chunk, prev, has_prev, shift, weights) -> dict:
    """What ``select_coherent`` and ``select_bidirectional`` share behind their own checks: ``prev``, ``has_prev``, ``shift`` and ``weights``
    checked against ``chunk``, and the descriptor fields of n explicit rows - identity rows, the mask words, fp32 contiguous inputs, the
    ``chosen`` and ``selected`` outputs - as tensors on the chunk's device."""
    n, _, W, A = chunk.shape
    if W * A > 4096:
        raise ValueError(f"{name}: W * A must be at most 4096, got {W} * {A}")
    if not torch.is_tensor(prev) or tuple(prev.shape) != (n, W, A):
        raise ValueError(f"{name}: prev must be ({n}, {W}, {A}), one previous plan per row, got {tuple(getattr(prev, 'shape', ()))}")
    has = np.asarray(has_prev.cpu() if torch.is_tensor(has_prev) else has_prev)
    if has.dtype != np.bool_ or has.shape != (n,):
        raise ValueError(f"{name}: has_prev must be {n} host bools, got {has.dtype} {has.shape}")
    shift = _checked_int(shift, 1, W - 1, f"{name}: shift must be an int in [1, W - 1] = [1, {W - 1}], got {shift!r}")
    wt = np.asarray(weights.cpu() if torch.is_tensor(weights) else weights, dtype=np.float32).reshape(-1)
    if wt.size != W - shift:
        raise ValueError(f"{name}: weights must have W - shift = {W - shift} entries, got {wt.size}")
    if chunk.device.type != "cuda" or prev.device != chunk.device:
        raise ValueError(f"{name}: chunk and prev must be on one ROCm device")
    dev = chunk.device
    return dict(rows=torch.arange(n, dtype=torch.int32, device=dev), count=None, m_b=n, num_envs=n, W=W, A=A, shift=shift,
                has_prev=torch.from_numpy(_mask_words(has, (n + 31) // 32).view("<i4").copy()).to(dev),
                chunk=chunk.to(torch.float32).contiguous(), plan=prev.to(torch.float32).contiguous(), weights=torch.from_numpy(wt.copy()).to(dev),
                chosen=torch.empty(n, W, A, dtype=torch.float32, device=dev), selected=torch.empty(n, dtype=torch.int32, device=dev))


@torch.no_grad()
def select_coherent(chunk: torch.Tensor, prev: torch.Tensor, has_prev, shift: int, weights):
    """The candidate selection of ``VectorEnvPolicy(candidates=N)`` on explicit rows (csrc/env_pool.hip; formula: include/mode_hip.h): ``chunk``
    (n, N, W, A) holds N candidate plans per row, ``prev`` (n, W, A) the rows' previous plans, ``has_prev`` n host bools, 1 <= shift < W,
    ``weights`` the W - shift weights of the coming steps (``coherence_weights``).  Candidate c of row i scores
    ``sum_w weights[w] * sum_a (chunk[i, c, w, a] - prev[i, w + shift, a]) ** 2`` in fp32 (0 where ``has_prev[i]`` is false); the smallest score
    is selected, the lowest index on ties, a NaN score only when every score is NaN (then candidate 0).  Returns ``(chosen (n, W, A) fp32,
    selected (n,) int32, scores (n, N) fp32)`` on the inputs' device."""
    from . import _lib as L
    from .engine import _stream
    n, N, W, A = _candidate_dims("select_coherent", "(n, N, W, A)", chunk)
    if not 1 <= N <= 64:
        raise ValueError(f"select_coherent: the number of candidates N must be in [1, 64], got {N}")
    f = _select_rows("select_coherent", chunk, prev, has_prev, shift, weights)
    scores = torch.empty(n, N, dtype=torch.float32, device=chunk.device)
    d = _select_desc(scores=scores, N=N, **f)
    with torch.cuda.device(chunk.device):
        L.check(L.load().mode_env_select(C.byref(d), _stream()), "env_select")
    return f["chosen"], f["selected"], scores


@torch.no_grad()
def select_bidirectional(chunk: torch.Tensor, prev: torch.Tensor, has_prev, shift: int, weights, n_weak: int, topk: int, contrast_weight: float):
    """The selection of ``VectorEnvPolicy(candidates=N, contrast=M)`` on explicit rows (csrc/env_pool.hip; formulas: include/mode_hip.h): ``chunk``
    (n, N + M, W, A) holds per row N strong candidates followed by ``n_weak`` = M weak ones; ``prev``, ``has_prev``, ``shift`` and ``weights`` as
    for ``select_coherent``.  ``bc`` is ``select_coherent``'s score of all N + M candidates; S+ / S- are the min(topk, N) strong / min(topk, M)
    weak candidates of smallest ``bc`` (lower index on ties, NaN last); ``fc[c] = mean_{p in S+} d(c, p) - mean_{q in S-} d(c, q)`` with d the
    unweighted squared distance over the whole chunk; ``total = bc + contrast_weight * fc``, and the strong candidate of smallest total is
    selected by ``select_coherent``'s rule.  Returns ``(chosen (n, W, A) fp32, selected (n,) int32 in [0, N), total (n, N), bc (n, N + M),
    fc (n, N))`` on the inputs' device."""
    from . import _lib as L
    from .engine import _stream
    name = "select_bidirectional"
    n, NT, W, A = _candidate_dims(name, "(n, N + M, W, A)", chunk)
    M = _checked_int(n_weak, 1, NT - 1, f"{name}: n_weak must be an int in [1, {NT - 1}] (of the {NT} candidates at least one is strong), got {n_weak!r}")
    if NT > 64:
        raise ValueError(f"{name}: the number of candidates N + M must be at most 64, got {NT}")
    K = _checked_int(topk, 1, None, f"{name}: topk must be an int >= 1, got {topk!r}")
    lam = _checked_float(contrast_weight, 0.0, float("inf"), f"{name}: contrast_weight must be a finite float >= 0, got {contrast_weight!r}")
    f = _select_rows(name, chunk, prev, has_prev, shift, weights)
    dev, N = chunk.device, NT - M
    total, fc = torch.empty(n, N, dtype=torch.float32, device=dev), torch.empty(n, N, dtype=torch.float32, device=dev)
    bc = torch.empty(n, NT, dtype=torch.float32, device=dev)
    lam_dev = torch.tensor([lam], dtype=torch.float32).to(dev)
    d = _select_desc(dict(lambda_=lam_dev, bc=bc, fc=fc, M=M, K=min(K, 64)), scores=total, N=N, **f)
    with torch.cuda.device(dev):
        L.check(L.load().mode_env_select_bid(C.byref(d), _stream()), "env_select_bid")
    return f["chosen"], f["selected"], total, bc, fc


class VectorEnvPolicy(ChunkedRolloutPolicy):
    """``MoDEAgent.reset`` / ``step`` (mode_agent.py:584-637) for each of ``num_envs`` environments of a batch on its own: every environment keeps
    its own plan, its own position in it and its own noise stream, so a batch behaves like ``num_envs`` independent agents whose episodes start,
    end and pause at different steps.  The schedule, the sampler keywords and the routing pre-cache are ``ChunkedRolloutPolicy``'s.

    ``reset(envs=None, seeds=None)``: the listed environments (None = all, a sequence of indices or a host bool mask (num_envs,)) drop their
    plans and replan at their next active step; ``seeds`` (one int per listed environment) re-keys their noise streams and rewinds them to draw
    0, else the streams run on.  Environment b starts with seed ``seed + b``.

    ``step(perceptual_emb, latent_goal, active=None) -> (num_envs, action_dim)`` device tensor: ``perceptual_emb = {'state_images': (num_envs,
    n_img, obs_dim)}`` or, with the perceptual encoders (``static_resnet`` / ``gripper_resnet``), the raw observation ``{'rgb_obs':
    {'rgb_static': (num_envs, T, 3, H, W), 'rgb_gripper': (num_envs, T, 3, Hg, Wg)}}`` (fp32 or bf16, 2 T = the model's n_img_tokens),
    ``latent_goal`` (num_envs, G) or (num_envs, 1, G), ``active`` a HOST bool mask (None = all).  An active environment whose
    counter is 0 replans from its own observation and goal with the next draw of its stream; every active environment emits
    ``plan[b, counter]`` and advances ``counter = (counter + 1) % multistep``; inactive ones do neither and get a zero row.  Rows of the inputs of
    environments that do not replan are not read.  ``replanned``: the environments that replanned at the last step (host list).

    The m replanning environments run one chunk at the smallest bucket batch >= m (``_buckets``), padded by repeating the last one; one hipGraph
    per (sampler, bucket) holds the chain and the commit of the plans + the emission of the step's actions (csrc/env_pool.hip).  A replanning
    step is one H2D copy of the control block, one gather launch and one replay; any other step is one launch.  Neither synchronises with the
    host.  ``warmup`` captures every bucket ahead of a control loop.  Samplers: ``_VECTOR_SAMPLERS``.

    Raw frames: only the replanning environments' frames are read and encoded.  One more launch gathers their rows of both cameras into the
    encoders' input at the bucket batch (csrc/env_pool.hip, rounding fp32 to bf16 on the way when the encoders run under bf16 autocast, as the
    stem would), and one more replay runs the two towers at batch mb * T with FiLM on each environment's own goal row (two graph branches, as
    ``GraphedVisualEncoder``) straight into the chunk's observation buffer: two launches and two replays per replanning step.  The encoder
    graphs live in the policy's own store, one per bucket; in-place weight updates are seen by the next replan; encoders in training mode or
    MODE_HIP_GRAPH=0 run eagerly on the gathered rows.  With ``camera_transforms`` (see ``ChunkedRolloutPolicy``) the frames are the cameras'
    uint8 ``(num_envs, T, H, W, 3)`` and that gather launch is the fused resize + normalise of the replanning rows (csrc/frame_prep.hip, the same
    rows of the control block), writing bf16 under bf16 autocast and fp32 otherwise: the launch budget is unchanged.

    ``temporal_ensemble=m`` (a finite float >= 0; None, the default, is everything above unchanged) averages the overlapping predictions of an
    environment's last plans instead of letting a replan overwrite them (ACT's temporal ensembling), for ``multistep = s < act_window_size = W``.
    Let t be the environment's local time, its active steps since its last reset.  A plan born at t_p predicts step t in its row t - t_p and is
    live while 0 <= t - t_p < W: at most K = ceil(W / s) plans (``ensemble_depth``, at most 64).  With the live plans ordered oldest first,
    x_i their rows for step t and w_i = exp(-m i) (``ensemble_weights``: fp64 on the host, rounded to fp32), the emitted action is
    sum_i w_i x_i / sum_i w_i, both sums in fp32 in that order; m = 0 is the mean, one live plan is emitted bit for bit (so s = W emits what a
    policy without the option does).  Replanning, the draws, the initial latents, the buckets and the launch budget are unchanged: the commit +
    emit launch of a step is the ensembled kernel (csrc/env_pool.hip), which also keeps the ring.  ``reset`` drops every plan of the listed
    environments and rewinds their t to 0; inactive steps do not advance t.  ``plans`` stays the newest plan; ``plan_ring``, ``plan_births``,
    ``local_times`` and ``ensemble_weight_table`` expose the device state.

    ``warm_start=k`` (an int, 1 <= k <= num_sampling_steps - 1, with ``multistep = s < act_window_size = W``; None, the default, is everything above
    unchanged: the same code paths, launches and results) resumes a replan from the environment's previous plan instead of from noise (SDEdit-style
    warm starting).  An environment is WARM once a plan has been committed for it since its last ``reset`` (a host mirror beside the counters;
    pausing changes nothing), so the first replan of an episode is always cold: today's replan, ``sigma_max * z`` through the full schedule.  A
    warm replan starts from ``env_warm_latents(plans[b], seed, draw, shift=s, sigma_start=sigmas[k])`` - the unexecuted tail of the old plan, its
    last row held, noised to level k with the same stream element z a cold replan would scale by sigma_max - and runs the policy's solver on
    ``sigmas[k:]``: num_sampling_steps - k denoiser steps instead of num_sampling_steps (``dpmpp_2m`` starts its history afresh at step k).  Both
    kinds consume one draw.  The sub-schedule is one tensor per device whose values are bit-equal to the full schedule's, so the routing
    pre-cache serves it; warm chunks keep chunk and encoder graphs of their own per bucket (captured by ``warmup`` too), so alternating kinds
    never recapture.  A step whose replanners are all of one kind costs what it did: one gather launch and one replay.  A step with both runs
    two chunks, each at its own bucket: the cold one is staged first with an empty active mask into a scratch output - it commits its plans
    (counter 0, draw + 1, with ensembling the ring slot and its birth) and emits nothing - then the warm one with the step's mask and output,
    whose commit + emit launch emits the just-committed cold environments from ``plans`` (or the ring) like any environment that did not replan.
    This holds for the ensembled kernel as well, so ``temporal_ensemble`` combines with it; the warm start then reads ``plans``, the newest
    plan, not the ensembled trajectory.  ``guidance_scale`` needs nothing extra.  ``replanned_warm``: the warm ones among ``replanned``.  What
    warm-started plans do to task success is NOT measured in this repository (no trained checkpoint, no simulator): only the mechanics - exact
    latents, schedule and bookkeeping - and the cost (profiles/vector_env_warm_start.txt) are pinned.

    ``candidates=N`` (an int, 2 <= N <= 64, with ``multistep = s < act_window_size = W`` and ``num_envs * N <= MODE_ENV_MAX``; None, the default,
    and 1 are everything above unchanged: the same code paths, launches, draws and results) draws N candidate plans per replan and keeps the one
    closest to what the environment's previous plan predicted for the coming steps (the backward-coherence criterion of Bidirectional Decoding,
    Liu et al.).  A replan at bucket mb runs its chunk at batch mb * N, environment-major: chunk row j * N + c is candidate c of the j-th
    replanner, its observation and goal rows written N times, its latent the stream element ``z(seed, draws[b] * N + c)`` (uint32 arithmetic)
    - a replan still advances ``draws[b]`` by one, so ``env_noise`` / ``env_warm_latents`` reproduce any candidate from (seed, draw, c).  With
    P = ``plans[b]`` (the newest plan, also under ensembling), L = W - s and ``wt = coherence_weights(coherence_decay, L)`` (``coherence_decay`` a
    finite float in (0, 1], default 0.5, only legal with ``candidates``), candidate c scores ``sum_{w<L} wt[w] * sum_a (X_c[w, a] - P[w + s, a])**2``
    in fp32; the smallest score is selected, the lowest index on ties, a NaN score never before a non-NaN one (all NaN: candidate 0).  An
    environment with no plan committed since its last ``reset`` scores 0 for every candidate and takes candidate 0.  The selection is one more
    kernel inside the chunk's graph, between the chain and the commit (csrc/env_pool.hip; ``select_coherent`` runs it on explicit rows); which
    replanners have a previous plan travels in the control block, so a replanning step is still one H2D copy, one gather launch and one replay
    per chunk kind, with no host sync.  The selected plan is what is committed and emitted; everything downstream - counter, ring slot and birth
    under ``temporal_ensemble``, ``plans`` - is unchanged.  ``selected`` (num_envs,) int32, -1 before any replan, and ``candidate_scores``
    (num_envs, N) expose the last replan's choice.  With ``warm_start=k`` a warm replan's candidates are ``env_warm_latents(plans[b], seed,
    draws[b] * N + c, s, sigmas[k])`` through the sub-schedule; with raw frames the encoders still run once per environment at batch mb * T and
    their rows are broadcast to the N candidate rows inside the encoder graph.  Known cost: a cold replan (an episode's first) also runs N
    candidates and, without ``contrast``, keeps the first - running cold chunks at N = 1 would need a second family of graphs; with
    ``contrast`` a cold replan selects among its N candidates by the contrast term alone (below).  What candidate selection does to task
    success is NOT measured in this repository: only the mechanics and the cost (profiles/vector_env_candidates.txt) are pinned.

    ``contrast=M`` (an int >= 1, with ``candidates=N >= 2``, ``N + M <= 64`` and ``num_envs * (N + M) <= MODE_ENV_MAX``; None, the default, is
    everything above unchanged: the same entry points, draw indices, graphs and bits) adds the forward-contrast criterion of Bidirectional
    Decoding.  A replanning environment runs N STRONG candidates - its own goal row - and M WEAK ones - a zero goal row, the unconditional
    branch that classifier-free guidance defines, so the weak policy needs no weights of its own.  The chunk, its buffers and its bucket
    templates are sized by N + M: chunk row j * (N + M) + c is candidate c of the j-th replanner, strong ones first, its latent the stream
    element ``z(seed, draws[b] * (N + M) + c)``; a replan still advances ``draws[b]`` by one.  With ``bc_c`` the coherence score above for all
    N + M candidates (0 without a previous plan), S+ / S- the ``min(contrast_topk, N)`` strong / ``min(contrast_topk, M)`` weak candidates of
    smallest ``bc`` (lower index on ties, NaN last; with no previous plan the first by index; ``contrast_topk`` an int >= 1, default min(N, M))
    and ``d`` the unweighted squared distance over the whole chunk, a strong candidate gets ``fc_c = mean_{p in S+} d(c, p) - mean_{q in S-}
    d(c, q)`` and ``total_c = bc_c + contrast_weight * fc_c`` (fp32; exact expressions: include/mode_hip.h); the strong candidate of smallest
    total is selected by the rule above and a weak one never is.  ``contrast_weight`` (a finite float >= 0, default 1.0) is a settable
    attribute backed by a device scalar the kernel reads: a new value is used by the next replan, recaptures no graph and is in no graph key.
    ``contrast_weight`` and ``contrast_topk`` are only legal with ``contrast``.  Commit, ring, ``plans`` and ``selected`` are as above;
    ``candidate_scores`` holds ``total``, and ``coherence_scores`` (num_envs, N + M) and ``contrast_scores`` (num_envs, N) hold ``bc`` and
    ``fc`` of the last replan (``select_bidirectional`` runs the kernel on explicit rows).  Raw frames: the encoder towers still run once per
    environment, FiLM-conditioned on the environment's goal, taken from the first (strong) row; weak candidates share those observation
    embeddings, only the denoiser's goal row is zero.  ``warm_start``: weak candidates are warm-started from the same previous plan, like the
    strong ones.  ``guidance_scale`` needs nothing special - a zero-goal row's guided prediction is its unconditional one - but costs: the
    chain then runs 2 * mb * (N + M) rows and evaluates every weak row twice for the same result.  Cost: (N, M) costs what ``candidates=N + M``
    costs, the chain batch being the same (profiles/vector_env_contrast.txt).  A second, separately loaded weak model (an earlier checkpoint,
    the base model under a LoRA adapter) is out of scope; the selection does not depend on where weak rows come from.  What forward contrast
    does to task success is NOT measured in this repository (no trained checkpoint, no simulator): only the mechanics and the cost are pinned."""

    def __init__(self, denoiser, num_envs: int, seed: int = 0, extra_args: Optional[dict] = None, temporal_ensemble: Optional[float] = None,
                 warm_start: Optional[int] = None, candidates: Optional[int] = None, coherence_decay: Optional[float] = None,
                 contrast: Optional[int] = None, contrast_weight: Optional[float] = None, contrast_topk: Optional[int] = None, **kw):
        from . import _lib as L
        from .modedit import MoDeDiT
        sampler = kw.get("sampler_type", "ddim")
        n_steps, W, s = int(kw.get("num_sampling_steps", 10)), int(kw.get("act_window_size", 10)), int(kw.get("multistep", 10))

        def need_tail(what: str) -> None:                                    # the options that read the previous plan's unexecuted tail
            if not s < W:
                raise ValueError(f"{what} the unexecuted tail of the previous plan: it needs multistep < act_window_size, got multistep={s}, "
                                 f"act_window_size={W}")

        def need_room(rows_per_env: int, factor: str, got: str) -> None:     # a chunk runs num_envs * rows_per_env rows at most
            if isinstance(num_envs, (int, np.integer)) and int(num_envs) * rows_per_env > L.MODE_ENV_MAX:
                raise ValueError(f"num_envs * {factor} must be at most {L.MODE_ENV_MAX} (the largest batch a chunk runs at), got {int(num_envs)} * {got}")

        self.candidates, self.coherence_decay, self._ncand = None, None, 1
        if candidates is not None:
            self.candidates = _checked_int(candidates, 1, 64, f"candidates must be None or an int in [1, 64], got {candidates!r}")
            self.coherence_decay = 0.5
            if self.candidates > 1:
                need_tail("candidates scores each candidate against")
                need_room(self.candidates, "candidates", f"{self.candidates}")
                self._ncand = self.candidates
        if coherence_decay is not None:
            if candidates is None:
                raise ValueError("coherence_decay weighs the candidates' scores: it is only legal with candidates=N")
            self.coherence_decay = _checked_float(coherence_decay, 0.0, 1.0, f"coherence_decay must be a finite float in (0, 1], got {coherence_decay!r}",
                                                  lo_open=True)
        self.contrast, self.contrast_topk, self._contrast_weight, self._nweak, self._lambda = None, None, None, 0, None
        if contrast is not None:
            M = _checked_int(contrast, 1, None, f"contrast must be None or an int >= 1, the number of weak (zero-goal) candidates, got {contrast!r}")
            if self._ncand < 2:
                raise ValueError(f"contrast compares the strong candidates with each other and with the weak ones: it needs candidates >= 2, got "
                                 f"candidates={candidates!r}")
            if self._ncand + M > 64:
                raise ValueError(f"candidates + contrast must be at most 64, got {self._ncand} + {M}")
            need_room(self._ncand + M, "(candidates + contrast)", f"({self._ncand} + {M})")
            self.contrast = self._nweak = M
            self.contrast_topk = min(self._ncand, M)
            if contrast_topk is not None:
                self.contrast_topk = _checked_int(contrast_topk, 1, None, f"contrast_topk must be None or an int >= 1, got {contrast_topk!r}")
            self._contrast_weight = self._checked_contrast_weight(1.0 if contrast_weight is None else contrast_weight)
        elif contrast_weight is not None or contrast_topk is not None:
            raise ValueError("contrast_weight and contrast_topk shape the forward-contrast term: they are only legal with contrast=M")
        self._nper = self._ncand + self._nweak                               # chunk rows per replanning environment
        self.warm_start = None
        if warm_start is not None:
            self.warm_start = _checked_int(warm_start, 1, n_steps - 1, f"warm_start must be None or an int in [1, num_sampling_steps - 1] = "
                                           f"[1, {n_steps - 1}], got {warm_start!r}")
            need_tail("warm_start resumes from")
        self._checked_transforms(kw.get("camera_transforms"), kw.get("static_resnet") is not None and kw.get("gripper_resnet") is not None)
        self.temporal_ensemble, self.ensemble_depth, self._ens = None, None, None   # (the base constructor calls reset)
        if temporal_ensemble is not None:
            # (float() first: a bool or a numeric string is taken for its value, anything else float() refuses in its own words)
            self.temporal_ensemble = _checked_float(float(temporal_ensemble), 0.0, float("inf"), f"temporal_ensemble must be None or a finite float "
                                                    f">= 0, got {temporal_ensemble!r}")
            if 1 <= s <= W and -(-W // s) > 64:
                raise ValueError(f"temporal_ensemble keeps ceil(act_window_size / multistep) = {-(-W // s)} plans per environment; at most 64")
        if sampler not in _VECTOR_SAMPLERS or extra_args:
            raise ValueError(f"VectorEnvPolicy supports the deterministic fused samplers {sorted(_VECTOR_SAMPLERS)} without extra_args; got "
                             f"sampler_type={sampler!r}, extra_args={extra_args!r}")
        if kw.get("generator") is not None:
            raise ValueError("VectorEnvPolicy draws its noise from per-environment streams: give seed= / reset(seeds=) instead of a generator")
        if not isinstance(getattr(denoiser, "inner_model", None), MoDeDiT):
            raise ValueError("VectorEnvPolicy needs a GCDenoiser over the HIP MoDeDiT")
        if not 1 <= int(num_envs) <= L.MODE_ENV_MAX:
            raise ValueError(f"num_envs must be in [1, {L.MODE_ENV_MAX}], got {num_envs}")
        self.num_envs = int(num_envs)
        self._counter = np.zeros(self.num_envs, dtype=np.int64)              # host mirror of the device counters: decides who replans
        self._warm = np.zeros(self.num_envs, dtype=np.bool_)                 # a plan was committed since the last reset: decides who replans warm
        super().__init__(denoiser, **kw)
        inner = denoiser.inner_model
        W, A = self.act_window_size, self.action_dim
        if (inner.action_seq_len, inner.action_dim) != (W, A):
            raise ValueError(f"act_window_size / action_dim ({W}, {A}) must be the model's action_seq_len / action_dim "
                             f"({inner.action_seq_len}, {inner.action_dim})")
        dev = next(inner.parameters()).device
        if dev.type != "cuda":
            raise ValueError("VectorEnvPolicy runs on a ROCm device: move the denoiser there first")
        self._solver = _VECTOR_SAMPLERS[sampler]
        n, self._nw = self.num_envs, (self.num_envs + 31) // 32
        self._plan = torch.zeros(n, W, A, dtype=torch.float32, device=dev)
        self._counter_dev = torch.zeros(n, dtype=torch.int32, device=dev)
        self._draws = torch.zeros(n, dtype=torch.int32, device=dev)          # uint32 bit patterns
        self._seeds = _u32_as_i32(range(seed, seed + n)).to(dev)
        nctrl = 4 + self._nw + n                                             # control block: include/mode_hip.h (ABI 13)
        self._sel, bid = None, None
        if self._ncand > 1:
            # candidate selection: the control block grows by the has-previous-plan bitmask behind the rows; the last selection per environment
            nctrl += self._nw
            self._selected = torch.full((n,), -1, dtype=torch.int32, device=dev)
            self._cand_scores = torch.zeros(n, self._ncand, dtype=torch.float32, device=dev)
            self._coh_w = torch.from_numpy(coherence_weights(self.coherence_decay, W - self.multistep)).to(dev)
            if self._nweak:
                # forward contrast: both terms of the last selection per environment, and the weight as the device scalar the kernel reads
                self._bc_scores = torch.zeros(n, self._nper, dtype=torch.float32, device=dev)
                self._fc_scores = torch.zeros(n, self._ncand, dtype=torch.float32, device=dev)
                self._lambda = torch.full((1,), self._contrast_weight, dtype=torch.float32, device=dev)
                bid = dict(lambda_=self._lambda, bc=self._bc_scores, fc=self._fc_scores, M=self._nweak, K=min(self.contrast_topk, 64))
        self._ctrl = torch.zeros(nctrl, dtype=torch.int32, device=dev)
        # pinned staging of the control block, a ring: a slot is rewritten only after the copy that read it has run (its event)
        self._ring = [torch.zeros(nctrl, dtype=torch.int32, pin_memory=True) for _ in range(4)]
        self._ring_ev = [torch.cuda.Event() for _ in self._ring]
        self._slot = 0
        self._scratch_out = torch.zeros(n, A, dtype=torch.float32, device=dev)
        self._desc = L.ModeEnvPoolDesc(num_envs=n, W=W, A=A, multistep=self.multistep, plan=self._plan.data_ptr(),
                                       counter=self._counter_dev.data_ptr(), draws=self._draws.data_ptr())
        if self._ncand > 1:
            self._sel = _select_desc(bid, rows=self._rows_ptr(), has_prev=self._rows_ptr() + 4 * n, count=self._ctrl, plan=self._plan, weights=self._coh_w,
                                     selected=self._selected, scores=self._cand_scores, num_envs=n, W=W, A=A, shift=self.multistep, N=self._ncand)
        self._ens = None
        if self.temporal_ensemble is not None:
            # the ring of each environment's last K plans with their birth times, the local times and the weight table: allocated here, once
            K = self.ensemble_depth = -(-W // self.multistep)
            try:
                self._ens_ring = torch.zeros(n, K, W, A, dtype=torch.float32, device=dev)
            except RuntimeError as e:                                        # (torch.OutOfMemoryError is one)
                raise ValueError(f"temporal_ensemble: cannot allocate the plan ring of {n} x {K} x {W} x {A} fp32 ({4 * n * K * W * A} bytes) on {dev}: {e}") from e
            self._ens_birth = torch.full((n, K), -1, dtype=torch.int32, device=dev)
            self._ens_t = torch.zeros(n, dtype=torch.int32, device=dev)
            self._ens_w = torch.from_numpy(ensemble_weights(self.temporal_ensemble, K)).to(dev)
            self._ens = L.ModeEnvEnsDesc(ring=self._ens_ring.data_ptr(), birth=self._ens_birth.data_ptr(), t=self._ens_t.data_ptr(),
                                         weights=self._ens_w.data_ptr(), K=K)
        self._lib = L.load()
        # the exports of this configuration, fixed here: (export, its name in an error) and, for the gathers, the arguments behind the common head
        # - those before a warm gather's sigma_start, those after it
        kind, per = ("_bid", (self._ncand, self._nweak)) if self._nweak else ("_cand", (self._ncand,)) if self._ncand > 1 else ("", ())
        self._gather_call = {False: ("mode_env_gather_noise" + kind, "env_gather_noise" + kind, (W * A, float(self.sigma_max)), per),
                             True: ("mode_env_gather_warm" + kind, "env_gather_warm" + kind, (self._plan.data_ptr(), W, A, self.multistep), per)}
        self._select_export, self._select_what = ("mode_env_select_bid", "env_select_bid") if self._nweak else ("mode_env_select", "env_select")
        self._commit_export, self._commit_what = ("mode_env_commit_emit", "env_commit_emit") if self._ens is None else \
            ("mode_env_commit_emit_ens", "env_commit_emit_ens")
        self._buckets = _buckets(n)
        self._templates = {}
        self._inputs = None
        self._enc_store = {}                                                # bucket -> gathered frame buffers + that bucket's encoder graph
        self._hooks = SimpleNamespace(store={}, prologue=self._gather, epilogue=self._commit, enc=self._enc_store)
        # warm chunks: a store of their own for the chunk graphs (an entry's key holds the schedule's length) and for the encoder graphs (an
        # entry's key holds the chunk entry's buffers), so that cold and warm chunks alternating at one bucket never recapture
        self._hooks_warm = SimpleNamespace(store={}, prologue=lambda ent: self._gather(ent, True), epilogue=self._commit, enc={})
        self.replanned, self.replanned_warm = [], []

    # ---------------------------------------------------------------------------------------------------------------- host-side bookkeeping
    def _env_index(self, envs) -> np.ndarray:
        n = self.num_envs
        if envs is None:
            return np.arange(n)
        if torch.is_tensor(envs):
            if envs.device.type != "cpu":
                raise ValueError("envs must be host indices or a host mask")
            envs = envs.numpy()
        a = np.asarray(envs)
        if a.dtype == np.bool_:
            if a.shape != (n,):
                raise ValueError(f"an environment mask must have shape ({n},), got {a.shape}")
            return np.flatnonzero(a)
        a = a.astype(np.int64).reshape(-1)
        if a.size and (a.min() < 0 or a.max() >= n or len(np.unique(a)) != a.size):
            raise ValueError(f"environment indices must be distinct and in [0, {n}), got {a.tolist()}")
        return a

    def _active_mask(self, active) -> np.ndarray:
        n = self.num_envs
        if active is None:
            return np.ones(n, dtype=np.bool_)
        if torch.is_tensor(active):
            if active.device.type != "cpu":
                raise ValueError("active must be a HOST mask (numpy / list / CPU tensor): a device mask would need a host sync per step")
            active = active.numpy()
        a = np.asarray(active)
        if a.dtype != np.bool_ or a.shape != (n,):
            raise ValueError(f"active must be a bool mask of shape ({n},), got {a.dtype} {a.shape}")
        return a

    def _active_words(self, act: np.ndarray) -> np.ndarray:
        return _mask_words(act, self._nw)

    def reset(self, envs=None, seeds=None) -> None:
        """Start a new episode in the listed environments (see the class docstring)."""
        idx = self._env_index(envs)
        self._counter[idx] = 0
        self._warm[idx] = False
        if seeds is not None:
            seeds = list(seeds)
            if len(seeds) != len(idx):
                raise ValueError(f"one seed per listed environment: {len(idx)} environments, {len(seeds)} seeds")
        if not len(idx) or (seeds is None and self._ens is None):
            return
        dev = self._seeds.device
        i = torch.from_numpy(idx).pin_memory().to(dev, non_blocking=True)
        if self._ens is not None:                                            # no plan from before the reset is live again, local time 0
            self._ens_birth[i] = -1
            self._ens_t[i] = 0
        if seeds is not None:
            self._seeds[i] = _u32_as_i32(seeds).pin_memory().to(dev, non_blocking=True)
            self._draws[i] = 0

    @property
    def plans(self) -> torch.Tensor:
        """[num_envs, act_window_size, action_dim] every environment's current plan (device)."""
        return self._plan

    @property
    def draws(self) -> torch.Tensor:
        """[num_envs] int32 (uint32 bit patterns): the draw index each environment's next replan takes (device)."""
        return self._draws

    def _cand_state(self, name: str) -> torch.Tensor:
        if self._sel is None:
            raise AttributeError("this policy was built without candidates (or with candidates=1): every replan draws one plan")
        return getattr(self, name)

    @property
    def selected(self) -> torch.Tensor:
        """[num_envs] int32: the candidate chosen at every environment's last replan, -1 before any (device, ``candidates`` only)."""
        return self._cand_state("_selected")

    @property
    def candidate_scores(self) -> torch.Tensor:
        """[num_envs, candidates] fp32: the scores of every environment's last replan (device, ``candidates`` only); with ``contrast`` the totals
        ``bc + contrast_weight * fc`` the selection minimised."""
        return self._cand_state("_cand_scores")

    def _contrast_state(self, name: str) -> torch.Tensor:
        if not self._nweak:
            raise AttributeError("this policy was built without contrast: its selection has the backward-coherence term only (candidate_scores)")
        return getattr(self, name)

    @property
    def coherence_scores(self) -> torch.Tensor:
        """[num_envs, candidates + contrast] fp32: the backward-coherence term of every candidate, strong ones first, at every environment's last
        replan (device, ``contrast`` only; ``candidate_scores`` then holds the total)."""
        return self._contrast_state("_bc_scores")

    @property
    def contrast_scores(self) -> torch.Tensor:
        """[num_envs, candidates] fp32: the forward-contrast term of the strong candidates at every environment's last replan (device, ``contrast``
        only)."""
        return self._contrast_state("_fc_scores")

    @staticmethod
    def _checked_contrast_weight(value) -> float:
        return _checked_float(value, 0.0, float("inf"), f"contrast_weight must be a finite float >= 0, got {value!r}")

    @property
    def contrast_weight(self) -> Optional[float]:
        """The weight lambda of the forward-contrast term in ``total = bc + lambda * fc`` (None without ``contrast``).  Settable: the new value is
        written into the device scalar the selection kernel reads, so the next replan uses it - no graph is captured again, no graph key holds it."""
        return self._contrast_weight

    @contrast_weight.setter
    def contrast_weight(self, value) -> None:
        if not self._nweak:
            raise AttributeError("this policy was built without contrast: there is no forward-contrast term to weigh")
        self._contrast_weight = self._checked_contrast_weight(value)
        self._lambda.fill_(self._contrast_weight)

    def _ens_state(self, name: str) -> torch.Tensor:
        if self._ens is None:
            raise AttributeError("this policy was built without temporal_ensemble: it keeps one plan per environment (plans)")
        return getattr(self, name)

    @property
    def plan_ring(self) -> torch.Tensor:
        """[num_envs, ensemble_depth, act_window_size, action_dim] the last plans of every environment (device, ``temporal_ensemble`` only): a plan
        born at local time t_p is in slot ``(t_p // multistep) % ensemble_depth``."""
        return self._ens_state("_ens_ring")

    @property
    def plan_births(self) -> torch.Tensor:
        """[num_envs, ensemble_depth] int32: the local time at which each ring slot's plan was born, -1 = empty (device)."""
        return self._ens_state("_ens_birth")

    @property
    def local_times(self) -> torch.Tensor:
        """[num_envs] int32: every environment's local time, its active steps since its last reset (device)."""
        return self._ens_state("_ens_t")

    @property
    def ensemble_weight_table(self) -> torch.Tensor:
        """[ensemble_depth] fp32: ``ensemble_weights(temporal_ensemble, ensemble_depth)`` as the kernel reads it (device)."""
        return self._ens_state("_ens_w")

    def _check_inputs(self, perceptual_emb: Dict, latent_goal: torch.Tensor):
        """Shape / device contract of the inputs: host metadata only (the rows are read by the gather launches, and only those that replan).
        Returns (state_images or None, latent_goal, (rgb_static, rgb_gripper) or None)."""
        inner = self.model.inner_model
        n = self.num_envs
        if not isinstance(perceptual_emb, dict):
            raise ValueError("perceptual_emb must be a dict: {'state_images': ...} or {'rgb_obs': {...}}")
        if "state_images" in perceptual_emb and "rgb_obs" in perceptual_emb:
            raise ValueError("give either embedded observations ('state_images') or raw camera frames ('rgb_obs'), not both")
        frames = None
        if "state_images" not in perceptual_emb:
            if "rgb_obs" not in perceptual_emb or self.encoders is None:
                raise ValueError("VectorEnvPolicy.step takes embedded observations {'state_images': (num_envs, n_img, obs_dim)}: embed raw camera "
                                 "frames first (policy.embed(obs, latent_goal) with the policy's perceptual encoders), or build the policy with "
                                 "static_resnet / gripper_resnet to pass {'rgb_obs': ...}")
            frames = self._check_frames(perceptual_emb["rgb_obs"])
            img = None
        else:
            img = perceptual_emb["state_images"]
            want = (n, inner.n_img_tokens, inner.obs_dim)
            if not torch.is_tensor(img) or tuple(img.shape) != want:
                raise ValueError(f"state_images must be {want} (one row per environment), got {tuple(getattr(img, 'shape', ()))}")
        gl = latent_goal
        if not torch.is_tensor(gl) or gl.shape[0] != n or gl.reshape(n, -1).shape[1] != inner.goal_dim or gl.dim() not in (2, 3):
            raise ValueError(f"latent_goal must be ({n}, {inner.goal_dim}) or ({n}, 1, {inner.goal_dim}), got {tuple(getattr(gl, 'shape', ()))}")
        dev = self._plan.device
        if (img is not None and img.device != dev) or gl.device != dev:
            raise ValueError(f"state_images and latent_goal must be on {dev}")
        return img, gl, frames

    def _frames_device(self) -> torch.device:
        return self._plan.device

    def _check_frames(self, rgb):
        """The raw observation's contract: both cameras, (num_envs, T, 3, H, W) each with one T, 2 T = n_img_tokens, fp32 or bf16, on the
        policy's device.  An environment's frames must be one contiguous block (the environments may lie at any pitch): other layouts are
        made so here."""
        if getattr(self, "camera_transforms", None) is not None:
            return self._check_u8_frames(rgb, self.num_envs)
        n = self.num_envs

        def camera(name, f):
            if not torch.is_tensor(f) or f.dim() != 5 or f.shape[0] != n or f.shape[2] != 3 or f.numel() == 0:
                raise ValueError(f"{name} must be ({n}, T, 3, H, W) (one row per environment), got {tuple(getattr(f, 'shape', ()))}")
            if f.dtype not in (torch.float32, torch.bfloat16):
                raise ValueError(f"{name} must be float32 or bfloat16, got {f.dtype}")
            if f.device != self._plan.device:
                raise ValueError(f"{name} must be on {self._plan.device}, got {f.device}")
            return f
        out = self._check_cameras(rgb, camera, "number of frames T", lambda f: f.shape[1])
        return tuple(f if f[0].is_contiguous() and (n == 1 or f.stride(0) >= f[0].numel()) else f.contiguous() for f in out)

    # ---------------------------------------------------------------------------------------------------------------- device side
    def _stage(self, m: int, rows: np.ndarray, act: np.ndarray, out_ptr: int) -> None:
        """Fill the next pinned slot with the control block and copy it to the device block the gather and the graphs read."""
        i = self._slot
        self._slot = (i + 1) % len(self._ring)
        self._ring_ev[i].synchronize()            # the copy that last read this slot: done long ago unless the host ran 4 replans ahead
        buf = self._ring[i].numpy()
        nw = self._nw
        buf[0], buf[1] = m, 0
        buf[2:4] = np.array([out_ptr], dtype="<u8").view("<i4")
        buf[4:4 + nw] = self._active_words(act).view("<i4")
        buf[4 + nw:4 + nw + len(rows)] = rows
        if self._sel is not None:                 # who has a plan to be coherent with: committed since its last reset, as of before this step
            buf[4 + nw + self.num_envs:] = _mask_words(self._warm, nw).view("<i4")
        self._ctrl.copy_(self._ring[i], non_blocking=True)
        self._ring_ev[i].record()

    def _gather(self, ent, warm: bool = False) -> None:
        """Chunk prologue: the listed environments' observations, goals and initial latents into the entry's input buffers (one launch) - the
        noise of a cold replan, or (``warm``) the latents of ``env_warm_latents``: their plans advanced by ``multistep`` rows and noised to
        ``sigmas[warm_start]``.  Raw frames: the goals and the latents (one launch), the frames (one launch), then the encoders of the chunk's
        kind into the entry's observation buffer."""
        from . import _lib as L
        from .engine import _stream
        img, gl, frames = self._inputs
        inner = self.model.inner_model
        x = ent["bufs"][0]
        N = self._nper
        rows = (self._rows_ptr(), x.shape[0] // N, self.num_envs, self._seeds.data_ptr(), self._draws.data_ptr(),
                None if img is None else img.data_ptr(), inner.n_img_tokens * inner.obs_dim, gl.data_ptr(), inner.goal_dim,
                None if img is None else ent["img"].data_ptr(), ent["goals"].data_ptr(), x.data_ptr())
        if N > 1 and "chosen" not in ent:                                    # (candidates, a new entry: this call is ahead of its capture)
            ent["chosen"] = torch.zeros(x.shape[0] // N, *x.shape[1:], dtype=torch.float32, device=x.device)
        export, what, pre, post = self._gather_call[warm]
        mid = (self._warm_schedule(x.device)[1],) if warm else ()
        L.check(getattr(self._lib, export)(*rows, *pre, *mid, *post, _stream()), what)
        if frames is not None:
            self._encode(ent, frames, (self._hooks_warm if warm else self._hooks).enc)

    def _warm_schedule(self, dev):
        """(``sigmas[warm_start:]``, ``float(sigmas[warm_start])``) of a warm replan, built once per device (one host read): the schedule is a
        contiguous clone handed to the sampler as the SAME object every call, like ``_schedule``'s, so that it is recognised without a compare."""
        cached = getattr(self, "_sigmas_warm", None)
        if cached is None or cached[0].device != torch.device(dev):
            sub = self._schedule(dev)[self.warm_start:].contiguous().clone()
            cached = self._sigmas_warm = (sub, float(sub[0]))
        return cached

    def _rows_ptr(self) -> int:
        return self._ctrl.data_ptr() + 4 * (4 + self._nw)

    def _frame_dtypes(self, frames):
        """Element type of the gathered frames: bf16 under bf16 autocast (the stem rounds an fp32 image to bf16 as it reads it, so converting in
        the gather is exact and halves the stem's reads), else the frames' own."""
        ac = self.encoders.autocast_dtype
        if ac == torch.bfloat16:
            return (torch.bfloat16,) * len(frames)
        return tuple(torch.float32 if self.camera_transforms is not None else f.dtype for f in frames)   # (uint8 camera frames: fp32 out)

    def _gather_frames(self, mb: int, frames, bufs) -> None:
        """frames[rows[j]] -> bufs[j] for j < mb, both cameras in one launch (csrc/env_pool.hip)."""
        from . import _lib as L
        from .engine import _stream
        if self.camera_transforms is not None:                              # the cameras' uint8 frames: resized and normalised on the way
            from .camera import launch
            launch([(t, f, b, None) for t, f, b in zip(self._transform_pair(), frames, bufs)], self._rows_ptr(), mb, self.num_envs)
            return
        d = L.ModeEnvFramesDesc(rows=self._rows_ptr(), m_b=mb, num_envs=self.num_envs)
        dt = {torch.float32: L.MODE_F32, torch.bfloat16: L.MODE_BF16}
        for k, (f, b) in enumerate(zip(frames, bufs)):
            d.cam[k] = L.ModeEnvFramesCam(src=f.data_ptr(), src_stride=f.stride(0) if f.shape[0] > 1 else f[0].numel(), row_elems=f[0].numel(),
                                          dst=b.data_ptr(), src_dtype=dt[f.dtype], dst_dtype=dt[b.dtype])
        L.check(self._lib.mode_env_gather_frames(C.byref(d), _stream()), "env_gather_frames")

    def _encode(self, ent, frames, store) -> None:
        """The bucket's encoders on the gathered frames, FiLM-conditioned on the gathered goals, into ``ent['img']``: a replay of the bucket's
        encoder graph (captured on first use, and again when the frame geometry, the weights' storage or the chunk entry's buffers moved), or
        the eager towers when the encoders are in training mode / MODE_HIP_GRAPH=0.  ``store``: the encoder store of the chunk's kind."""
        enc = self.encoders
        N = self._nper                                                      # (forward contrast: the weak rows share the embeddings too)
        mb, n_img = ent["goals"].shape[0] // N, self.model.inner_model.n_img_tokens
        dts = self._frame_dtypes(frames)
        shapes = [tuple(f.shape[1:]) for f in frames]                      # of one environment's gathered frames
        if self.camera_transforms is not None:
            shapes = [t.out_shape(f.shape)[1:] for t, f in zip(self._transform_pair(), frames)]
        geom = tuple((tuple(f.shape[1:]), shp, dt) for f, shp, dt in zip(frames, shapes, dts))   # (source H, W included: the kernel's tables)
        st = store.get(mb)
        if st is None or st["geom"] != geom:
            st = store[mb] = dict(geom=geom, graph=None,
                                            bufs=tuple(torch.empty(mb, *shp, dtype=dt, device=f.device) for f, shp, dt in zip(frames, shapes, dts)))
        self._gather_frames(mb, frames, st["bufs"])
        goals, img = ent["goals"], ent["img"]
        if N == 1:
            towers = lambda: img.copy_(enc._eager(st["bufs"][0], st["bufs"][1], goals).view(mb, n_img, -1))
        else:
            # candidates: the towers run once per environment at batch mb * T, FiLM on a contiguous copy of the mb goal rows (the first of each
            # environment's N); the mb embedding rows are then broadcast to the environment's N candidate rows
            def towers():
                emb = enc._eager(st["bufs"][0], st["bufs"][1], goals.view(mb, N, -1)[:, 0].contiguous())
                img.view(mb, N, n_img, -1).copy_(emb.view(mb, 1, n_img, -1).expand(mb, N, n_img, -1))
        if enc.static_resnet.training or enc.gripper_resnet.training or not graphs_enabled():
            towers()
            return
        wdt = enc.autocast_dtype if enc.autocast_dtype is not None else dts[0]
        key = (wdt, enc._param_key(), ent["img"].data_ptr(), goals.data_ptr())
        if st["graph"] is None or st["key"] != key:
            st["graph"] = None                                              # (the old graph's pool goes before the new capture)
            st["graph"], _, st["tables"] = enc.capture(towers, img.device, wdt)
            st["key"] = key
        enc._refresh(wdt)                                                   # weights whose version moved since the last replan: re-cast in place
        st["graph"].replay()

    def _commit(self, ent, capturing: bool) -> None:
        """Chunk epilogue: commit + emit reading the device control block.  Outside a capture (the warm-up run) the same kernel runs with no
        replan and no active environment into a scratch row block: it loads the code object and changes nothing."""
        d = type(self._desc).from_buffer_copy(self._desc)
        d.chunk = ent["bufs"][0].data_ptr()
        if self._sel is not None:
            # candidates: between the chain and the commit, the selection of each real row's most coherent candidate into the entry's
            # ``chosen`` rows, which the commit then takes for the chunk.  It reads the control block in the warm-up run too: there it writes,
            # for the rows staged, what the replay writes again (no row when ``warmup`` staged none).
            from . import _lib as L
            from .engine import _stream
            sel = type(self._sel).from_buffer_copy(self._sel)
            sel.chunk, sel.chosen, sel.m_b = d.chunk, ent["chosen"].data_ptr(), ent["chosen"].shape[0]
            L.check(getattr(self._lib, self._select_export)(C.byref(sel), _stream()), self._select_what)
            d.chunk = sel.chosen
        if capturing:
            d.ctrl = self._ctrl.data_ptr()
        else:
            d.out = self._scratch_out.data_ptr()
        self._launch(d)

    def _launch(self, d) -> None:
        from . import _lib as L
        from .engine import _stream
        if self._ens is not None:                                            # temporal ensembling: the same step on the ring of plans
            e = type(self._ens).from_buffer_copy(self._ens)
            e.pool = d
            d = e
        L.check(getattr(self._lib, self._commit_export)(C.byref(d), _stream()), self._commit_what)

    def _run_chunk(self, mb: int, m: int, warm: bool = False) -> None:
        """One replanning chunk at bucket ``mb`` with ``m`` real rows (the control block is staged): gather launch + one replay.  ``warm``: the
        warm-started chunk - the warm gather, the schedule from ``warm_start`` on, the warm chunks' stores."""
        inner = self.model.inner_model
        eng = inner.engine
        if self.need_precompute_experts_for_inference:
            if not inner._routes_per_chunk():                               # goal / token routing resolve their routing inside the chunk
                self.precompute_expert_for_inference()
            self.need_precompute_experts_for_inference = False
        sig = self._warm_schedule(eng.device)[0] if warm else self._schedule(eng.device)
        tpl = self._templates.get(mb)
        if tpl is None:
            dev, B = eng.device, mb * self._nper                            # (candidates: N (+ M weak) chunk rows per environment)
            tpl = self._templates[mb] = ({"state_images": torch.zeros(B, inner.n_img_tokens, inner.obs_dim, device=dev)},
                                         torch.zeros(B, self.act_window_size, self.action_dim, device=dev), torch.zeros(B, inner.goal_dim, device=dev))
        w = getattr(self.model, "guidance_scale", None)                  # classifier-free guidance: the bucket's mb rows run as 2·mb inside the chain
        gkey, plan = inner._chunk_plan(eng, self._solver, sig.numel() - 1, w is not None)
        inner._sample_chunk(eng, gkey, plan, tpl[0], tpl[1], tpl[2], sig, float(self.model.sigma_data),
                            hooks=self._hooks_warm if warm else self._hooks, rows=m * self._nper, guidance=w)

    @staticmethod
    def _prepared(img, gl, frames):
        """What the gather launches read: fp32 contiguous observation and goal rows; frames as checked."""
        return (None if img is None else img.to(torch.float32).contiguous()), gl.to(torch.float32).contiguous(), frames

    @torch.no_grad()
    def warmup(self, perceptual_emb: Dict, latent_goal: torch.Tensor) -> None:
        """Capture the chunk of every bucket now - with raw frames also every bucket's encoder graph - (the inputs give valid rows for the capture
        runs); the policy's state does not change."""
        self.model.eval()
        self._inputs = self._prepared(*self._check_inputs(perceptual_emb, latent_goal))
        none = np.zeros(self.num_envs, dtype=np.bool_)
        for mb in self._buckets:
            for warm in (False, True) if self.warm_start is not None else (False,):
                self._stage(0, np.zeros(mb, dtype=np.int32), none, self._scratch_out.data_ptr())
                self._run_chunk(mb, 0, warm)
        self._inputs = None

    @torch.no_grad()
    def step(self, perceptual_emb: Dict, latent_goal: torch.Tensor, active=None) -> torch.Tensor:
        if self.model.training or self.model.inner_model.training:       # (eval() walks every submodule: not on every step)
            self.model.eval()
        inputs = self._check_inputs(perceptual_emb, latent_goal)
        act = self._active_mask(active)
        rows = np.flatnonzero(act & (self._counter == 0)).astype(np.int32)
        m = len(rows)
        out = torch.empty(self.num_envs, self.action_dim, dtype=torch.float32, device=self._plan.device)
        warm = rows[self._warm[rows]] if self.warm_start is not None else rows[:0]
        if m:
            # one chunk per kind of replanner.  With both kinds the cold chunk goes first, staged with no active environment and the scratch
            # output: its launch commits its plans and emits nothing; the warm chunk's launch then emits the whole step, the cold ones from plans
            cold = rows[~self._warm[rows]] if len(warm) else rows
            chunks = [(r, w) for r, w in ((cold, False), (warm, True)) if len(r)]
            none = np.zeros(self.num_envs, dtype=np.bool_)
            self._inputs = self._prepared(*inputs)
            try:
                for i, (r, w) in enumerate(chunks):
                    last = i == len(chunks) - 1
                    mb = next(b for b in self._buckets if b >= len(r))
                    self._stage(len(r), np.concatenate([r, np.full(mb - len(r), r[-1], dtype=np.int32)]), act if last else none,
                                out.data_ptr() if last else self._scratch_out.data_ptr())
                    self._run_chunk(mb, len(r), w)
            finally:
                self._inputs = None
        else:
            d = type(self._desc).from_buffer_copy(self._desc)
            d.out = out.data_ptr()
            words = self._active_words(act)
            C.memmove(d.active, words.ctypes.data, 4 * self._nw)
            self._launch(d)
        self._counter[act] = (self._counter[act] + 1) % self.multistep
        self._warm[rows] = True
        self.replanned, self.replanned_warm = rows.tolist(), warm.tolist()
        return out


def _read_checkpoint_file(path: str, trust_pickle: bool = False) -> Dict[str, torch.Tensor]:
    """The file forms `MoDEAgent.load_pretrained_parameters` accepts (mode_agent.py:141-158): a checkpoint DIRECTORY holding
    ``model_cleaned.safetensors`` (preferred) or ``model_cleaned.pt``; a ``.safetensors`` file; a Lightning ``.ckpt`` / ``torch.save``d dict whose
    weights sit under ``'state_dict'`` (a bare state_dict is accepted too).  Lightning checkpoints carry hyper-parameter objects, which torch >= 2.6
    refuses under its ``weights_only=True`` default: the safe load is tried first and the full unpickler only after it fails - the reference
    (torch 2.2) always unpickles; load only checkpoints you trust."""
    if os.path.isdir(path):
        st, pt = os.path.join(path, "model_cleaned.safetensors"), os.path.join(path, "model_cleaned.pt")
        if os.path.exists(st):
            path = st
        elif os.path.exists(pt):
            path = pt
        else:
            raise FileNotFoundError(f"No cleaned weights found in {path}")     # the reference's message (mode_agent.py:155)
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    try:
        blob = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as safe_err:                                               # pickle.UnpicklingError and friends: non-tensor objects in the file
        # Full unpickling executes whatever the file says: only on the caller's explicit say-so (Lightning checkpoints carry omegaconf objects and need it;
        # the reference's own loader, mode_agent.py:135-160, reads the cleaned tensor files above, which never get here)
        if not (trust_pickle or os.environ.get("MODE_TRUST_CKPT", "0") == "1"):
            raise RuntimeError(f"cannot read checkpoint {path} with weights_only=True ({safe_err!r}); pass trust_pickle=True / set MODE_TRUST_CKPT=1 to allow "
                               "full unpickling of a file you trust") from safe_err
        import warnings
        warnings.warn(f"loading {path} with the full unpickler (trusted by the caller)")
        try:
            blob = torch.load(path, map_location="cpu", weights_only=False)
        except Exception as e:
            raise RuntimeError(f"cannot read checkpoint {path}: weights_only load failed with {safe_err!r}, full unpickling with {e!r}") from e
    return blob.get("state_dict", blob) if isinstance(blob, dict) else blob


def load_denoiser_checkpoint(model, source, prefix: str = "model.inner_model.", strict: bool = False, trust_pickle: bool = False):
    """Load the denoiser's tensors from an agent checkpoint: a ``.safetensors`` file (the published HF weights), a ``torch.save``d
    ``state_dict`` / Lightning checkpoint, or an in-memory mapping.  Keys are matched by name after stripping the agent's prefix
    (``model.inner_model.`` — mode_agent.py:209-251 loads by key and skips the CLIP / ResNet tensors, which belong to the out-of-scope
    encoders); the kernel-side layout is untouched because the Parameters are arena views.  Returns (missing, unexpected, skipped_shape)."""
    if isinstance(source, (str, bytes, os.PathLike)):
        sd = _read_checkpoint_file(os.fsdecode(source), trust_pickle)
    else:
        sd = dict(source)
    own = model.state_dict()
    picked, skipped = {}, []
    for key, t in sd.items():
        if "visual" in key or "clip" in key.lower():
            continue
        name = key[len(prefix):] if key.startswith(prefix) else key
        if name not in own:
            continue
        if tuple(own[name].shape) != tuple(t.shape):
            if own[name].numel() == t.numel():
                t = t.reshape(own[name].shape)
            else:
                skipped.append(name)
                continue
        picked[name] = t
    res = model.load_state_dict(picked, strict=strict)
    return list(res.missing_keys), list(res.unexpected_keys), skipped


# Key prefixes of older published checkpoints -> the agent's current attribute names (mode_agent.py:216-226).  Tried in this order, first match wins,
# and only for keys the agent does not have under their own name.
_AGENT_KEY_REMAP = (
    ("img_encoder_image_wrist.", "gripper_resnet."),
    ("img_encoder_image_secondary.", "static_resnet."),
    ("img_encoder_image_primary.", "static_resnet."),
    ("net.", "gripper_resnet.resnet."),
)


def _fit_checkpoint_tensor(key: str, t: torch.Tensor, shape) -> Optional[torch.Tensor]:
    """The reference loader's shape rule (mode_agent.py:163-200): equal shapes pass; a 0-d entry becomes zeros; 1-d -> 1-d of another length is tiled
    (BatchNorm vectors); 1-d or 2-d -> 4-d with the same element count is viewed as the convolution weight; ``running_*`` buffers of another rank
    with the same element count are viewed; anything else is incompatible (None)."""
    shape = tuple(shape)
    if tuple(t.shape) == shape:
        return t
    want = 1
    for d in shape:
        want *= d
    if t.dim() == 0:
        return torch.zeros(shape, device=t.device)
    if t.dim() == 1 and len(shape) == 1:
        return t.repeat(shape[0] // t.shape[0]) if t.shape[0] != shape[0] else t
    if t.dim() == 1 and len(shape) == 4:
        return t.view(shape)                                                   # raises on an element-count mismatch, like the reference
    if t.dim() == 2 and len(shape) == 4 and t.numel() == want:
        return t.view(shape)
    if "running_" in key and t.dim() != len(shape) and t.numel() == want:
        return t.view(shape)
    return None


def _agent_parts(target) -> Dict[str, torch.nn.Module]:
    """{'model': GCDenoiser, 'static_resnet': ..., 'gripper_resnet': ...} from a mapping, a ChunkedRolloutPolicy, or any object with those attributes
    (the attribute names ARE the key prefixes of the agent's state_dict, mode_agent.py:79, 90-91)."""
    if isinstance(target, dict):
        parts = dict(target)
    else:
        parts = {"model": getattr(target, "model", None)}
        enc = getattr(target, "encoders", None)
        for name in ("static_resnet", "gripper_resnet"):
            parts[name] = getattr(target, name, None) if getattr(target, name, None) is not None else getattr(enc, name, None)
    parts = {k: v for k, v in parts.items() if v is not None}
    if not parts:
        raise ValueError("nothing to load into: expected 'model' and / or 'static_resnet' / 'gripper_resnet'")
    return parts


def load_agent_checkpoint(target, source, strict: bool = False, verbose: bool = False, trust_pickle: bool = False) -> Dict[str, object]:
    """Load ONE agent checkpoint - the published HF ``.safetensors``, a Lightning ``.ckpt`` / ``torch.save``d ``state_dict`` or a mapping - into the
    denoiser AND both perceptual encoders, as ``MoDEAgent.load_pretrained_parameters`` does (mode_agent.py:135-251): CLIP tensors are skipped
    (``'visual'`` / ``'clip'`` in the key), keys the agent does not know are retried under the prefix table of older releases
    (``img_encoder_image_wrist.`` -> ``gripper_resnet.``, ``img_encoder_image_primary.`` / ``secondary.`` -> ``static_resnet.``, ``net.`` ->
    ``gripper_resnet.resnet.``), tensors are fitted by the reference's reshape rule, incompatible ones are skipped and reported, and the result is
    loaded with ``load_state_dict(strict=strict)``.

    ``target``: ``{'model': GCDenoiser, 'static_resnet': m, 'gripper_resnet': m}`` (any subset), a ``ChunkedRolloutPolicy`` built with encoders, or an
    object with those attributes.  Returns ``{'direct', 'reshaped', 'skipped', 'missing', 'unexpected'}`` (counts for the first two, key lists for the
    rest; keys carry the agent-level prefix).  Parameters are written in place (arena views, the graphs' static pointers stay valid).

    Files are read with ``weights_only=True``; a file that needs the full unpickler (a Lightning ``.ckpt`` with omegaconf / argparse objects next to the weights)
    is only read on the caller's say-so - ``trust_pickle=True`` or ``MODE_TRUST_CKPT=1`` - because unpickling executes what the file says."""
    if isinstance(source, (str, bytes, os.PathLike)):
        sd = _read_checkpoint_file(os.fsdecode(source), trust_pickle)
    else:
        sd = dict(source)
    parts = _agent_parts(target)
    current = {f"{name}.{k}": v for name, mod in parts.items() for k, v in mod.state_dict().items()}
    picked: Dict[str, Dict[str, torch.Tensor]] = {name: {} for name in parts}
    direct, reshaped, skipped = 0, 0, []
    for key, t in sd.items():
        if "visual" in key or "clip" in key.lower():
            continue
        tkey = key
        if key not in current:
            for old, new in _AGENT_KEY_REMAP:
                if key.startswith(old):
                    tkey = key.replace(old, new)
                    break
        if tkey not in current:
            continue                                                           # the reference drops unknown keys before load_state_dict too
        fitted = _fit_checkpoint_tensor(tkey, t, current[tkey].shape)
        if fitted is None:
            skipped.append(tkey)
            if verbose:
                print(f"Skipping incompatible tensor {tkey}: checkpoint {tuple(t.shape)} vs {tuple(current[tkey].shape)}")
            continue
        if tuple(fitted.shape) != tuple(t.shape):
            reshaped += 1
        else:
            direct += 1
        name, sub = tkey.split(".", 1)
        picked[name][sub] = fitted
    missing, unexpected = [], []
    from .perceptual_encoders import invalidate_conv_shadows
    for name, mod in parts.items():
        res = mod.load_state_dict(picked[name], strict=strict)
        invalidate_conv_shadows(mod)                                             # cached compute-dtype conv weights are re-cast on next use, whatever the loader's write path
        missing += [f"{name}.{k}" for k in res.missing_keys]
        unexpected += [f"{name}.{k}" for k in res.unexpected_keys]
    if verbose:
        print(f"Direct copies: {direct}  reshaped: {reshaped}  skipped: {len(skipped)}  missing: {len(missing)}")
    return {"direct": direct, "reshaped": reshaped, "skipped": skipped, "missing": missing, "unexpected": unexpected}
