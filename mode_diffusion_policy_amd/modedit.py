"""Drop-in mirror of the reference's ``mode.models.networks.modedit`` for the denoising path.

Same constructor keys (conf/model/mode_agent.yaml:46-76), same ``forward(states, actions, goals, sigma, uncond)`` signature
(modedit.py:741-809), same ``state_dict`` key set and the same side-channel attributes the agent reaches
through (``blocks``, ``logits_per_layer``, ``probs_per_layer``, expert-usage counters, ``freeze_router`` …) — but the module
tree below only HOLDS parameters; every FLOP of ``forward`` runs in the HIP library (``engine.DitEngine``).
There is no CPU / eager fallback: calling ``forward`` without the library or off-device raises.
"""
from __future__ import annotations

import logging
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib as L
from .engine import DitEngine, graphs_enabled, warm_and_capture

logger = logging.getLogger(__name__)


def _f32(t, dev):
    """A call's tensor as the launch chain reads it: fp32, contiguous, on the engine's device (the tensor itself when it already is all that)."""
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _edm_rows(s, sigma_data: float, next=None, ms=None):
    """The rows the chain reads per noise level ``s`` [n] (score_wrappers.py:31-43): c_in [n] and scal [n, 4] = [c_skip, c_out, s'/s, ms] - ``next``: the
    level each step goes to (DDIM's update, 0 without), ``ms``: the two-point multistep weight (``_dpmpp_2m_weights``, 0 without)."""
    s2 = s * s + sigma_data ** 2
    c_in = (1.0 / s2.sqrt()).contiguous()
    return c_in, torch.stack([sigma_data ** 2 / s2, s * sigma_data / s2.sqrt(), torch.zeros_like(s) if next is None else next / s,
                              torch.zeros_like(s) if ms is None else ms], 1).contiguous()


class _Eval(NamedTuple):
    """One denoiser evaluation of a captured chunk (``_chunk_steps``): ids into the chunk's [B, A_len, A_dim] buffers (None = not passed) and whether
    the head applies the schedule's linear update ``sched["lin"][j]`` (two-stage solvers, ModeHeadDesc.lin) instead of DDIM's (scal[2], with scal[3]
    weighing ``den_prev`` for two-point multistep solvers, ModeHeadDesc.den_prev).  No sigma, no coefficient: a list of these is a buffer PATTERN."""
    x_in: int
    x_out: int
    den_out: Optional[int] = None
    den_prev: Optional[int] = None
    aux1: Optional[int] = None
    aux2: Optional[int] = None
    lin: bool = False


class _Holder(nn.Module):
    """Parameter container; its own forward is never part of the product path."""

    def forward(self, *a, **k):  # pragma: no cover
        raise L.ModeHipUnavailable("parameter holder: the MoDE denoiser only runs through the HIP engine")


class RMSNorm(_Holder):
    """gain ``g`` of x / max(||x||·dim^-1/2, eps) · g  (modedit.py:72-80)."""

    def __init__(self, dim: int, eps: float = 1e-8):
        super().__init__()
        self.scale, self.eps = dim ** -0.5, eps
        self.g = nn.Parameter(torch.ones(dim))


class SwishGLU(_Holder):
    """``project`` = Linear(in, 2*out): first half value, second half gate (modedit.py:83-90)."""

    def __init__(self, in_dim: int, out_dim: int):
        super().__init__()
        self.project = nn.Linear(in_dim, 2 * out_dim)


class Mlp(_Holder):
    """Expert MLP holder: mlp.0 = SwishGLU(D,4D), mlp.2 = Linear(4D,D,no bias) (modedit.py:220-265)."""

    def __init__(self, n_embd: int, bias: bool = False, dropout: float = 0.0):
        super().__init__()
        self.mlp = nn.Sequential(SwishGLU(n_embd, 4 * n_embd), nn.Dropout(dropout), nn.Linear(4 * n_embd, n_embd, bias=bias))


class Attention(_Holder):
    """q/k/v Linear(+bias), c_proj (no bias), qk-RMSNorm gains (modedit.py:94-129)."""

    def __init__(self, n_embd: int, n_head: int, attn_pdrop: float):
        super().__init__()
        assert n_embd % n_head == 0
        self.key = nn.Linear(n_embd, n_embd)
        self.query = nn.Linear(n_embd, n_embd)
        self.value = nn.Linear(n_embd, n_embd)
        self.c_proj = nn.Linear(n_embd, n_embd, bias=False)
        self.q_norm = RMSNorm(n_embd // n_head, eps=1e-6)
        self.k_norm = RMSNorm(n_embd // n_head, eps=1e-6)
        self.n_head, self.n_embd, self.attn_pdrop = n_head, n_embd, attn_pdrop


class CondRouterMLP(_Holder):
    """Linear(D,2D) -> GELU -> Dropout(0) -> Linear(2D,E), init N(0,0.02)/zero bias (modedit.py:170-217)."""

    def __init__(self, n_embd: int, num_experts: int):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(n_embd, 2 * n_embd), nn.GELU(), nn.Dropout(0), nn.Linear(2 * n_embd, num_experts))
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, mean=0.0, std=0.02)
                nn.init.zeros_(m.bias)


class RouterCond(_Holder):
    def __init__(self, n_embd: int, num_experts: int, top_k: int, use_argmax: bool, normalize: bool):
        super().__init__()
        self.num_experts, self.top_k, self.use_argmax, self.normalize = num_experts, top_k, use_argmax, normalize
        self.temperature = 1.0
        self.router = CondRouterMLP(n_embd, num_experts)
        self.logits = None


class NoiseBlockMoE(_Holder):
    """One MoE-DiT block (modedit.py:424-528).  ``isinstance(block, NoiseBlockMoE)`` is what the agent's expert-usage
    logging checks (mode_agent.py:470-476)."""

    def __init__(self, n_embd, n_heads, attn_pdrop, mlp_pdrop, num_experts=4, top_k=2, router_normalize=True, use_argmax=False):
        super().__init__()
        self.n_embd = n_embd
        self.ln_1 = RMSNorm(n_embd, eps=1e-6)
        self.attn = Attention(n_embd, n_heads, attn_pdrop)
        self.ln_2 = RMSNorm(n_embd, eps=1e-6)
        self.router = RouterCond(n_embd, num_experts, top_k, use_argmax, router_normalize)
        self.experts = nn.ModuleDict({f"expert_{i}": Mlp(n_embd, bias=False, dropout=mlp_pdrop) for i in range(num_experts)})
        self.num_experts = num_experts
        self.logits = None
        self.probs = None
        self.expert_usage = torch.zeros(num_experts)
        self.inference_expert_usage = torch.zeros(num_experts)
        self.total_tokens_processed = 0
        self.fused_experts = {}     # {sigma bits: (e0, e1, p0, p1)} — routing cache; weights are never duplicated
        self.routing_info = {}

    def get_expert_usage(self):
        return self.inference_expert_usage

    def reset_expert_usage(self):
        self.expert_usage.zero_()
        self.inference_expert_usage.zero_()
        self.total_tokens_processed = 0

    def reset_expert_cache(self):
        self.fused_experts = {}
        self.routing_info = {}


class MoDeDiT(nn.Module):
    """Mixture-of-Experts Diffusion Transformer denoiser on MI355X (reference: modedit.py:641-1090)."""

    def __init__(self, obs_dim: int, goal_dim: int, device: str, goal_conditioned: bool, action_dim: int, embed_dim: int,
                 embed_pdrob: float, attn_pdrop: float, n_layers: int, n_heads: int, goal_seq_len: int, obs_seq_len: int,
                 action_seq_len: int, state_dim=None, mlp_pdrop: float = 0.1, goal_drop: float = 0.1, linear_output: bool = True,
                 use_proprio: bool = False, cond_router: bool = True, num_experts: int = 4, top_k: int = 2,
                 router_normalize: bool = True, use_goal_in_routing: bool = False, use_argmax: bool = False, causal: bool = True,
                 use_shared_expert: bool = False, use_noise_token_as_input: bool = True, use_custom_attn_mask: bool = False,
                 init_style: str = "default", compute_dtype: str = "bf16", n_img_tokens: int = 2):
        super().__init__()
        # flag combinations the reference itself cannot run or that leave the benchmarked path
        unsupported = dict(use_proprio=use_proprio, use_custom_attn_mask=use_custom_attn_mask, use_shared_expert=use_shared_expert,
                           not_goal_conditioned=not goal_conditioned, not_linear_output=not linear_output,
                           not_causal=not causal)
        bad = [k for k, v in unsupported.items() if v]
        if bad:
            raise NotImplementedError(f"MoDeDiT (HIP): unsupported configuration flags: {bad}")
        if goal_seq_len != 1 or obs_seq_len != 1:
            raise NotImplementedError("MoDeDiT (HIP): goal_seq_len == obs_seq_len == 1 is the only layout the reference ships")
        if embed_pdrob:
            raise NotImplementedError("MoDeDiT (HIP): embed_pdrob must be 0 (as in conf/model/mode_agent.yaml:61)")
        self.device = device
        self.use_proprio = use_proprio
        self.obs_dim, self.goal_dim, self.action_dim, self.embed_dim = obs_dim, goal_dim, action_dim, embed_dim
        self.sigma_emb = nn.Linear(1, embed_dim)
        self.sigma_linear = nn.Linear(embed_dim, embed_dim, bias=False)
        seq_size = goal_seq_len + obs_seq_len - 1 + action_seq_len
        self.tok_emb = nn.Linear(obs_dim, embed_dim, bias=False)
        self.gripper_embed = nn.Linear(obs_dim, embed_dim, bias=False)        # dead in the reference too (never gets a grad)
        self.goal_emb = nn.Linear(goal_dim, embed_dim, bias=False)
        self.action_emb = nn.Linear(action_dim, embed_dim, bias=False)
        self.pos_emb = nn.Parameter(torch.zeros(1, seq_size, embed_dim))
        self.cond_mask_prob = goal_drop
        self.attn_pdrop, self.mlp_pdrop = attn_pdrop, mlp_pdrop
        self.num_layers, self.n_heads = n_layers, n_heads
        self.blocks = nn.ModuleList([
            NoiseBlockMoE(embed_dim, n_heads, attn_pdrop, mlp_pdrop, num_experts=num_experts, top_k=top_k,
                          router_normalize=router_normalize, use_argmax=use_argmax) for _ in range(n_layers)])
        self.ln = RMSNorm(embed_dim, eps=1e-6)
        self.linear_output = linear_output
        self.out = nn.Linear(embed_dim, action_dim)
        self.goal_seq_len, self.action_seq_len = goal_seq_len, action_seq_len
        self.num_experts, self.top_k = num_experts, top_k
        self.router_normalize, self.use_argmax = router_normalize, use_argmax
        self.use_shared_expert = use_shared_expert
        self.use_noise_token_as_input = use_noise_token_as_input
        self.use_goal_in_routing = use_goal_in_routing
        # cond_router=False (modedit.py:296-301, 322-325, 550-553): every block routes each TOKEN on its own ln_2-normalised state instead of the
        # conditioning row - same router parameters (Linear(D,2D), Linear(2D,E)), routing resolved inside the launch chain, per layer: inference
        # (forward / denoise / every sampler) and training (layer-by-layer forward with the host's multinomial draw in between, training.py).
        self.cond_router = bool(cond_router)
        self.init_style = init_style           # accepted and ignored, like the reference
        self.goal_conditioned, self.causal = goal_conditioned, causal
        self.n_img_tokens = n_img_tokens
        self.seq_len = (1 if use_noise_token_as_input else 0) + goal_seq_len + n_img_tokens + action_seq_len
        self.logits_per_layer = None
        self.probs_per_layer = None
        self.compute_dtype = compute_dtype
        self._engine: Optional[DitEngine] = None
        self._route_cache = {}
        # How the HIP backward hands over parameter gradients (training.py): "autograd" = through autograd like the reference module (accumulate
        # hooks fire: torch DistributedDataParallel as Lightning wraps it, hook-driven clipping, any torch optimizer); "arena" = written straight
        # into the flat gradient arena, p.grad aliases it, autograd sees None (FusedAdamW / ArenaGradReducer switch to it).
        self.grad_mode = "autograd"

    # ------------------------------------------------------------------ engine access
    @property
    def engine(self) -> DitEngine:
        if self._engine is None or self._engine.compute_dtype != self.compute_dtype:
            self._engine = DitEngine(self, self.compute_dtype)
        self._engine.ensure_weights()
        return self._engine

    # ------------------------------------------------------------------ reference-compatible helpers
    def get_params(self):
        return self.parameters()

    def preprocess_goals(self, goals, states_length, uncond=False):
        """modedit.py:862-880 (incl. the element-wise Bernoulli goal mask in training, :882-893)."""
        if goals.dim() == 2:
            goals = goals.unsqueeze(1)
        if goals.shape[1] == states_length and self.goal_seq_len == 1:
            goals = goals[:, :1, :]
        if goals.shape[-1] == 2 * self.obs_dim:
            goals = goals[:, :, : self.obs_dim]
        if self.training and self.cond_mask_prob > 0.0:
            mask = torch.bernoulli(torch.full_like(goals, self.cond_mask_prob))
            goals = goals * (1.0 - mask)
        if uncond:
            goals = torch.zeros_like(goals)
        # the reference's goal_emb (nn.Linear(goal_dim, D), modedit.py:690) raises a shape error on anything else; the HIP GEMM would read
        # goal_dim floats per row regardless - refuse here.  (goal_dim == 2 * obs_dim trips the slice above in the reference as well.)
        if goals.shape[-1] != self.goal_dim or goals.shape[1] != self.goal_seq_len:
            raise ValueError(f"goals must be (B, {self.goal_seq_len}, {self.goal_dim}) after preprocess_goals, got {tuple(goals.shape)}")
        return goals

    def _check_batch(self, B, img, goals, actions) -> None:
        """Shape contract of one call: the chain reads B x (n_img x obs_dim | goal_dim | A_len x A_dim) floats from raw pointers - a tensor of
        any other shape must be refused here (the reference fails in its nn.Linear / torch.cat shape checks instead)."""
        if img.shape[0] != B or goals.shape[0] != B:
            raise ValueError(f"batch mismatch: actions have {B} samples, state_images {img.shape[0]}, goals {goals.shape[0]}")
        if actions.dim() != 3 or actions.shape[1] != self.action_seq_len or actions.shape[2] != self.action_dim:
            raise ValueError(f"actions must be (B, {self.action_seq_len}, {self.action_dim}), got {tuple(actions.shape)}")

    def forward(self, states, actions, goals, sigma, uncond: Optional[bool] = False):
        """states: {'state_images': (B, 2, obs_dim)}; actions (B, A_len, A_dim); goals (B,1,G)|(B,G); sigma (B,)|() -> (B, A_len, A_dim)."""
        if self.training:
            from .training import dit_forward_train        # HIP forward with activation stash + HIP backward behind autograd
            return dit_forward_train(self, states, actions, goals, sigma, uncond)
        eng = self.engine
        dev, B = eng.device, actions.shape[0]
        if B == 0:                                                       # empty batch: empty prediction, no launches
            return torch.empty(0, self.action_seq_len, self.action_dim, dtype=torch.float32, device=dev)
        img, goals, acts = self._inputs(eng, states, actions, goals, uncond)
        emb_t = eng.sigma_embed(self._sigma_rows(eng, sigma, B))
        img_e, goal_e = eng.embed_obs(img, goals)
        F = torch.empty(B, self.action_seq_len, self.action_dim, dtype=torch.float32, device=dev)
        self._routed_forward(eng, B, emb_t, goal_e, img_e, acts, F=F)
        self.logits_per_layer = [None] * self.num_layers                   # only populated in training (modedit.py:584-593)
        self.probs_per_layer = [None] * self.num_layers
        return F

    def _routed_forward(self, eng, B, emb_t, goal_e, img_e, x, account: bool = True, guidance=None, **head) -> None:
        """One denoiser forward with its routing.  The conditioning rows are emb_t ([1, D] for the whole batch or [B, D]), or with goal routing
        emb_t + goal_e, one row per sample (modedit.py:801-802).  Token routing: every block routes its tokens inside the chain, no dispatch
        records; otherwise router + dispatch of the conditioning rows.  ``head``: the output head's arguments of ``DitEngine.forward``.
        ``guidance`` (the device scalar of ``_guidance``): B pairs run as 2B samples, the unconditional halves behind the conditional ones - per-sample
        conditioning rows are [emb_t + goal_e ; emb_t] (goal routing) or emb_t twice; routing, dispatch and the usage counters cover all 2B·T tokens."""
        D, T = self.embed_dim, self.seq_len
        Bi = self._internal_batch(B, guidance is not None)
        cond = (emb_t.expand(B, D) + goal_e).contiguous() if self.use_goal_in_routing else emb_t
        if guidance is not None and (self.use_goal_in_routing or cond.shape[0] != 1):   # per-sample rows: the unconditional half has its own
            cond = torch.cat([cond, emb_t.expand(B, D)])
        R, N = cond.shape[0], Bi * T
        es, cs = 0 if emb_t.shape[0] == 1 else D, 0 if R == 1 else D
        if self.cond_router:
            idx, w, _, _ = eng.route(cond)
            rec = self._last_meta = eng.dispatch(idx, w, self.num_layers, R, N if R == 1 else T, N)
            ml = eng.meta_layout(N)
            eng.forward(B, emb_t, es, cond, cs, rec.data_ptr(), ml.total_words, goal_e, img_e, x, uniform=R == 1, guidance=guidance, **head)
        else:
            ml, rec = None, torch.empty(self.num_layers, N, self.top_k, dtype=torch.int32, device=eng.device)
            idx = rec                                                    # token routing: the call's record IS its decisions
            eng.forward(B, emb_t, es, cond, cs, None, 0, goal_e, img_e, x, topk_out=idx, guidance=guidance, **head)
        self._last_topk = idx
        if account:
            self._account_calls(eng, [rec], Bi, ml)

    # ------------------------------------------------------------------ classifier-free guidance
    def _guidance(self, w):
        """The guidance scale of a guided call as the chain reads it: ONE device fp32 scalar owned by the model, whose address every captured guided
        graph bakes in - a new value is a 4-byte copy made here, outside any capture, never a recapture.  ``w``: None (unguided: None comes back), a
        number, or that scalar itself (a call made from inside a chain that is being captured).  D_w = D_u + w (D_c - D_u) with D_u the prediction for
        a zero goal: the chain then runs both branches of every sample, 2B rows (``DitEngine.forward``).  Shapes that only the fallback row kernels
        take are refused here, before the first launch, and so is training mode (goal dropout is the training-time half of the method).
        The scalar is per MODEL: calls are meant to follow one another on one stream.  Two denoisers with different scales that share this model
        from different streams or threads would race on it - give each its own model then."""
        if w is None or torch.is_tensor(w):
            return w
        if self.training:
            raise ValueError("classifier-free guidance is an inference-time combine: call .eval() first (guidance_scale is set)")
        if self.embed_dim > 4096 or self.top_k > 2:
            raise ValueError(f"classifier-free guidance runs in the row kernels only: embed_dim <= 4096 and top_k <= 2 (got embed_dim={self.embed_dim}, "
                             f"top_k={self.top_k})")
        dev = self.engine.device
        t = getattr(self, "_guid_dev", None)
        if t is None or t.device != dev:
            t, self._guid_val = torch.empty(1, dtype=torch.float32, device=dev), None
            self._guid_dev = t
        if self._guid_val != float(w):
            t.copy_(torch.tensor([float(w)], dtype=torch.float32))
            self._guid_val = float(w)
        return t

    # ------------------------------------------------------------------ fused EDM forward / DDIM sampler
    def _inputs(self, eng, states, action, goals, uncond=False):
        """The input contract of every path: (state_images [B, n_img, obs_dim], goals [B, G], x [B, A_len, A_dim]) as ``_f32`` tensors, any other shape
        refused (``_check_batch``).  ``states=None``: the caller holds these observations' embeddings already - only x is converted."""
        x = _f32(action, eng.device)
        if states is None:
            return None, None, x
        img = _f32(states["state_images"], eng.device)
        if img.dim() != 3 or img.shape[1] != self.n_img_tokens or img.shape[2] != self.obs_dim:
            raise ValueError(f"state_images must be (B, {self.n_img_tokens}, {self.obs_dim}), got {tuple(img.shape)}")
        goals = _f32(self.preprocess_goals(goals, 1, uncond=bool(uncond)), eng.device)
        goals = goals.reshape(goals.shape[0], -1)                        # (B, 1, G) after preprocess_goals: a view, still contiguous
        self._check_batch(x.shape[0], img, goals, x)
        return img, goals, x

    @staticmethod
    def _sigma_rows(eng, sigma, B: int):
        """The noise levels of one call as a flat fp32 device vector: one for the whole batch, or one per sample."""
        sig = _f32(sigma, eng.device).reshape(-1)
        if sig.numel() not in (1, B):
            raise ValueError("sigma must be a scalar or have one entry per sample")
        return sig

    @staticmethod
    def _internal_batch(B: int, guided: bool) -> int:
        """Rows the chain runs for B samples: under classifier-free guidance every sample is a (conditional, unconditional) pair."""
        return 2 * B if guided else B

    def _graph_key(self, eng, B: int, sigma_data: float, guided: bool):
        """What every captured chain depends on besides its own schedule / sampler (arena pointers are static: weight updates keep graphs valid)."""
        return (B, eng.compute_dtype, eng._structs_for, str(eng.device), float(sigma_data), self._routing_mode(), guided)

    def _capture_entry(self, eng, cache: dict, key, capacity: int, img, goals, x, guided: bool, body, before=None, **extra) -> tuple:
        """A new entry of a store of captured denoiser chains (``denoise_graphed``'s, ``ChunkedRolloutPolicy``'s): its own copies of the inputs, the
        observation-embedding buffers, the workspace the graph owns and ``extra``; ``body(ent)`` is warmed up and captured into ``ent["graph"]`` on that
        workspace, after ``before(ent)``.  Returns (entry, what the CAPTURED call of ``body`` returned: the tensors a replay writes).  A store at
        ``capacity`` drops its oldest entry first (no hoarding)."""
        if len(cache) >= capacity:
            cache.pop(next(iter(cache)))
        B, dev = x.shape[0], eng.device
        ent = dict(img=img.clone(), goals=goals.clone(), x=x.clone(), img_e=torch.empty(B * self.n_img_tokens, self.embed_dim, device=dev),
                   goal_e=torch.empty(B, self.embed_dim, device=dev), ws=self._chunk_ws(eng, self._internal_batch(B, guided), 1), **extra)
        with eng.pinned_workspace(ent["ws"]):
            if before is not None:
                before(ent)
            ent["graph"], out = warm_and_capture(lambda: body(ent), dev)
        cache[key] = ent
        return ent, out

    @torch.no_grad()
    def denoise(self, states, action, goals, sigma, sigma_data: float, _account: bool = True, _obs_emb=None, guidance=None):
        """GCDenoiser.forward (score_wrappers.py:65-80) with c_in / c_out / c_skip fused into the HIP chain.  ``_obs_emb``: (img_e, goal_e) already
        computed for these observations (denoise_graphed keeps them across the calls of one sampler run).  ``guidance``: classifier-free guidance
        scale w (``_guidance``) - the result is D_u + w (D_c - D_u), formed in the head kernel."""
        guidance = self._guidance(guidance)
        eng = self.engine
        dev, B = eng.device, action.shape[0]
        if B == 0:
            return _f32(action, dev).clone()
        img, goals, x = self._inputs(eng, states if _obs_emb is None else None, action, goals)
        sig = self._sigma_rows(eng, sigma, B)
        c_in, scal = _edm_rows(sig, sigma_data)
        R, emb_t = sig.numel(), eng.sigma_embed(sig)
        img_e, goal_e = _obs_emb if _obs_emb is not None else eng.embed_obs(img, goals)
        den = torch.empty_like(x)
        self._routed_forward(eng, B, emb_t, goal_e, img_e, x, account=_account, guidance=guidance, c_in=c_in, c_in_stride=0 if R == 1 else 1,
                             scal_ptr=scal.data_ptr(), scal_stride=0 if R == 1 else 4, denoised=den)
        return den

    @torch.no_grad()
    def denoise_graphed(self, states, action, goals, sigma, sigma_data: float, guidance=None):
        """``denoise`` for a batch that shares ONE noise level (a 0-dim / 1-element sigma, device or host), replayed as a hipGraph: sigma embedding,
        fp32 router + dispatch of all layers, EDM scalings, observation embeddings and the denoiser forward are captured once per batch size with
        sigma as a DEVICE scalar, so the same graph serves every noise level of every sampler (euler, heun, dpm-solver++ ...: gc_sampling.py:165-994)
        - no per-step host work beyond three small input copies.  Goal routing: the graph also forms cond = emb + goal_emb(goal) and routes
        and dispatches those B rows; token routing: the forward routes every token itself.  Returns None with MODE_HIP_GRAPH=0.
        ``guidance``: as for ``denoise``; guided and unguided graphs are separate cache entries, the scale's value is in no key."""
        guidance = self._guidance(guidance)
        eng = self.engine
        dev, B = eng.device, action.shape[0]
        if B == 0 or not graphs_enabled():
            return None
        sig = torch.as_tensor(sigma, dtype=torch.float32).detach().reshape(-1)[:1]
        guided = guidance is not None
        key = self._graph_key(eng, B, sigma_data, guided)
        cache = self._route_cache.setdefault("denoise_graphs", {})
        ent = cache.get(key)
        # The observations are the same tensors for every denoiser call of a sampler run (gc_sampling.py's loops pass `state` / `goal` through
        # unchanged): their embeddings - two fp32 GEMMs, 6 % of a call at B = 128 - are computed once per (tensor objects, in-place version, weights)
        # and kept beside the graph.  The cache holds references to the tensors it was computed from, so an address cannot be recycled under it.
        src = (states["state_images"], goals)
        okey = (src[0]._version, src[1]._version, eng._wkey)
        fresh = ent is None or ent.get("obs_ref") is None or ent["obs_ref"][0] is not src[0] or ent["obs_ref"][1] is not src[1] or ent["obs_key"] != okey
        img, gl, x = self._inputs(eng, states if fresh else None, action, goals)
        if not fresh and x.shape != ent["x"].shape:
            raise ValueError(f"action must be {tuple(ent['x'].shape)}, got {tuple(x.shape)}")
        # embedded OUTSIDE the graph, and ahead of its warm-up: routing on uninitialised memory can yield out-of-range expert ids
        embed = lambda e: eng.embed_obs(e["img"], e["goals"], out=(e["img_e"], e["goal_e"]))
        if ent is None:
            def run(e):
                out = self.denoise(None, e["x"], None, e["sig"], sigma_data, _account=False, _obs_emb=(e["img_e"], e["goal_e"]), guidance=guidance)
                return out, self._last_topk, self._last_meta if self.cond_router else None
            ent, res = self._capture_entry(eng, cache, key, 8, img, gl, x, guided, run, before=embed, sig=sig.to(dev, copy=True))
            ent["out"], ent["topk"], ent["meta"] = res
        if fresh:
            ent["img"].copy_(img); ent["goals"].copy_(gl)
            embed(ent)
            # (a Bernoulli goal mask - training mode with goal_drop > 0 - must be redrawn per call: no reuse then)
            keep = not (self.training and getattr(self, "goal_drop", 0.0) > 0)
            ent["obs_ref"], ent["obs_key"] = (src if keep else None), okey
        ent["x"].copy_(x); ent["sig"].copy_(sig, non_blocking=True)
        ent["graph"].replay()
        if self._routes_per_chunk():
            self._last_topk = ent["topk"]
        self._account_calls(eng, [ent["meta"] if self.cond_router else ent["topk"]], self._internal_batch(B, guided))
        return ent["out"].clone()

    def _schedule_state(self, eng, sig, B, sigma_data: float, out=None, solver: str = "ddim", lin=None):
        """Everything of a DDIM run that depends on the noise SCHEDULE only (not on the observations): per-step EDM scalings, the sigma
        embeddings, and the routing of all steps and layers with its dispatch records.  The reference resolves the same thing once per noise level
        and caches it (precompute_experts_for_inference / the cache read at modedit.py:542-546); here it is a set of device tensors the captured
        launch chain reads.  Routing decisions cached by ``precompute_experts_for_inference`` for these exact sigma values (and these weights) are
        CONSUMED here - no router launch at all; otherwise the fp32 router runs on the device.  With ``out`` the results are written in place
        (the graph has the pointers baked in).  ``B`` is the chain's internal batch (twice the samples under guidance): the dispatch records are for B·T tokens."""
        T, Ly = self.seq_len, self.num_layers
        # two-stage solvers (sample_two_stage_fused): `sig` lists the sigma of EVERY denoiser evaluation, `lin` [n, 4] the linear update of each
        s, nxt = (sig.contiguous(), torch.zeros_like(sig)) if lin is not None else (sig[:-1].contiguous(), sig[1:])
        n = s.numel()
        ms = self._dpmpp_2m_weights(sig) if (solver == "dpmpp_2m" and lin is None) else None
        c_in, scal = _edm_rows(s, sigma_data, nxt, ms)
        st = dict(c_in=c_in, scal=scal, emb_all=eng.sigma_embed(s))      # emb_all [n, D]: one conditioning row per step
        if lin is not None:
            st["lin"] = lin.to(device=eng.device, dtype=torch.float32).contiguous()
        # goal / token routing depends on the observations: it is resolved inside the captured chunk (_chunk_routing), not here - and a
        # routing cache filled by precompute_experts_for_inference for ONE goal never stands in for the others
        if not self._routes_per_chunk():
            cached = None
            if all(blk.fused_experts for blk in self.blocks) and getattr(self, "_fused_for", None) == eng._wkey:
                keys = [float(v) for v in s.tolist()]                    # (host sync: only when the schedule state is (re)built)
                if all(k_ in blk.fused_experts for blk in self.blocks for k_ in keys):
                    cached = keys
            if cached is not None:
                idx = torch.tensor([[blk.fused_experts[k_][0] for k_ in cached] for blk in self.blocks], dtype=torch.int32, device=eng.device)
                w = torch.tensor([[blk.fused_experts[k_][1] for k_ in cached] for blk in self.blocks], dtype=torch.float32, device=eng.device)
            else:
                idx, w, _, _ = eng.route(st["emb_all"])                  # [L, n, k]: routing for ALL steps up front
            N = B * T
            st.update(idx=idx.contiguous(), w=w.contiguous(), meta=eng.dispatch(idx.contiguous(), w.contiguous(), Ly * n, 1, N, N), from_cache=cached is not None)
        if out is None:
            return st
        for k_, v in st.items():                                         # device tensors in place (the graph reads them); from_cache is a host value
            if k_ == "from_cache":
                out[k_] = v
            else:
                out[k_].copy_(v)
        return out

    @staticmethod
    def _dpmpp_2m_weights(sig):
        """DPM-Solver++(2M), gc_sampling.py:700-734: from the second step on (and not into sigma = 0) the update takes (1 + 1/(2r)) D - (1/(2r)) D_old for D,
        r = h_last / h in t = -ln sigma.  Returns [n] fp32: 1/(2r) per step in the reference's operation order, 0 where the plain step applies
        (the head kernel's scal[:, 3], ModeHeadDesc.den_prev)."""
        s, nxt = sig[:-1], sig[1:]
        ms = torch.zeros_like(s)
        if s.numel() > 1:
            h = s.log() - nxt.log()
            r = h[:-1] / h[1:]
            ms[1:] = torch.where(nxt[1:] > 0, 1.0 / (2.0 * r), torch.zeros_like(r))
        return ms

    def _routing_mode(self):
        """Part of every captured chunk's key: the chain a graph holds depends on how the model routes."""
        return bool(self.use_goal_in_routing), bool(self.cond_router)

    def _routes_per_chunk(self) -> bool:
        """Goal routing (router input emb_t + goal_emb(goal): one row per sample) or token routing (cond_router=False: one decision per token
        inside the chain): the routing of a sampler run depends on the observations, so the captured chunk resolves it itself."""
        return self.use_goal_in_routing or not self.cond_router

    def _chunk_routing(self, eng, sched, goal_e, n: int, B: int, ml, tok=None, guided: bool = False):
        """Routing state of a captured chunk of n denoiser evaluations, issued right after the observation embeddings; returns (args of
        evaluation j -> dict, route output or None, dispatch records or None).  Goal routing: the conditioning rows of every level,
        cond[j·B + b] = emb_all[j] + goal_e[b] ([n·B, D]), one router launch over all of them and one dispatch launch; the router output
        [L, n·B, k] is, contiguously, [(L·n), B, k], so level j's records sit at meta + j·words with layer stride n·words - the layout of the
        schedule-only routing.  Token routing (``tok``: int32 [n, L, B·T, k]): every forward routes its tokens itself and writes its
        decisions to tok[j].  The default (conditioning-row routing on sigma only) reads the schedule state's records, as before.
        ``B`` is the chain's internal batch: with ``guided`` goal_e has B/2 rows and a level's B conditioning rows are emb_all[j] + goal_e for
        the conditional half, emb_all[j] alone for the unconditional half."""
        D, T = self.embed_dim, self.seq_len
        emb_all = sched["emb_all"]
        cond = idx = None
        meta = sched.get("meta")
        if self.use_goal_in_routing:
            if guided:
                cond = emb_all[:, None, :].repeat(1, B, 1)
                cond[:, :B // 2] += goal_e[None, :, :]
                cond = cond.reshape(n * B, D)
            else:
                cond = (emb_all[:, None, :] + goal_e[None, :, :]).reshape(n * B, D)
            if self.cond_router:
                idx, w, _, _ = eng.route(cond)
                meta = eng.dispatch(idx, w, self.num_layers * n, B, T, B * T)

        def at(j):
            c, cs = (emb_all[j], 0) if cond is None else (cond[j * B:(j + 1) * B], D)
            if tok is not None:
                return dict(cond=c, cond_stride=cs, meta_ptr=None, meta_stride=0, uniform=False, topk_out=tok[j])
            return dict(cond=c, cond_stride=cs, meta_ptr=meta.data_ptr() + 4 * j * ml.total_words, meta_stride=n * ml.total_words,
                        uniform=cond is None, topk_out=None)
        return at, idx, meta

    def _chunk_steps(self, eng, img, goals, bufs, sched, evals, tok=None, guidance=None):
        """The observation-dependent launch chain of a fused sampler run: embeddings of the observations (+ the routing of goal-routed models)
        + one denoiser forward per entry of ``evals`` (``_Eval`` records over the buffers ``bufs``); pure launches, no host sync -> capturable.
        Reads the schedule state by pointer.  Returns the meta layout and the chunk's routing output {idx, meta} (``_chunk_routing``).  ``guidance``
        (device scalar): every forward is the guided one - the buffers and the observation embeddings keep B rows, routing and the forwards' interior have 2B."""
        B, T = bufs[0].shape[0], self.seq_len
        Bi = self._internal_batch(B, guidance is not None)
        img_e, goal_e = eng.embed_obs(img, goals)                        # step-invariant, hoisted (modedit.py:760,765)
        ml = eng.meta_layout(Bi * T)
        emb_all, c_in, scal = sched["emb_all"], sched["c_in"], sched["scal"]
        at, idx, meta = self._chunk_routing(eng, sched, goal_e, len(evals), Bi, ml, tok, guided=guidance is not None)
        buf = lambda i: None if i is None else bufs[i]
        for j, ev in enumerate(evals):
            r = at(j)
            eng.forward(B, emb_all[j], 0, r["cond"], r["cond_stride"], r["meta_ptr"], r["meta_stride"], goal_e, img_e, bufs[ev.x_in],
                        c_in=c_in.data_ptr() + 4 * j, c_in_stride=0, scal_ptr=scal.data_ptr() + 16 * j, scal_stride=0, x_next=bufs[ev.x_out],
                        uniform=r["uniform"], denoised=buf(ev.den_out), den_prev=buf(ev.den_prev),
                        lin_ptr=sched["lin"].data_ptr() + 16 * j if ev.lin else None, aux1=buf(ev.aux1), aux2=buf(ev.aux2), topk_out=r["topk_out"],
                        guidance=guidance)
        return ml, dict(idx=idx, meta=meta)

    @staticmethod
    def _ddim_evals(n: int, multistep: bool):
        """``_chunk_steps`` entries of an n-step DDIM run: the state (buffer 0) is updated in place.  ``multistep`` (DPM-Solver++(2M)): the head
        also writes each step's denoised prediction to buffer 1 / 2 alternately and reads the previous step's from the other one."""
        den = lambda s: 1 + (s & 1) if multistep and s >= 0 else None
        return [_Eval(x_in=0, x_out=0, den_out=den(s), den_prev=den(s - 1)) for s in range(n)]

    # ---- two-stage solvers on the fused chain (Heun, DPM-Solver-2, DPM-Solver++(2S)) -------------------------------------------------------
    @staticmethod
    def _two_stage_plan(solver: str, sv):
        """Host plan of a deterministic two-stage solver over the levels ``sv`` (python floats): one entry per DENOISER EVALUATION -
        (sigma, x_in, x_out, (l0, l1, l2, l3), aux1, aux2, den_out) with buffer ids 0 = state, 1 = probe, 2 = first-stage prediction (None = unused);
        the head computes x_out = l0 x_in + l1 D(x_in; sigma) + l2 aux1 + l3 aux2 (ModeHeadDesc.lin).  The recurrences are the reference's
        (gc_sampling.py:257-312 sample_heun, :315-373 sample_dpm_2, :956-994 sample_dpmpp_2s; churn 0), multiplied out:
          Euler into sigma' (all three, and the only stage of a step into sigma' = 0):  x + (x - D)/s (s' - s) = (s'/s) x + (1 - s'/s) D
          Heun corrector:   x + ((x - D)/s + (p - D_p)/s') dt/2,  p = Euler probe at s'
          DPM-Solver-2:     x + (m - D_m)/s_m (s' - s),  m = Euler probe at s_m = sqrt(s s') (log-midpoint)
          DPM-Solver++(2S): m = (s_m/s) x - expm1(-h/2) D;  x' = (s'/s) x - expm1(-h) D_m,  h = ln s - ln s'"""
        import math
        plan = []
        for i in range(len(sv) - 1):
            s_, t_ = sv[i], sv[i + 1]
            if t_ == 0.0:
                plan.append((s_, 0, 0, (0.0, 1.0, 0.0, 0.0), None, None, None))
                continue
            if solver == "heun":
                r, dt = t_ / s_, t_ - s_
                plan.append((s_, 0, 1, (r, 1.0 - r, 0.0, 0.0), None, None, 2))
                plan.append((t_, 1, 0, (dt / (2 * t_), -dt / (2 * t_), 1.0 + dt / (2 * s_), -dt / (2 * s_)), 0, 2, None))
                continue
            # the log-midpoint exactly as the step loops compute it (fp32 tensor ops): the denoiser is evaluated at the same sigma bits
            sm = float(torch.tensor(s_, dtype=torch.float32).log().lerp(torch.tensor(t_, dtype=torch.float32).log(), 0.5).exp()) if solver == "dpm_2" else \
                float((0.5 * (torch.tensor(s_, dtype=torch.float32).log() + torch.tensor(t_, dtype=torch.float32).log())).exp())
            if solver == "dpm_2":
                r1, dt = sm / s_, t_ - s_
                plan.append((s_, 0, 1, (r1, 1.0 - r1, 0.0, 0.0), None, None, None))
                plan.append((sm, 1, 0, (dt / sm, -dt / sm, 1.0, 0.0), 0, None, None))
            elif solver == "dpmpp_2s":
                h = math.log(s_) - math.log(t_)
                plan.append((s_, 0, 1, (sm / s_, -math.expm1(-0.5 * h), 0.0, 0.0), None, None, None))
                plan.append((sm, 1, 0, (0.0, -math.expm1(-h), t_ / s_, 0.0), 0, None, None))
            else:
                raise ValueError(solver)
        return plan

    @torch.no_grad()
    def sample_two_stage_fused(self, states, action, goals, sigmas, sigma_data: float, solver: str, guidance=None):
        """sample_heun / sample_dpm_2 / sample_dpmpp_2s (deterministic: no churn, no clipping, no callback) as ONE hipGraph replay of the fused chain:
        every stage of these solvers is linear in (stage input, its prediction, the step's state, the first stage's prediction), which the head kernel
        applies (ModeHeadDesc.lin).  The schedule-dependent part - which sigma every evaluation sees, the coefficients, embeddings, routing - is a
        plan rebuilt only when the schedule values, the weights or the batch size change.  None when the fast path does not apply."""
        assert solver in ("heun", "dpm_2", "dpmpp_2s"), solver
        guidance = self._guidance(guidance)
        eng = self.engine
        if action.shape[0] == 0 or not graphs_enabled() or sigmas.numel() < 2:
            return None
        return self._sample_chunk(eng, *self._chunk_plan(eng, solver, sigmas.numel() - 1, guidance is not None), states, action, goals, sigmas, sigma_data,
                                  guidance=guidance)

    def _chunk_plan(self, eng, solver: str, n: int, guided: bool = False):
        """(graph key, plan) of a fused sampler over an n-step schedule for ``_sample_chunk``: "ddim" / "dpmpp_2m" (the one-evaluation-per-step
        chain) or "heun" / "dpm_2" / "dpmpp_2s" (two-stage solvers).  ``guided``: the classifier-free-guidance chain, kept under a key of its own, so
        that a model used both ways keeps both graphs."""
        cfg = ":cfg" if guided else ""
        if solver in ("ddim", "dpmpp_2m"):
            multi = solver != "ddim"
            return ("graph:" + solver if multi else "graph") + cfg, (lambda sig: (self._ddim_evals(n, multi), sig, dict(solver=solver)))

        def plan(sig):
            p = self._two_stage_plan(solver, [float(v) for v in sig.tolist()])          # (host sync: only when the schedule changed)
            evals = [_Eval(x_in=xin, x_out=xout, den_out=dout, aux1=a1, aux2=a2, lin=True) for _, xin, xout, _, a1, a2, dout in p]
            ev = torch.tensor([e[0] for e in p], dtype=torch.float32, device=eng.device)
            return evals, ev, dict(lin=torch.tensor([e[3] for e in p], dtype=torch.float32))
        return "graph:" + solver + cfg, plan

    @torch.no_grad()
    def sample_ddim_fused(self, states, action, goals, sigmas, sigma_data: float, solver: str = "ddim", guidance=None):
        """sample_ddim (gc_sampling.py:922-951) o GCDenoiser o MoDeDiT as one hipGraph replay.  The graph holds only what depends on the
        observations (embeddings + the denoiser forwards); sigma embeddings, routing, dispatch and the EDM scalings of the schedule live in a
        schedule state that is rebuilt only when the sigma VALUES, the weights or the batch size change.
        ``solver="dpmpp_2m"``: sample_dpmpp_2m (gc_sampling.py:700-734) on the same chain - its step is DDIM's exponential-integrator step applied to a
        two-point extrapolation of the denoised prediction, which the head kernel forms from the previous step's prediction (ModeHeadDesc.den_prev)."""
        assert solver in ("ddim", "dpmpp_2m"), solver
        guidance = self._guidance(guidance)
        eng = self.engine
        dev, B = eng.device, action.shape[0]
        if B == 0:                                                       # empty batch: nothing to denoise
            return _f32(action, dev).clone()
        n, multi = sigmas.numel() - 1, solver != "ddim"
        if graphs_enabled():                                             # one captured chain per solver; its buffer pattern is fixed by n
            return self._sample_chunk(eng, *self._chunk_plan(eng, solver, n, guidance is not None), states, action, goals, sigmas, sigma_data,
                                      guidance=guidance)
        img, goals, x0 = self._inputs(eng, states, action, goals)
        sig = _f32(sigmas, dev)
        if self._routes_per_chunk():                                    # goal / token routing without graphs: the per-step generic path
            x = x0.clone()
            prev = None
            for i in range(n):
                den = self.denoise({"state_images": img}, x, goals, sig[i].reshape(1), sigma_data, guidance=guidance)
                r = sig[i + 1] / sig[i]
                dd = den
                if solver == "dpmpp_2m" and prev is not None and float(sig[i + 1]) > 0:
                    c = 1.0 / (2.0 * ((sig[i - 1].log() - sig[i].log()) / (sig[i].log() - sig[i + 1].log())))
                    dd = (1.0 + c) * den - c * prev
                x = r * x + (1.0 - r) * dd
                prev = den
            return x
        bufs = [x0.clone(memory_format=torch.contiguous_format)] + [torch.empty(x0.shape, dtype=torch.float32, device=dev) for _ in range(2)]
        sched = self._schedule_state(eng, sig, self._internal_batch(B, guidance is not None), sigma_data, solver=solver)
        self._account_chunk(dict(sched=sched), self._chunk_steps(eng, img, goals, bufs, sched, self._ddim_evals(n, multi), guidance=guidance)[0], n, B,
                            guided=guidance is not None)
        return bufs[0]

    def _sample_chunk(self, eng, gkey, plan, states, action, goals, sigmas, sigma_data: float, hooks=None, rows: Optional[int] = None, guidance=None):
        """The fused samplers' hipGraph path: the launch chain of ``_chunk_steps`` captured once per ``_route_cache[gkey]`` entry (one per solver)
        and replayed per call.  ``plan(sig) -> (evaluations, sigma of the schedule state, its keyword arguments)`` is asked for when the entry is
        made and when the schedule changes; a new schedule is then written into the schedule state in place (the graph has its pointers baked
        in), unless its evaluations take another pattern of buffers, which needs another chain.

        ``hooks`` (rollout.VectorEnvPolicy): the caller's own store and device-side stages instead of the input copies and the returned clone -
        entries live in ``hooks.store[(gkey, B)]``, one per batch size; ``hooks.prologue(ent)`` writes the entry's inputs (img, goals, bufs[0])
        before every replay (and once before the capture's warm-up, which must route valid data); ``hooks.epilogue(ent, capturing)`` is
        captured at the end of the chain and reads its result, bufs[0].  The inputs then only give the shapes; returns None.  ``rows``: the
        first ``rows`` samples are real, the rest padding - the expert-usage counters count the real ones only.  ``guidance``: the chain is the
        guided one (``gkey`` from ``_chunk_plan(..., guided=True)``); B stays the number of samples, the chain's interior has 2B."""
        guidance = self._guidance(guidance)
        guided = guidance is not None
        dev, B = eng.device, action.shape[0]
        Bi = self._internal_batch(B, guided)
        img, goals, x0 = self._inputs(eng, states, action, goals)
        sig = _f32(sigmas, dev)
        key = (sig.numel(),) + self._graph_key(eng, B, sigma_data, guided)
        # identity of the schedule: a host-side tag of its VALUES when the tensor came from a get_sigmas_* / get_noise_schedule generator (the
        # agent builds a fresh tensor per chunk, mode_agent.py:752) - else the caller's tensor OBJECT (kept alive below, so neither its id nor its
        # storage can be recycled while the key is live) -, the weights, and the routing cache generation.  No device read on either path.
        # A tag only vouches for the values the generator wrote: once the tensor has been edited in place (its version moved past the one recorded in
        # the tag) two tagged tensors with different edits would share (tag, version) - such a tensor is identified as an object, with the device
        # compare below as the fallback, like any untagged tensor.
        tag = getattr(sigmas, "_mode_sched", None)
        if tag is not None and sigmas._version != tag[3]:
            tag = None
        sid = ("tag", tag) if tag is not None else ("obj", id(sigmas), sigmas._version)
        sched_key = (sid, eng._wkey, getattr(self, "_fused_gen", 0))
        cache, ckey = (self._route_cache, gkey) if hooks is None else (hooks.store, (gkey, B))
        ent = cache.get(ckey)
        fresh, planned = ent is None or ent["key"] != key, None
        if not fresh and ent["sched_key"] != sched_key:
            # an UNTAGGED foreign tensor object that may carry the same values: one small device compare (host sync) - the rare path; tagged
            # schedules and a reused tensor object never get here with an unchanged schedule
            same_values = (tag is None and ent["sched_key"][1:] == sched_key[1:] and bool(torch.equal(sig, ent["sig"])))
            ent["sig_ref"] = sigmas if tag is None else None
            if not same_values:
                planned = plan(sig)
                if planned[0] != ent["evals"]:
                    fresh = True                                         # another zero pattern: another chain
                else:
                    ent["sig"].copy_(sig)
                    with eng.pinned_workspace(ent["ws"]):
                        self._schedule_state(eng, planned[1], Bi, sigma_data, out=ent["sched"], **planned[2])
            ent["sched_key"] = sched_key
        if fresh:
            evals, s_sig, s_kw = planned if planned is not None else plan(sig)
            n = len(evals)
            ent = dict(key=key, img=img.clone(), goals=goals.clone(), sig=sig.clone(), evals=evals, sched_key=sched_key,
                       sig_ref=sigmas if tag is None else None,
                       bufs=[x0.clone(memory_format=torch.contiguous_format)] + [torch.zeros(x0.shape, dtype=torch.float32, device=dev) for _ in range(2)])
            # the graph owns its workspace: the engine's shared scratch buffer is re-allocated whenever a larger chain (a training step, a
            # bigger batch) asks for more, and a replay would then read freed memory
            ent["ws"] = self._chunk_ws(eng, Bi, n)
            ent["tok"] = self._chunk_topk_buffer(eng, n, Bi)

            def chain():
                out = self._chunk_steps(eng, ent["img"], ent["goals"], ent["bufs"], ent["sched"], evals, tok=ent["tok"], guidance=guidance)
                if hooks is not None:
                    hooks.epilogue(ent, torch.cuda.is_current_stream_capturing())
                return out
            with eng.pinned_workspace(ent["ws"]):
                ent["sched"] = self._schedule_state(eng, s_sig, Bi, sigma_data, **s_kw)
                if hooks is not None:
                    hooks.prologue(ent)
                ent["graph"], (ent["ml"], ent["route"]) = warm_and_capture(chain, dev)
            cache[ckey] = ent
        if hooks is None:
            ent["img"].copy_(img); ent["goals"].copy_(goals); ent["bufs"][0].copy_(x0)
        else:
            hooks.prologue(ent)
        ent["graph"].replay()
        self._account_chunk(ent, ent["ml"], len(ent["evals"]), B, rows, guided)
        return ent["bufs"][0].clone() if hooks is None else None

    def _chunk_ws(self, eng, B: int, n: int) -> torch.Tensor:
        """The workspace a captured chunk of n evaluations owns: the forward's, or the schedule's sigma embedding / the router's over n rows
        (n·B conditioning rows with goal routing), whichever is larger.  ``B``: the chain's internal batch."""
        rows = n * B if self.use_goal_in_routing else n
        return torch.empty(max(eng.workspace_bytes(B, 0), eng.workspace_bytes(0, rows)), dtype=torch.uint8, device=eng.device)

    def _chunk_topk_buffer(self, eng, n: int, B: int):
        """Token routing: int32 [n, L, B·T, k] that the n forwards of a captured chunk write their decisions to (B: the chain's internal batch); None
        otherwise."""
        if self.cond_router:
            return None
        return torch.empty(n, self.num_layers, B * self.seq_len, self.top_k, dtype=torch.int32, device=eng.device)

    def _account_chunk(self, ent, ml, n: int, B: int, rows: Optional[int] = None, guided: bool = False) -> None:
        """After a run of a chunk of n evaluations: ``_last_topk`` (level j of every layer at [:, j]) and the expert-usage counters, with device
        ops only - token routing: ONE histogram of the chunk's decisions; otherwise the dispatch records' per-expert counts.  ``rows`` < B: only
        the first ``rows`` samples are counted - token / goal routing: a histogram of their decisions (a goal-routed decision stands for the
        sample's T tokens); noise-level routing sends every sample to the same experts, so the counts scale by rows / B exactly.  ``guided``: the
        chain ran 2B samples, the unconditional halves behind the conditional ones; both halves' tokens are tokens processed and are counted (the
        first ``rows`` samples OF EACH HALF when padded)."""
        T, halves = self.seq_len, 2 if guided else 1
        N, r = self._internal_batch(B, guided) * T, B if rows is None else rows
        real = lambda t, per: t if r == B else torch.cat([t[:, :, h * B * per: (h * B + r) * per] for h in range(halves)], 2)   # the real rows of [L, n, halves·B·per, k]
        if ent.get("tok") is not None:
            self._last_topk = ent["tok"].transpose(0, 1)                 # [L, n, N, k]
            self._account_token_usage(real(self._last_topk, T), halves * r * T * n)
        elif self.use_goal_in_routing:
            self._last_topk = ent["route"]["idx"].view(self.num_layers, n, halves * B, self.top_k)
            if r == B:
                self._account_usage(ent["route"]["meta"], ml, N, n)
            else:
                self._account_token_usage(real(self._last_topk, 1), halves * r * T * n, weight=T)
        else:
            self._last_topk = ent["sched"]["idx"]
            self._account_usage(ent["sched"]["meta"], ml, N, n, rows=None if r == B else (r, B))

    def _account_calls(self, eng, recs, Bi: int, ml=None) -> None:
        """The expert-usage counters after ``len(recs)`` denoiser calls at internal batch ``Bi``.  ``recs``: per call its dispatch records [L, words], or
        under token routing its decisions [L, Bi·T, k] - ONE histogram of them all.  ``ml``: the records' layout, when the caller has it at hand."""
        N, calls = Bi * self.seq_len, len(recs)
        rec = recs[0] if calls == 1 else torch.stack(recs, 1)            # [L, calls, ...]
        if not self.cond_router:
            self._account_token_usage(rec, N * calls)
        else:
            self._account_usage(rec, eng.meta_layout(N) if ml is None else ml, N, calls)

    def _add_usage(self, counts, n_tokens: int) -> None:
        """Expert-usage counters (modedit.py:568-572, 594): ``counts`` [L, E] added on the device - no host sync on the hot path - and
        ``n_tokens`` to every block's token count."""
        if getattr(self, "_usage_dev", None) is None or self._usage_dev.device != counts.device:
            self._usage_dev = torch.zeros(self.num_layers, self.num_experts, dtype=torch.int64, device=counts.device)
        self._usage_dev += counts
        for blk in self.blocks:
            blk.total_tokens_processed += n_tokens

    def _account_usage(self, meta, ml, n_tokens: int, n: int = 1, rows=None) -> None:
        """Usage counters from dispatch records: ``meta`` [L·n, words] or [L, n, words], n forwards of n_tokens tokens each per layer (layer-major).
        ``rows`` = (r, B): count r of the records' B samples (records of one routing row for the whole batch: every count is a multiple of B)."""
        counts = meta[..., ml.counts: ml.counts + self.num_experts]
        counts = counts if n == 1 else counts.reshape(self.num_layers, n, -1).sum(1)
        if rows is not None:
            counts, n_tokens = counts.long() * rows[0] // rows[1], n_tokens * rows[0] // rows[1]
        self._add_usage(counts, n_tokens * n)

    def _account_token_usage(self, idx, n_tokens: int, weight: int = 1) -> None:
        """Usage counters under token routing: idx int32 [L, ..., k] (every token's experts) -> per-layer histogram; ``weight``: tokens per decision."""
        Ly, E = self.num_layers, self.num_experts
        self._add_usage(torch.zeros(Ly, E, dtype=torch.int64, device=idx.device).scatter_add_(
            1, idx.reshape(Ly, -1).long(), torch.full((Ly, idx[0].numel()), weight, dtype=torch.int64, device=idx.device)), n_tokens)

    def sync_expert_usage(self):
        """Fold the device-side counters into the per-block host tensors the agent's heat-map reads (mode_agent.py:466-511)."""
        if getattr(self, "_usage_dev", None) is not None:
            host = self._usage_dev.cpu().to(torch.float32)
            for i, blk in enumerate(self.blocks):
                blk.inference_expert_usage += host[i]
            self._usage_dev.zero_()

    # ------------------------------------------------------------------ aux losses (training side channel)
    def load_balancing_loss(self):
        """modedit.py:898-928.  After a training forward this is an output of the HIP autograd node: ``entropy_gamma * load_balancing_loss()``
        added to the loss back-propagates into the routers (mode_agent.py:413-415)."""
        aux = getattr(self, "_aux_losses", None)
        if self.training and aux is not None:
            return aux[0]
        terms = [b.probs["load_balancing_term"] for b in self.blocks if b.probs is not None]
        return sum(terms) / len(terms) if terms else 0.0

    def compute_router_z_loss(self, eps=1e-6):
        """modedit.py:930-969 (on the max-shifted logits, as the reference does); graph-attached after a training forward like
        ``load_balancing_loss`` (eps is the reference's default 1e-6 there)."""
        aux = getattr(self, "_aux_losses", None)
        if self.training and aux is not None and eps == 1e-6:
            return aux[1]
        z = [torch.log(torch.exp(lg).sum(-1) + eps).pow(2).mean() for lg in self.logits_per_layer]
        return sum(z) / len(z)

    # ------------------------------------------------------------------ per-sigma routing cache (reference: fused expert cache)
    def precompute_experts_for_inference(self, sigma, goal=None):
        """Reference modedit.py:971-992 duplicates two experts' weights per (sigma, layer) (~12 GB at C2) and keys the cache on a
        Python float mean that only hits at B=1.  Here only the routing decision (e0,e1,p0,p1) is cached,
        keyed on the exact sigma bits; weights are never copied."""
        if self.training or not self.cond_router:                        # token routing depends on the observations: nothing to cache per noise level
            return
        eng = self.engine
        sig = sigma.detach().to(device=eng.device, dtype=torch.float32).reshape(-1)[:1].contiguous()
        emb = eng.sigma_embed(sig)
        cond = emb
        if self.use_goal_in_routing and goal is not None:
            _, goal_e = eng.embed_obs(torch.zeros(1, self.n_img_tokens, self.obs_dim, device=eng.device),
                                      goal.detach().to(eng.device, torch.float32).reshape(1, -1).contiguous())
            cond = emb + goal_e
        idx, w, _, _ = eng.route(cond.contiguous())
        key = float(sig.item())
        idx_h, w_h = idx.cpu(), w.cpu()
        if getattr(self, "_fused_for", None) != eng._wkey:               # entries made with other weights are stale: drop them
            self.reset_all_caches()
            self._fused_for = eng._wkey
        for i, blk in enumerate(self.blocks):
            blk.fused_experts[key] = (idx_h[i, 0].tolist(), w_h[i, 0].tolist())
            blk.routing_info[key] = {"indices": idx_h[i, 0].numpy(), "probs": w_h[i, 0].numpy()}
        self._fused_gen = getattr(self, "_fused_gen", 0) + 1             # the sampler's schedule state picks the new entries up

    def reset_all_caches(self):
        for blk in self.blocks:
            blk.reset_expert_cache()
        self._fused_gen = getattr(self, "_fused_gen", 0) + 1

    def freeze_router(self):
        for blk in self.blocks:
            blk.router.eval()
            for p in blk.router.parameters():
                p.requires_grad = False

    def unfreeze_router(self):
        for blk in self.blocks:
            blk.router.train()
            for p in blk.router.parameters():
                p.requires_grad = True

    def prepare_for_finetuning(self, freeze_routers: bool = True, freeze_expert_weights: float = 0.3, reset_expert_stats: bool = True):
        if freeze_routers:
            self.freeze_router()
