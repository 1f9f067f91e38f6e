"""Validation without a simulator, on the device: the reference's ``validation_step`` (mode_agent.py:442-464) - run the INFERENCE sampler on
held-out windows and measure the error between the sampled chunk and the demonstrated actions - as a loop that reads nothing back.

``data.WindowSweep`` hands out every held-out window exactly once (one launch per batch), ``Validator.predict`` plans a chunk for the batch on the
path ``ChunkedRolloutPolicy.denoise_actions`` takes (one hipGraph replay for the fused samplers), and ``mode_action_error`` (csrc/data_stream.hip;
formulas and summation order: include/mode_hip.h) adds the batch's masked squared and absolute errors into fp64 accumulators on the device.  The
caller's ``float(result["mse"])`` is the only host sync of a validation pass.

``LevelValidator`` is the other held-out signal: the denoising (score-matching) loss itself, per noise level.  ``mode_val_noise_levels`` gives every
swept window a level of a fixed sigma table and its noised input, one denoiser evaluation per batch predicts the clean chunk, and ``mode_level_error``
adds the masked squared error into fp64 accumulators per level - the same summation body as ``mode_action_error``, the same no-read-back loop.
"""
from __future__ import annotations

import math
from typing import Callable, Optional

import torch

from . import _lib
from .data import MAX_BATCH, MAX_WINDOW_FLOATS, WindowSweep
from .engine import _launch, _ptr
from .rollout import ChunkedRolloutPolicy


def _same(name: str, who: str, t, shape, dt, dev) -> None:
    if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous {dt} {shape} tensor on {dev}, got "
                         f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")


def _mean(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """``num / den`` where ``den > 0``, else 0: a mean over nothing is 0."""
    return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))


def _raw_unit(store, raw_units: bool) -> Optional[torch.Tensor]:
    """``unit[a] = 1 / (double) scale[a]``, 0 where ``scale[a] == 0``; None without ``raw_units`` or for a store without normalisation."""
    if not raw_units or store.scale is None:
        return None
    s = store.scale.to(torch.float64)
    return torch.where(s != 0, 1.0 / torch.where(s != 0, s, torch.ones_like(s)), torch.zeros_like(s)).contiguous()


def _check_validator_args(who: str, sweep, embed) -> None:
    if not isinstance(sweep, WindowSweep):
        raise ValueError(f"{who} needs a data.WindowSweep, got {type(sweep).__name__}")
    if not callable(embed):
        raise ValueError("embed must be a function batch -> {'state_images': [B, n_img_tokens, obs_dim]}")


def _check_draws(draws) -> None:
    if isinstance(draws, bool) or not isinstance(draws, int) or draws < 1:
        raise ValueError(f"draws must be an int >= 1, got {draws!r}")


def _held_out_pass(val, denoiser, draws, ema, add: Callable[[dict], None]) -> None:
    """The pass both validators run (``val``: the ``Validator`` or ``LevelValidator``): ``add(val.batch(i, draw))`` for every batch of every draw with
    ``denoiser`` in eval mode and, with ``ema``, the averaged weights swapped in; in a ``finally`` the live weights are swapped back and every
    submodule gets the ``training`` flag it had."""
    modes = [(m, m.training) for m in denoiser.modules()]
    if ema is not None:
        ema.swap()
    try:
        denoiser.eval()
        for draw in range(draws):
            for i in range(len(val)):
                add(val.batch(i, draw))
    finally:
        if ema is not None:
            ema.swap()
        for m, was in modes:
            m.training = was


def action_error(pred: torch.Tensor, target: torch.Tensor, sq: torch.Tensor, ab: torch.Tensor, cnt: torch.Tensor, mask: Optional[torch.Tensor] = None,
                 weight: Optional[torch.Tensor] = None, unit: Optional[torch.Tensor] = None, accumulate: bool = True) -> None:
    """``mode_action_error`` on the current stream: with ``c[b, w] = weight[b] * mask[b, w]`` (an absent factor is 1, a value that is not > 0 counts as
    0) and ``e = (pred - target) * unit[a]`` in fp64 from the fp32 difference,

        sq[w * A + a] (+)= sum_b c e^2,   ab[w * A + a] (+)= sum_b c |e|,   cnt[w] (+)= sum_b c

    ``pred``, ``target`` [B, W, A] fp32, ``mask`` [B, W] fp32, ``weight`` [B] fp32, ``unit`` [A] fp64, ``sq`` / ``ab`` [W * A] and ``cnt`` [W] fp64, all
    contiguous on one ROCm device.  Terms with ``c == 0`` are skipped, so ``pred`` may hold anything there.  No atomics: the result's bits depend on
    the shapes and the order of the calls only.  ``accumulate=False`` stores instead of adding."""
    if not torch.is_tensor(pred) or pred.dim() != 3 or pred.device.type != "cuda":
        raise ValueError(f"action_error: pred must be a [B, W, A] tensor on a ROCm device, got {tuple(getattr(pred, 'shape', ()))}")
    B, W, A = pred.shape
    if not 1 <= B <= MAX_BATCH or W < 1 or A < 1 or W * A > MAX_WINDOW_FLOATS:
        raise ValueError(f"action_error: needs 1 <= B <= {MAX_BATCH} and 1 <= W * A <= {MAX_WINDOW_FLOATS}, got {(B, W, A)}")
    for name, t, shape, dt in (("pred", pred, (B, W, A), torch.float32), ("target", target, (B, W, A), torch.float32), ("mask", mask, (B, W), torch.float32),
                               ("weight", weight, (B,), torch.float32), ("unit", unit, (A,), torch.float64), ("sq", sq, (W * A,), torch.float64),
                               ("ab", ab, (W * A,), torch.float64), ("cnt", cnt, (W,), torch.float64)):
        if t is None and name in ("mask", "weight", "unit"):
            continue
        _same(name, "action_error", t, shape, dt, pred.device)
    d = _lib.ModeActionErrorDesc(pred=_ptr(pred), target=_ptr(target), mask=_ptr(mask), weight=_ptr(weight), unit=_ptr(unit), sq=_ptr(sq), ab=_ptr(ab),
                                 cnt=_ptr(cnt), B=B, W=W, A=A, accumulate=1 if accumulate else 0)
    _launch(_lib.load().mode_action_error, d, pred.device)


class ValidationResult(dict):
    """What ``Validator.run`` returns: device tensors, nothing read back.

        mse, mae (scalars: the mean over every real step and action dimension), mse_per_step [W], mse_per_dim [A], count (the number of real,
        non-padded steps summed over the draws), and the accumulators sq / ab [W, A] and cnt [W] they derive from

    ``mse_executed(multistep)``: the mean over the first ``multistep`` steps of the chunk - the ones a rollout executes before it replans.  A mean over
    no step is 0.  Accumulators of several ranks (or passes) add: ``ValidationResult.from_sums(sq, ab, cnt)`` derives the means of the sums."""

    @classmethod
    def from_sums(cls, sq: torch.Tensor, ab: torch.Tensor, cnt: torch.Tensor) -> "ValidationResult":
        W = cnt.shape[0]
        sq, ab = sq.reshape(W, -1), ab.reshape(W, -1)
        A = sq.shape[1]
        count = cnt.sum()
        return cls(sq=sq, ab=ab, cnt=cnt, count=count, mse=_mean(sq.sum(), A * count), mae=_mean(ab.sum(), A * count),
                   mse_per_step=_mean(sq.sum(1), A * cnt), mse_per_dim=_mean(sq.sum(0), count.expand(A)))

    def mse_executed(self, multistep: int) -> torch.Tensor:
        W, A = self["sq"].shape
        if isinstance(multistep, bool) or not isinstance(multistep, int) or not 1 <= multistep <= W:
            raise ValueError(f"multistep must be an int in 1..{W}, got {multistep!r}")
        return _mean(self["sq"][:multistep].sum(), A * self["cnt"][:multistep].sum())


class Validator:
    """``run()`` sweeps ``sweep`` once per draw: for every batch the sampler plans a chunk from the batch's own noise, and the masked error between
    the plan and the demonstrated window is added into device accumulators.  One sweep launch (two with cameras), ``embed``, one sampler call and
    one error launch per batch; no host sync.

    ``embed(batch) -> {"state_images": [B, n_img_tokens, obs_dim]}`` is the caller's: the perceptual encoders on ``batch["rgb_obs"]``, or stored
    features looked up by ``batch["index"]``.

    ``batch(i, draw=0)``: batch ``i`` of the sweep with its noise scaled by ``sigma_max`` INSIDE the sweep's launch (one fp32 product per element,
    what ``ChunkedRolloutPolicy.denoise_actions`` does to its normal draw) - ``predict`` takes ``batch["noise"]`` as the sampler's initial latent as
    it is, so hand it batches made here.

    ``predict(batch) -> [B, W, A]``: the path of ``ChunkedRolloutPolicy.denoise_actions`` with ``x = batch["noise"]`` - routing precompute on first
    use, one hipGraph replay per batch for the fused and graphable samplers, the step-by-step loop otherwise.  ``B`` is fixed and the last batch is
    padded with ``valid = 0`` rows, so a sweep captures once.  Like ``denoise_actions`` it puts the denoiser in eval mode.

    ``run(draws=1, ema=None) -> ValidationResult``: eval mode for the pass and the previous mode afterwards; with ``ema=ArenaEMA`` the averaged
    weights are swapped in before and the live ones back in a ``finally`` (also when ``embed`` raises).  The error weighs row b's step w with
    ``valid[b] * action_mask[b, w]``: padded steps and padding rows count nothing.  ``raw_units=True`` with a normalised store reports the error in
    the store's raw action units, ``unit[a] = 1 / (double) scale[a]``, 0 where ``scale[a] == 0``: a constant dimension (it normalises to -1 whatever
    the action) contributes NO error.  ``raw_units=False`` or a store without normalisation: the error of the values the model sees.

    The goal is whatever the sweep puts into ``batch["latent_goal"]``: a ``WindowSweep(goal="hindsight", goal_horizon=...)`` on a store with
    ``step_goals`` validates the image-goal modality (a future step's stored embedding as the goal; ``"last"``: the episode's final step), the
    default sweep the episode's own goal.  Nothing here changes for it.

    The held-out score-matching loss per noise level is ``LevelValidator``'s, below.  Not here: encoding goal frames (the sweep gathers stored
    embeddings; ``batch["goal_index"]`` names the frame for an encoder of the caller's), disk formats, and gathering results across ranks - rank
    ``r`` of ``n`` may run the batches ``r, r + n, ...`` itself and sum the returned accumulators (``ValidationResult.from_sums``)."""

    def __init__(self, denoiser, sweep: WindowSweep, embed: Callable[[dict], dict], num_sampling_steps: int = 10, sigma_min: float = 0.001,
                 sigma_max: float = 80.0, noise_scheduler: str = "exponential", sampler_type: str = "ddim", raw_units: bool = True):
        _check_validator_args("Validator", sweep, embed)
        st = sweep.store
        self.sweep, self.embed, self.sigma_max = sweep, embed, float(sigma_max)
        self.policy = ChunkedRolloutPolicy(denoiser, num_sampling_steps=num_sampling_steps, sigma_min=sigma_min, sigma_max=sigma_max,
                                           noise_scheduler=noise_scheduler, sampler_type=sampler_type, act_window_size=sweep.window,
                                           multistep=sweep.window, action_dim=st.action_dim)
        self.unit = _raw_unit(st, raw_units)

    def __len__(self) -> int:
        return len(self.sweep)

    def batch(self, i: int, draw: int = 0) -> dict:
        return self.sweep.batch(i, draw, noise_scale=self.sigma_max)

    @torch.no_grad()
    def predict(self, batch: dict) -> torch.Tensor:
        return self.policy.denoise_actions(self.embed(batch), batch["latent_goal"], x=batch["noise"])

    @torch.no_grad()
    def run(self, draws: int = 1, ema=None) -> ValidationResult:
        _check_draws(draws)
        W, A, dev = self.sweep.window, self.sweep.store.action_dim, self.sweep.store.device
        sq, ab = (torch.zeros(W * A, dtype=torch.float64, device=dev) for _ in range(2))
        cnt = torch.zeros(W, dtype=torch.float64, device=dev)
        _held_out_pass(self, self.policy.model, draws, ema, lambda b: action_error(
            self.predict(b).to(torch.float32).contiguous(), b["actions"], sq, ab, cnt, mask=b["action_mask"], weight=b["valid"], unit=self.unit))
        return ValidationResult.from_sums(sq, ab, cnt)


# ------------------------------------------------------------------------------------------------ held-out denoising loss per noise level
MAX_LEVELS = 256           # the kernels' limit (include/mode_hip.h)


def noise_levels(actions: torch.Tensor, noise: torch.Tensor, window: torch.Tensor, sigmas: torch.Tensor, draw: int = 0):
    """``mode_val_noise_levels`` on the current stream -> ``(level [B] int32, sigma [B] fp32, noised [B, W, A] fp32)``:

        level[j] = (window[j] + draw) mod 2^32 mod K,   sigma[j] = sigmas[level[j]],   noised[j] = actions[j] + noise[j] * sigma[j]

    (one fp32 product and one fp32 sum per element, unfused).  ``actions``, ``noise`` [B, W, A] fp32, ``window`` [B] int32, ``sigmas`` [K] fp32,
    ``K <= 256``, all contiguous on one ROCm device.  A row depends on its window number, the draw and the table only."""
    if not torch.is_tensor(actions) or actions.dim() != 3 or actions.device.type != "cuda":
        raise ValueError(f"noise_levels: actions must be a [B, W, A] tensor on a ROCm device, got {tuple(getattr(actions, 'shape', ()))}")
    if isinstance(draw, bool) or not isinstance(draw, int) or not 0 <= draw < 2 ** 32:
        raise ValueError(f"draw must be an int in 0..2^32 - 1, got {draw!r}")
    B, W, A = actions.shape
    K = sigmas.shape[0] if torch.is_tensor(sigmas) and sigmas.dim() == 1 else 0
    if not 1 <= B <= MAX_BATCH or W < 1 or A < 1 or W * A > MAX_WINDOW_FLOATS or not 1 <= K <= MAX_LEVELS:
        raise ValueError(f"noise_levels: needs 1 <= B <= {MAX_BATCH}, 1 <= W * A <= {MAX_WINDOW_FLOATS} and 1 <= K <= {MAX_LEVELS}, got {(B, W, A)}, K = {K}")
    dev = actions.device
    for name, t, shape, dt in (("actions", actions, (B, W, A), torch.float32), ("noise", noise, (B, W, A), torch.float32),
                               ("window", window, (B,), torch.int32), ("sigmas", sigmas, (K,), torch.float32)):
        _same(name, "noise_levels", t, shape, dt, dev)
    level = torch.empty(B, dtype=torch.int32, device=dev)
    sigma = torch.empty(B, dtype=torch.float32, device=dev)
    x = torch.empty(B, W, A, dtype=torch.float32, device=dev)
    d = _lib.ModeValLevelsDesc(actions=actions.data_ptr(), noise=noise.data_ptr(), window=window.data_ptr(), sigmas=sigmas.data_ptr(), B=B, W=W, A=A, K=K,
                               draw=draw, level=level.data_ptr(), sigma=sigma.data_ptr(), x=x.data_ptr())
    _launch(_lib.load().mode_val_noise_levels, d, dev)
    return level, sigma, x


def level_error(pred: torch.Tensor, target: torch.Tensor, level: torch.Tensor, sq: torch.Tensor, cnt: torch.Tensor, mask: Optional[torch.Tensor] = None,
                weight: Optional[torch.Tensor] = None, accumulate: bool = True) -> None:
    """``mode_level_error`` on the current stream: ``action_error`` without ``unit`` and ``ab``, binned by ``level`` [B] int32 -

        sq[k, w * A + a] (+)= sum over {b: level[b] == k} of c e^2,   cnt[k, w] (+)= sum over {b: level[b] == k} of c

    with ``sq`` [K, W * A] and ``cnt`` [K, W] fp64, ``K <= 256``.  A row whose level is outside ``0..K-1`` counts nowhere; rows of another level and
    terms with ``c == 0`` are skipped, so ``pred`` may hold anything there.  Level ``k``'s slice has the bits ``action_error`` gives with the weight
    zeroed on every other level's rows."""
    if not torch.is_tensor(pred) or pred.dim() != 3 or pred.device.type != "cuda":
        raise ValueError(f"level_error: pred must be a [B, W, A] tensor on a ROCm device, got {tuple(getattr(pred, 'shape', ()))}")
    B, W, A = pred.shape
    K = cnt.shape[0] if torch.is_tensor(cnt) and cnt.dim() == 2 else 0
    if not 1 <= B <= MAX_BATCH or W < 1 or A < 1 or W * A > MAX_WINDOW_FLOATS or not 1 <= K <= MAX_LEVELS:
        raise ValueError(f"level_error: needs 1 <= B <= {MAX_BATCH}, 1 <= W * A <= {MAX_WINDOW_FLOATS} and cnt [K, W] with 1 <= K <= {MAX_LEVELS}, "
                         f"got {(B, W, A)}, cnt {tuple(getattr(cnt, 'shape', ()))}")
    for name, t, shape, dt in (("pred", pred, (B, W, A), torch.float32), ("target", target, (B, W, A), torch.float32), ("mask", mask, (B, W), torch.float32),
                               ("weight", weight, (B,), torch.float32), ("level", level, (B,), torch.int32), ("sq", sq, (K, W * A), torch.float64),
                               ("cnt", cnt, (K, W), torch.float64)):
        if t is None and name in ("mask", "weight"):
            continue
        _same(name, "level_error", t, shape, dt, pred.device)
    d = _lib.ModeLevelErrorDesc(pred=_ptr(pred), target=_ptr(target), mask=_ptr(mask), weight=_ptr(weight), level=_ptr(level), sq=_ptr(sq),
                                cnt=_ptr(cnt), B=B, W=W, A=A, K=K, accumulate=1 if accumulate else 0)
    _launch(_lib.load().mode_level_error, d, pred.device)


def level_table(levels="density", num_levels: int = 16, sigma_min: float = 0.001, sigma_max: float = 80.0, num_sampling_steps: int = 10,
                sigma_data: float = 0.5) -> torch.Tensor:
    """The noise levels of a ``LevelValidator`` as a 1-d CPU tensor (fp64 for ``"density"``, else as given), before the cast to fp32:

        "density"   the K = num_levels quantiles u_k = (k + 0.5) / K of the shipped training density - ``utils.rand_log_logistic(u=)`` with
                    loc = ln(sigma_data), scale = 0.5, truncated to [sigma_min, sigma_max], in its fp64 arithmetic.  Each level stands for 1 / K of the
                    density's mass, so the equal-weight mean over the levels estimates the training loss's expectation over sigma.
        "schedule"  ``get_sigmas_exponential(num_sampling_steps, sigma_min, sigma_max)`` without its trailing 0: the levels the sampler visits.
        a sequence  or 1-d tensor of finite positive values, taken as it is."""
    from .gc_sampling import get_sigmas_exponential
    from .utils import rand_log_logistic
    if isinstance(levels, str):
        if levels == "density":
            K = num_levels
            if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= MAX_LEVELS:
                raise ValueError(f"num_levels must be an int in 1..{MAX_LEVELS}, got {K!r}")
            if not (0 < sigma_min < sigma_max and math.isfinite(sigma_max) and sigma_data > 0):
                raise ValueError(f"needs 0 < sigma_min < sigma_max < inf and sigma_data > 0, got {sigma_min!r}, {sigma_max!r}, {sigma_data!r}")
            u = (torch.arange(K, dtype=torch.float64) + 0.5) / K
            table = rand_log_logistic((K,), loc=math.log(sigma_data), scale=0.5, min_value=sigma_min, max_value=sigma_max, dtype=torch.float64, u=u)
        elif levels == "schedule":
            n = num_sampling_steps
            if isinstance(n, bool) or not isinstance(n, int) or n < 1:
                raise ValueError(f"num_sampling_steps must be an int >= 1, got {n!r}")
            table = get_sigmas_exponential(n, sigma_min, sigma_max)[:n].clone()
        else:
            raise ValueError(f"levels must be 'density', 'schedule' or a sequence of noise levels, got {levels!r}")
    else:
        try:
            table = torch.as_tensor(levels).detach().cpu()
        except (TypeError, ValueError, RuntimeError) as e:
            raise ValueError(f"levels must be 'density', 'schedule' or a sequence of noise levels, got {type(levels).__name__}") from e
        if table.dim() != 1 or table.dtype == torch.bool or table.is_complex():
            raise ValueError(f"levels must be a 1-d sequence of numbers, got shape {tuple(table.shape)}, {table.dtype}")
        if not table.is_floating_point():
            table = table.to(torch.float64)
    if not 1 <= table.numel() <= MAX_LEVELS:
        raise ValueError(f"the level table needs 1..{MAX_LEVELS} entries, got {table.numel()}")
    as32 = table.to(torch.float32)
    if not bool((torch.isfinite(as32) & (as32 > 0)).all()):
        raise ValueError("every noise level must be finite and positive as an fp32 value")
    return table


class LevelResult(dict):
    """What ``LevelValidator.run`` returns: device tensors, nothing read back.

        sigmas [K] fp32; the accumulators sq [K, W, A] and cnt [K, W] (fp64, the model's normalised units); count_per_level [K];
        mse_per_level [K], mse_per_level_step [K, W], mse_per_level_dim [K, A]: means of |D - a|^2 over the real steps (and action dimensions) of a
            level - with ``unit`` [A] fp64 in raw action units, ``unit[a]^2`` applied per dimension in fp64 here;
        loss_per_level [K] = lambda(sigma_k) * sum_{w, a} sq[k] / (A * sum_w cnt[k]), lambda = (sigma^2 + sigma_data^2) / (sigma sigma_data)^2 =
            1 / c_out^2 in fp64 from the fp32 level: ``GCDenoiser.loss``'s masked mean at that level (F - target = (D - a) / c_out), always in the
            model's own units;
        loss: the mean of loss_per_level over the levels with a positive count.

    A mean over nothing is 0.  Accumulators of several ranks (or passes) over the same table add: ``LevelResult.from_sums(sq, cnt, sigmas,
    sigma_data, unit)`` derives the means of the sums."""

    @classmethod
    def from_sums(cls, sq: torch.Tensor, cnt: torch.Tensor, sigmas: torch.Tensor, sigma_data: float, unit: Optional[torch.Tensor] = None) -> "LevelResult":
        K, W = cnt.shape
        sq = sq.reshape(K, W, -1)
        A = sq.shape[2]
        count = cnt.sum(1)
        raw = sq if unit is None else sq * (unit.to(sq) * unit.to(sq))
        s = sigmas.to(sq)
        lam = (s * s + sigma_data ** 2) / (s * sigma_data) ** 2
        loss_k = lam * _mean(sq.sum((1, 2)), A * count)
        live = (count > 0).to(sq)
        return cls(sigmas=sigmas, sq=sq, cnt=cnt, count_per_level=count, mse_per_level=_mean(raw.sum((1, 2)), A * count),
                   mse_per_level_step=_mean(raw.sum(2), A * cnt), mse_per_level_dim=_mean(raw.sum(1), count[:, None].expand(K, A)),
                   loss_per_level=loss_k, loss=_mean((loss_k * live).sum(), live.sum()))


class LevelValidator:
    """The held-out denoising (score-matching) loss resolved by noise level: the training objective itself on held-out windows, one denoiser
    evaluation per window instead of a sampler run, accumulated on the device per level of a fixed sigma table.

    ``levels`` / ``num_levels`` / ``sigma_min`` / ``sigma_max`` / ``num_sampling_steps``: the table, see ``level_table`` (``"density"``, the default:
    quantiles of the training density, whose equal-weight mean - ``result["loss"]`` - estimates the training loss; ``"schedule"``: the levels the
    sampler visits; or explicit values).  It is cast to fp32 once and lives on the device; at most 256 levels.

    ``batch(i, draw=0)``: the sweep's batch with unit-normal noise (``noise_scale=1.0``) plus ``level`` [B] int32, ``sigma`` [B] fp32 and
    ``noised`` [B, W, A] from one ``mode_val_noise_levels`` launch: window g meets level ``(g + draw) mod K`` with the noise of (g, draw), whatever
    the batch size - two checkpoints are compared on the same draws, and draws ``0..K-1`` give every window every level exactly once.

    ``predict(batch) -> [B, W, A]``: ``denoiser(embed(batch), batch["noised"], batch["latent_goal"], batch["sigma"])`` under ``no_grad`` in eval
    mode - ``MoDeDiT.denoise`` on the HIP chain with one sigma per row.  ``denoiser.guidance_scale`` is left as the caller set it; the training loss
    corresponds to ``None``.

    ``run(draws=None, ema=None) -> LevelResult``: ``draws`` defaults to K, the full window x level cross.  Eval mode, the EMA swap and the restore
    in a ``finally`` are ``Validator.run``'s.  Per batch: one sweep launch (two with cameras; one more with hindsight goals), the prep launch,
    ``embed``, one denoiser evaluation and one ``mode_level_error`` launch weighted by ``valid * action_mask``; nothing is read back.
    ``raw_units`` as in ``Validator``: the ``mse_*`` entries in the store's raw action units, a constant dimension contributing nothing;
    ``loss_per_level`` and ``loss`` stay in the model's units.

    Not here: continuous or jittered sigma inside a bin, per-level expert-utilisation statistics, pre-cached routing per level, capturing the
    per-batch chain as one graph, and gathering across ranks (the accumulators add: ``LevelResult.from_sums``)."""

    def __init__(self, denoiser, sweep: WindowSweep, embed: Callable[[dict], dict], levels="density", num_levels: int = 16, sigma_min: float = 0.001,
                 sigma_max: float = 80.0, num_sampling_steps: int = 10, raw_units: bool = True):
        _check_validator_args("LevelValidator", sweep, embed)
        st = sweep.store
        self.denoiser, self.sweep, self.embed = denoiser, sweep, embed
        self.sigma_data = float(denoiser.sigma_data)
        table = level_table(levels, num_levels, sigma_min, sigma_max, num_sampling_steps, self.sigma_data)
        self.sigmas = table.to(torch.float32).to(st.device).contiguous()
        self.unit = _raw_unit(st, raw_units)

    def __len__(self) -> int:
        return len(self.sweep)

    @property
    def num_levels(self) -> int:
        return self.sigmas.shape[0]

    def batch(self, i: int, draw: int = 0) -> dict:
        b = self.sweep.batch(i, draw, noise_scale=1.0)
        b["level"], b["sigma"], b["noised"] = noise_levels(b["actions"], b["noise"], b["window"], self.sigmas, int(draw))
        return b

    @torch.no_grad()
    def predict(self, batch: dict) -> torch.Tensor:
        self.denoiser.eval()
        return self.denoiser(self.embed(batch), batch["noised"], batch["latent_goal"], batch["sigma"])

    @torch.no_grad()
    def run(self, draws: Optional[int] = None, ema=None) -> LevelResult:
        K, W, A, dev = self.num_levels, self.sweep.window, self.sweep.store.action_dim, self.sweep.store.device
        draws = K if draws is None else draws
        _check_draws(draws)
        sq = torch.zeros(K, W * A, dtype=torch.float64, device=dev)
        cnt = torch.zeros(K, W, dtype=torch.float64, device=dev)
        _held_out_pass(self, self.denoiser, draws, ema, lambda b: level_error(
            self.predict(b).to(torch.float32).contiguous(), b["actions"], b["level"], sq, cnt, mask=b["action_mask"], weight=b["valid"]))
        return LevelResult.from_sums(sq, cnt, self.sigmas, self.sigma_data, self.unit)
