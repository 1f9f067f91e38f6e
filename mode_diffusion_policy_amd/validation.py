"""Validation without a simulator, on the device: the reference's ``validation_step`` (mode_agent.py:442-464) - run the INFERENCE sampler on
held-out windows and measure the error between the sampled chunk and the demonstrated actions - as a loop that reads nothing back.

``data.WindowSweep`` hands out every held-out window exactly once (one launch per batch), ``Validator.predict`` plans a chunk for the batch on the
path ``ChunkedRolloutPolicy.denoise_actions`` takes (one hipGraph replay for the fused samplers), and ``mode_action_error`` (csrc/data_stream.hip;
formulas and summation order: include/mode_hip.h) adds the batch's masked squared and absolute errors into fp64 accumulators on the device.  The
caller's ``float(result["mse"])`` is the only host sync of a validation pass.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Optional

import torch

from .data import MAX_BATCH, MAX_WINDOW_FLOATS, WindowSweep
from .rollout import ChunkedRolloutPolicy


def action_error(pred: torch.Tensor, target: torch.Tensor, sq: torch.Tensor, ab: torch.Tensor, cnt: torch.Tensor, mask: Optional[torch.Tensor] = None,
                 weight: Optional[torch.Tensor] = None, unit: Optional[torch.Tensor] = None, accumulate: bool = True) -> None:
    """``mode_action_error`` on the current stream: with ``c[b, w] = weight[b] * mask[b, w]`` (an absent factor is 1, a value that is not > 0 counts as
    0) and ``e = (pred - target) * unit[a]`` in fp64 from the fp32 difference,

        sq[w * A + a] (+)= sum_b c e^2,   ab[w * A + a] (+)= sum_b c |e|,   cnt[w] (+)= sum_b c

    ``pred``, ``target`` [B, W, A] fp32, ``mask`` [B, W] fp32, ``weight`` [B] fp32, ``unit`` [A] fp64, ``sq`` / ``ab`` [W * A] and ``cnt`` [W] fp64, all
    contiguous on one ROCm device.  Terms with ``c == 0`` are skipped, so ``pred`` may hold anything there.  No atomics: the result's bits depend on
    the shapes and the order of the calls only.  ``accumulate=False`` stores instead of adding."""
    from . import _lib as L
    from .engine import _stream
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
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or t.device != pred.device or not t.is_contiguous():
            raise ValueError(f"action_error: {name} must be a contiguous {dt} {shape} tensor on {pred.device}, got "
                             f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
    p = lambda t: None if t is None else t.data_ptr()
    d = L.ModeActionErrorDesc(pred=p(pred), target=p(target), mask=p(mask), weight=p(weight), unit=p(unit), sq=p(sq), ab=p(ab), cnt=p(cnt), B=B, W=W, A=A,
                              accumulate=1 if accumulate else 0)
    with torch.cuda.device(pred.device):
        L.check(L.load().mode_action_error(C.byref(d), _stream()), "action_error")


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
        mean = lambda num, den: torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
        return cls(sq=sq, ab=ab, cnt=cnt, count=count, mse=mean(sq.sum(), A * count), mae=mean(ab.sum(), A * count),
                   mse_per_step=mean(sq.sum(1), A * cnt), mse_per_dim=mean(sq.sum(0), count.expand(A)))

    def mse_executed(self, multistep: int) -> torch.Tensor:
        W, A = self["sq"].shape
        if isinstance(multistep, bool) or not isinstance(multistep, int) or not 1 <= multistep <= W:
            raise ValueError(f"multistep must be an int in 1..{W}, got {multistep!r}")
        num, den = self["sq"][:multistep].sum(), A * self["cnt"][:multistep].sum()
        return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))


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

    Not here: a held-out score-matching loss per noise level (``GCDenoiser.loss`` on ``WindowSweep`` batches gives one), encoding goal frames (the
    sweep gathers stored embeddings; ``batch["goal_index"]`` names the frame for an encoder of the caller's), disk formats, and gathering results
    across ranks - rank ``r`` of ``n`` may run the batches ``r, r + n, ...`` itself and sum the returned accumulators
    (``ValidationResult.from_sums``)."""

    def __init__(self, denoiser, sweep: WindowSweep, embed: Callable[[dict], dict], num_sampling_steps: int = 10, sigma_min: float = 0.001,
                 sigma_max: float = 80.0, noise_scheduler: str = "exponential", sampler_type: str = "ddim", raw_units: bool = True):
        if not isinstance(sweep, WindowSweep):
            raise ValueError(f"Validator needs a data.WindowSweep, got {type(sweep).__name__}")
        if not callable(embed):
            raise ValueError("embed must be a function batch -> {'state_images': [B, n_img_tokens, obs_dim]}")
        st = sweep.store
        self.sweep, self.embed, self.sigma_max = sweep, embed, float(sigma_max)
        self.policy = ChunkedRolloutPolicy(denoiser, num_sampling_steps=num_sampling_steps, sigma_min=sigma_min, sigma_max=sigma_max,
                                           noise_scheduler=noise_scheduler, sampler_type=sampler_type, act_window_size=sweep.window,
                                           multistep=sweep.window, action_dim=st.action_dim)
        self.unit = None
        if raw_units and st.scale is not None:
            s = st.scale.to(torch.float64)
            self.unit = torch.where(s != 0, 1.0 / torch.where(s != 0, s, torch.ones_like(s)), torch.zeros_like(s)).contiguous()

    def __len__(self) -> int:
        return len(self.sweep)

    def batch(self, i: int, draw: int = 0) -> dict:
        return self.sweep.batch(i, draw, noise_scale=self.sigma_max)

    @torch.no_grad()
    def predict(self, batch: dict) -> torch.Tensor:
        return self.policy.denoise_actions(self.embed(batch), batch["latent_goal"], x=batch["noise"])

    @torch.no_grad()
    def run(self, draws: int = 1, ema=None) -> ValidationResult:
        if isinstance(draws, bool) or not isinstance(draws, int) or draws < 1:
            raise ValueError(f"draws must be an int >= 1, got {draws!r}")
        den, sw = self.policy.model, self.sweep
        W, A, dev = sw.window, sw.store.action_dim, sw.store.device
        modes = [(m, m.training) for m in den.modules()]
        sq, ab = (torch.zeros(W * A, dtype=torch.float64, device=dev) for _ in range(2))
        cnt = torch.zeros(W, dtype=torch.float64, device=dev)
        if ema is not None:
            ema.swap()
        try:
            den.eval()
            for draw in range(draws):
                for i in range(len(sw)):
                    b = self.batch(i, draw)
                    action_error(self.predict(b).to(torch.float32).contiguous(), b["actions"], sq, ab, cnt,mask=b["action_mask"], weight=b["valid"], unit=self.unit)
        finally:
            if ema is not None:
                ema.swap()
            for m, was in modes:
                m.training = was
        return ValidationResult.from_sums(sq, ab, cnt)
