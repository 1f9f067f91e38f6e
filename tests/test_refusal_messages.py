"""CPU: the full text of every refusal of data.py and validation.py that needs no device - the constructors, split_episodes, mixture_weights,
epoch_of, level_table, mse_executed and batch() up to its device check.  The messages are part of the interface (callers and logs quote them):
each case states one as a literal, so that a change to how the checks are written cannot reword one unnoticed.  No kernel is launched here."""
import numpy as np
import pytest
import torch

from mode_diffusion_policy_amd import data, validation

A, G, W = 3, 5, 4
LENGTHS = (1, 3, 4, 7)
EMBED = "embed must be a function batch -> {'state_images': [B, n_img_tokens, obs_dim]}"
ROCM = "the store must be on a ROCm device (there is no CPU path), got cpu"


def open_store(step_goals=False):
    st = data.EpisodeStore(A, G, device="cpu")
    for n in LENGTHS:
        st.add_episode(np.zeros((n, A), np.float32), np.zeros(G, np.float32), step_goals=np.zeros((n, G), np.float32) if step_goals else None)
    return st


def store(step_goals=False):
    return open_store(step_goals).finalize(None)


def stream(**kw):
    return data.WindowStream(store(), **{**dict(batch_size=8, window=W), **kw})


def sweep(**kw):
    return data.WindowSweep(store(), **{**dict(batch_size=8, window=W), **kw})          # 15 windows: two batches


def mix(**kw):
    return data.mixture_weights(store(), **{**dict(groups=[0, 1, 0, 1], group_weights=(1.0, 2.0)), **kw})


class Den:
    sigma_data = 0.5


def level_validator():
    return validation.LevelValidator(Den(), sweep(), lambda b: b, levels=[0.5, 1.0])


def result():
    return validation.ValidationResult.from_sums(torch.zeros(W * A, dtype=torch.float64), torch.zeros(W * A, dtype=torch.float64),
                                                 torch.zeros(W, dtype=torch.float64))


CASES = []


def case(name, fn, message):
    CASES.append(pytest.param(fn, message, id=name))


# ---- data.EpisodeStore
for v in (0, -1, True, 2.5):
    case(f"store-action_dim-{v!r}", lambda v=v: data.EpisodeStore(v, G, device="cpu"), f"action_dim must be a positive int, got {v!r}")
case("store-goal_dim", lambda: data.EpisodeStore(A, 0, device="cpu"), "goal_dim must be a positive int, got 0")
case("normalize-text", lambda: open_store().finalize(("a", "b")), "normalize must be 'minmax', None or (lo, hi), got ('a', 'b')")
case("normalize-tensor-shape", lambda: open_store().finalize((torch.zeros(2), torch.ones(2))),
     "normalize=(lo, hi) needs two finite [3] vectors with hi >= lo")

# ---- data.split_episodes
case("split-no-store", lambda: data.split_episodes(object(), 0.5), "split_episodes needs an EpisodeStore")
case("split-neither", lambda: data.split_episodes(store()), "give exactly one of val_fraction and val_episodes")
case("split-both", lambda: data.split_episodes(store(), 0.5, [0]), "give exactly one of val_fraction and val_episodes")
for v in (0.0, 1.0, -0.5, 1.5, True, "x", float("nan"), float("inf"), 0, 1):
    case(f"split-fraction-{v!r}", lambda v=v: data.split_episodes(store(), v), f"val_fraction must lie strictly inside (0, 1), got {v!r}")
case("split-ids-text", lambda: data.split_episodes(store(), val_episodes="abc"), "val_episodes must be a 1-d sequence of ints, got <U3 ()")
case("split-ids-ragged", lambda: data.split_episodes(store(), val_episodes=[[1], [1, 2]]), "val_episodes must be a sequence of episode ids")
case("split-ids-2d", lambda: data.split_episodes(store(), val_episodes=[[0]]), "val_episodes must be a 1-d sequence of ints, got int64 (1, 1)")
case("split-ids-float", lambda: data.split_episodes(store(), val_episodes=[0.5]), "val_episodes must be a 1-d sequence of ints, got float64 (1,)")
case("split-ids-tensor-range", lambda: data.split_episodes(store(), val_episodes=torch.tensor([0, 9])), "val_episodes holds an id outside 0..3")
case("split-ids-repeat", lambda: data.split_episodes(store(), val_episodes=[0, 0]), "val_episodes repeats an id")
case("split-empty-side", lambda: data.split_episodes(store(), val_episodes=[0, 1, 2, 3]),
     "the split leaves a side empty: 0 training and 4 validation episodes of 4")

# ---- what data.WindowStream and data.WindowSweep share
for who, make in (("WindowStream", stream), ("WindowSweep", sweep)):
    verb = "draw" if who == "WindowStream" else "sweep"
    case(f"{who}-open-store", lambda who=who: getattr(data, who)(open_store(), 8, W), f"{who} needs a finalized EpisodeStore")
    for v in (0, 65536, True, 2.0, None):
        case(f"{who}-batch_size-{v!r}", lambda make=make, v=v: make(batch_size=v), f"batch_size must be an int in 1..65535, got {v!r}")
    for v in (0, 4097, False, "4"):
        case(f"{who}-window-{v!r}", lambda make=make, v=v: make(window=v), f"window must be an int in 1..4096, got {v!r}")
    for v in (-1, 2 ** 32, True, 0.0):
        case(f"{who}-seed-{v!r}", lambda make=make, v=v: make(seed=v), f"seed must be an int in 0..4294967295, got {v!r}")
    case(f"{who}-window-floats", lambda make=make: make(window=2000), "window * action_dim must be at most 4096, got 2000 * 3")
    case(f"{who}-pad", lambda make=make: make(pad="zero"), "pad must be one of ('hold', 'none'), got 'zero'")
    for v in (1.5, -0.1, True, "x", float("nan"), None):
        case(f"{who}-hindsight_prob-{v!r}", lambda make=make, v=v: make(hindsight_prob=v), f"hindsight_prob must lie in [0, 1], got {v!r}")
    case(f"{who}-no-step_goals", lambda make=make: make(goal="hindsight", goal_horizon=(0, 1)),
         f"{who}(goal='hindsight') needs a store with step_goals (EpisodeStore.add_episode(step_goals=))")
    case(f"{who}-nothing-fits", lambda make=make: make(window=8, pad="none"), f"no window of 8 steps fits any episode (pad='none'): nothing to {verb}")
    case(f"{who}-nothing-selected-fits", lambda make=make: make(pad="none", episodes=[0, 1]),
         f"no window of 4 steps fits any selected episode (pad='none'): nothing to {verb}")
    case(f"{who}-episodes-range", lambda make=make: make(episodes=[4]), "episodes holds an id outside 0..3")
    case(f"{who}-episodes-tensor-bool", lambda make=make: make(episodes=torch.tensor([True, False])),
         "episodes must be a 1-d sequence of ints, got bool (2,)")

# ---- data.WindowStream
case("stream-order", lambda: stream(order="shuffle"), "order must be one of ('iid', 'epoch'), got 'shuffle'")
case("stream-weights-text", lambda: stream(episode_weights="abcd"), "episode_weights must be a sequence of numbers, one per episode")
case("stream-weights-tensor-shape", lambda: stream(episode_weights=torch.ones(3)),
     "episode_weights must hold one number per episode of the store (4), got shape (3,)")
for v in (-1, 2 ** 32, 1.5, True, None):
    case(f"stream-epoch_of-{v!r}", lambda v=v: stream(order="epoch").epoch_of(v), f"step must be an int in 0..2^32 - 1, got {v!r}")
    case(f"stream-batch-step-{v!r}", lambda v=v: stream().batch(v), f"step must be an int in 0..2^32 - 1, got {v!r}")
case("stream-batch-device", lambda: stream().batch(0), "WindowStream.batch: " + ROCM)
case("stream-batch-device-ordered", lambda: stream(order="epoch").batch(np.int64(3)), "WindowStream.batch: " + ROCM)

# ---- data.WindowSweep
for v in (0, -2, True, 1.5):
    case(f"sweep-stride-{v!r}", lambda v=v: sweep(stride=v), f"stride must be an int >= 1, got {v!r}")
case("sweep-noise_scale", lambda: sweep(noise_scale=float("inf")), "noise_scale must be a finite number, got inf")
case("sweep-batch-noise_scale", lambda: sweep().batch(0, noise_scale=float("nan")), "noise_scale must be a finite number, got nan")
for v in (-1, 2, True, 0.0):
    case(f"sweep-batch-index-{v!r}", lambda v=v: sweep().batch(v), f"batch index must be an int in 0..1, got {v!r}")
for v in (-1, 2 ** 32, False, 1.0):
    case(f"sweep-batch-draw-{v!r}", lambda v=v: sweep().batch(0, v), f"draw must be an int in 0..2^32 - 1, got {v!r}")
case("sweep-batch-device", lambda: sweep().batch(np.int32(1), np.int64(2)), "WindowSweep.batch: " + ROCM)

# ---- data.mixture_weights
case("mix-open-store", lambda: data.mixture_weights(open_store(), [], ()), "mixture_weights needs a finalized EpisodeStore")
case("mix-pad", lambda: mix(pad="zero"), "pad must be one of ('hold', 'none'), got 'zero'")
for v in (None, 0, True, 2.0):
    case(f"mix-window-{v!r}", lambda v=v: mix(pad="none", window=v), f"pad='none' needs window, an int >= 1, got {v!r}")
case("mix-nothing-fits", lambda: mix(pad="none", window=8), "no window fits any selected episode: nothing to weigh")
case("mix-weights-text", lambda: mix(group_weights="ab"), "groups must be a sequence of ints and group_weights a sequence of numbers")
case("mix-weights-sum", lambda: mix(group_weights=(0, 0)),
     "group_weights must be a non-empty 1-d sequence of finite non-negative numbers with a positive sum")
case("mix-groups-tensor-size", lambda: mix(groups=torch.tensor([0, 1, 0])), "groups must hold one int in 0..1 per episode of the store (4)")
case("mix-groups-float", lambda: mix(groups=[0.0, 1, 0, 1]), "groups must hold one int in 0..1 per episode of the store (4)")
case("mix-group-without-start", lambda: mix(episodes=[0, 2]), "group 1 has a positive weight but no window start")

# ---- validation: the constructors, run(draws=), level_table, mse_executed and the launch wrappers up to their device check
for who in ("Validator", "LevelValidator"):
    case(f"{who}-no-sweep", lambda who=who: getattr(validation, who)(Den(), object(), lambda b: b), f"{who} needs a data.WindowSweep, got object")
    case(f"{who}-no-sweep-stream", lambda who=who: getattr(validation, who)(Den(), stream(), lambda b: b),
         f"{who} needs a data.WindowSweep, got WindowStream")
    case(f"{who}-embed", lambda who=who: getattr(validation, who)(Den(), sweep(), None), EMBED)
for v in (0, -1, True, 1.5, np.int64(1)):                                                      # validation takes a Python int only
    case(f"LevelValidator-run-draws-{v!r}", lambda v=v: level_validator().run(draws=v), f"draws must be an int >= 1, got {v!r}")
    case(f"Validator-run-draws-{v!r}", lambda v=v: validation.Validator(Den(), sweep(), lambda b: b).run(draws=v),
         f"draws must be an int >= 1, got {v!r}")
for v in (0, 257, 2.0, True, np.int64(4)):
    case(f"level_table-num_levels-{v!r}", lambda v=v: validation.level_table("density", num_levels=v), f"num_levels must be an int in 1..256, got {v!r}")
for v in (0, False, np.int64(3)):
    case(f"level_table-steps-{v!r}", lambda v=v: validation.level_table("schedule", num_sampling_steps=v),
         f"num_sampling_steps must be an int >= 1, got {v!r}")
case("level_table-kind", lambda: validation.level_table("quantiles"),
     "levels must be 'density', 'schedule' or a sequence of noise levels, got 'quantiles'")
case("level_table-size", lambda: validation.level_table([0.5] * 257), "the level table needs 1..256 entries, got 257")
case("level_table-values", lambda: validation.level_table([0.0, 1.0]), "every noise level must be finite and positive as an fp32 value")
for v in (0, W + 1, True, 1.0, np.int64(1)):
    case(f"mse_executed-{v!r}", lambda v=v: result().mse_executed(v), f"multistep must be an int in 1..{W}, got {v!r}")
case("action_error-device", lambda: validation.action_error(torch.zeros(2, W, A), None, None, None, None),
     f"action_error: pred must be a [B, W, A] tensor on a ROCm device, got (2, {W}, {A})")
case("level_error-device", lambda: validation.level_error(torch.zeros(2, W, A), None, None, None, None),
     f"level_error: pred must be a [B, W, A] tensor on a ROCm device, got (2, {W}, {A})")
case("noise_levels-device", lambda: validation.noise_levels(torch.zeros(2, W, A), None, None, None),
     f"noise_levels: actions must be a [B, W, A] tensor on a ROCm device, got (2, {W}, {A})")


@pytest.mark.parametrize("fn, message", CASES)
def test_refusal_text(fn, message):
    with pytest.raises(ValueError) as e:
        fn()
    assert str(e.value) == message


def test_numpy_ints_are_taken_where_python_ints_are():
    """The other side of the int checks of data.py: a numpy integer is an int there (validation.py takes a Python int only, above)."""
    st = store()
    ws = data.WindowStream(st, np.int64(8), np.int32(W), seed=np.uint32(7), order="epoch")
    assert (ws.batch_size, ws.window, ws.seed) == (8, W, 7) and all(type(v) is int for v in (ws.batch_size, ws.window, ws.seed))
    assert ws.epoch_of(np.int64(4)) == 2
    sw = data.WindowSweep(st, 8, W, stride=np.int64(2))
    assert sw.stride == 2 and type(sw.stride) is int and len(sw) == 2
    assert data.mixture_weights(st, [0, 1, 0, 1], (1.0, 2.0), window=np.int64(W), pad="none").shape == (4,)
    assert data.EpisodeStore(np.int64(A), np.int32(G), device="cpu").action_dim == A
