"""CPU: the numpy restatement of hindsight goal relabelling (tests/goal_refs.py) against what include/mode_hip.h promises for
mode_data_relabel_goals, and the host side of the feature - EpisodeStore(step_goal_dtype=).add_episode(step_goals=) and the goal keywords of
data.WindowStream / data.WindowSweep.  No kernel is launched here."""
import numpy as np
import pytest
import torch

import data_refs as R
import goal_refs as GR
import val_refs as V
from mode_diffusion_policy_amd import data

W, A, G = 4, 3, 5
KEYS = ((0, 0), (7, 3), (123, 1000))          # (seed, step) of the statistical checks


def tables(W=W):
    lengths = GR.episode_lengths(W)
    return lengths, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def stream_rows(seed, step, B, W=W):
    """index, episode of a WindowStream(pad="hold") batch on the test store."""
    b = R.sample_windows(GR.make_store(W, A, G, seed=2), W, B, seed, step, "hold")
    return b["index"], b["episode"]


def test_goal_steps_stay_inside_the_episode_and_the_horizon():
    lengths, begin = tables()
    assert lengths == [1, 3, 4, 7]
    clamped = free = 0
    for seed, step in KEYS:
        index, episode = stream_rows(seed, step, 130)
        for lo, hi in ((0, 0), (1, 1), (0, 6), (3, 9), (GR.LAST, GR.LAST)):
            ref = GR.relabel(begin, index, episode, seed, step, lo, hi, GR.FULL)
            last = begin[episode.astype(np.int64) + 1] - 1
            assert np.array_equal(ref["last"], last)
            assert (ref["goal_index"] >= index).all() and (ref["goal_index"] <= last).all()
            assert (ref["d"] >= lo).all() and (ref["d"] <= hi).all()
            assert np.array_equal(ref["goal_offset"], np.minimum(ref["d"], last - index))
            assert np.array_equal(ref["goal_index"], index + ref["goal_offset"]) and ref["goal_index"].dtype == np.int32
            if (lo, hi) == (0, 0):
                assert np.array_equal(ref["goal_index"], index)
            if lo == GR.LAST:
                assert np.array_equal(ref["goal_index"], last)
            if (lo, hi) == (0, 6):
                assert len(set(ref["d"].tolist())) == 7                                  # every offset of the horizon is drawn
                clamped += int((ref["d"] > last - index).sum())
                free += int((ref["d"] < last - index).sum())
    assert clamped > 0 and free > 0                                                     # both sides of the episode's end are exercised


def test_a_row_depends_on_seed_step_and_id_only():
    lengths, begin = tables()
    seed, step, lo, hi, th = 11, 5, 0, 6, GR.thresh_of(0.5)
    i7, e7 = stream_rows(seed, step, 7)
    i130, e130 = stream_rows(seed, step, 130)
    r7, r130 = GR.relabel(begin, i7, e7, seed, step, lo, hi, th), GR.relabel(begin, i130, e130, seed, step, lo, hi, th)
    for k in ("goal_index", "goal_offset", "goal_kind"):
        assert np.array_equal(r7[k], r130[k][:7]), k
    assert 0 < r130["goal_kind"].sum() < 130
    again = GR.relabel(begin, i130, e130, seed, step, lo, hi, th)
    assert all(np.array_equal(again[k], r130[k]) for k in r130)
    other = GR.relabel(begin, i130, e130, seed, step + 1, lo, hi, th)
    assert not np.array_equal(other["d"], r130["d"]) and not np.array_equal(other["goal_kind"], r130["goal_kind"])
    # a sweep keys the draws by the window's number: window g gets the same goal at B = 3 and B = 8, padding rows that of the window they repeat
    eps = GR.make_store(W, A, G, seed=2)
    per_window = {}
    for B in (3, 8):
        n_total = int(V.sweep_table(lengths, W, 1, "hold")[-1])
        for i in range(V.num_batches(n_total, B)):
            b = V.sweep_windows(eps, W, B, i, 1, "hold")
            ref = GR.relabel(begin, b["index"], b["episode"], seed, 2, lo, hi, th, ids=b["window"])
            for j in range(B):
                got = (int(ref["goal_index"][j]), int(ref["goal_offset"][j]), float(ref["goal_kind"][j]))
                assert per_window.setdefault(int(b["window"][j]), got) == got
    assert sorted(per_window) == list(range(15))
    assert len({v[1] for v in per_window.values()}) > 1 and len({v[2] for v in per_window.values()}) == 2


def test_mixing_share_and_offset_shares_lie_inside_four_sigma():
    """4096 rows: sigma of a share p is sqrt(p (1 - p) / 4096) - 0.0068 at p = 0.25, 0.0055 at p = 1 / 7; the caps 0.03 and 0.025 are >= 4 sigma."""
    ids = np.arange(4096)
    assert 4 * np.sqrt(0.25 * 0.75 / 4096) < 0.03 and 4 * np.sqrt((1 / 7) * (6 / 7) / 4096) < 0.025
    for seed, step in KEYS:
        kind, d = GR.draws(seed, step, ids, 3, 9, GR.thresh_of(0.25))
        assert abs(kind.mean() - 0.25) <= 0.03, (seed, step, kind.mean())
        shares = np.bincount(d - 3, minlength=7) / 4096.0
        assert shares.shape == (7,) and (np.abs(shares - 1 / 7) <= 0.025).all(), (seed, step, shares)
        assert not GR.draws(seed, step, ids, 3, 9, 0)[0].any()                           # thresh = 0 relabels nothing
        assert GR.draws(seed, step, ids, 3, 9, GR.FULL)[0].all()                         # thresh = 2^32 relabels everything
    assert GR.thresh_of(0.0) == 0 and GR.thresh_of(1.0) == 2 ** 32 and GR.thresh_of(0.5) == 2 ** 31
    # the rows a threshold leaves out keep their episode goal, the others carry the stored step's embedding
    lengths, begin = tables()
    index, episode = stream_rows(7, 3, 64)
    sg = np.concatenate(GR.step_goal_table(GR.make_store(W, A, G, seed=2), G))
    goals = np.arange(4 * G, dtype=np.float32).reshape(4, G)
    ref = GR.relabel(begin, index, episode, 7, 3, 0, 6, GR.thresh_of(0.5))
    out = GR.relabelled_goals(goals[episode], sg, ref)
    on = ref["goal_kind"] == 1
    assert 0 < on.sum() < 64 and np.array_equal(out[~on], goals[episode][~on]) and np.array_equal(out[on], sg[ref["goal_index"][on]])


def _lowbias32(x):
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
    return x


def test_one_row_by_hand():
    """seed 7, step 3, row id 1 of a window that starts at row 9 of the episode [8, 15), horizon 3 .. 9, hindsight_prob 0.25 - in Python ints:
    h4 * 7 = 24665749864 = 5 * 2^32 + 3190913384, so d = 3 + 5 = 8 and the goal step 9 + 8 = 17 is held at the episode's last row 14;
    h5 = 388598871 < 2^30, so the row is relabelled."""
    seed, step, rid, lo, hi = 7, 3, 1, 3, 9
    k4 = _lowbias32((seed + 4) ^ ((0x9E3779B9 * (step + 1)) & 0xFFFFFFFF))
    k5 = _lowbias32((seed + 5) ^ ((0x9E3779B9 * (step + 1)) & 0xFFFFFFFF))
    h4, h5 = _lowbias32(k4 ^ rid), _lowbias32(k5 ^ rid)
    d = lo + ((h4 * (hi - lo + 1)) >> 32)
    kind = h5 < 2 ** 30
    r = min(9 + d, 14)
    begin = np.array([0, 1, 4, 8, 15])
    index, episode = np.full(6, 9), np.full(6, 3)
    ref = GR.relabel(begin, index, episode, seed, step, lo, hi, 2 ** 30)
    assert (int(ref["d"][1]), int(ref["goal_index"][1]), int(ref["goal_offset"][1]), float(ref["goal_kind"][1])) == (d, r, r - 9, float(kind))
    assert (k4, k5, h4, h5, d, r, kind) == (2966517509, 2866098989, 3523678552, 388598871, 8, 14, True)
    assert (int(ref["d"][5]), int(ref["goal_index"][5]), float(ref["goal_kind"][5])) == (3, 12, 0.0)      # row 5: h4 = 491124960, h5 = 3368719393
    # the same id given explicitly, at another place in the batch
    ref = GR.relabel(begin, index[:1], episode[:1], seed, step, lo, hi, 2 ** 30, ids=[1])
    assert (int(ref["goal_index"][0]), float(ref["goal_kind"][0])) == (r, float(kind))
    # bf16: round to nearest even, and the exact expansion
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0e38, 1e-40], np.float32)       # 1 + 2^-8: a tie, to even (down); 1 + 3 * 2^-8: a tie, up
    bits = GR.bf16_bits(x)
    assert bits[:3].tolist() == [0x3F80, 0x3F80, 0x3F82]
    assert np.array_equal(bits, torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(GR.bf16_expand(bits).view(np.uint32), torch.from_numpy(x).to(torch.bfloat16).float().numpy().view(np.uint32))


def test_store_takes_step_goals_for_every_episode_or_none():
    eps = GR.make_store(W, A, G, seed=2)
    sg = GR.step_goal_table(eps, G)
    st = data.EpisodeStore(A, G, device="cpu")
    assert st.step_goal_dtype == torch.float32
    st.add_episode(eps[0][0], eps[0][1], step_goals=sg[0])
    bad = [
        lambda s: s.add_episode(eps[1][0], eps[1][1]),                                                       # every episode or none
        lambda s: s.add_episode(eps[1][0], eps[1][1], step_goals=sg[2]),                                     # one embedding per step
        lambda s: s.add_episode(eps[1][0], eps[1][1], step_goals=sg[1][:, :4]),                              # the goal space's width
        lambda s: s.add_episode(eps[1][0], eps[1][1], step_goals=sg[1].astype(np.int32)),
        lambda s: s.add_episode(eps[1][0], eps[1][1], step_goals=sg[1].tolist()),
        lambda s: s.add_episode(eps[1][0], eps[1][1], step_goals=np.full((3, G), np.inf, np.float32)),
        lambda s: s.add_episode(eps[1][0], eps[1][1], step_goals=np.full((3, G), 1e39, np.float64)),         # overflows fp32
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call(st)
        assert st.num_steps == 1 and st.num_episodes == 1, i
    for e, s in zip(eps[1:], sg[1:]):
        st.add_episode(e[0], e[1], step_goals=torch.from_numpy(s).double())
    st.finalize()
    assert st.step_goals.dtype == torch.float32 and np.array_equal(st.step_goals.numpy().view(np.uint32), np.concatenate(sg).view(np.uint32))
    none = data.EpisodeStore(A, G, device="cpu")
    none.add_episode(eps[0][0], eps[0][1])
    with pytest.raises(ValueError, match="every episode or for none"):
        none.add_episode(eps[1][0], eps[1][1], step_goals=sg[1])
    assert none.finalize().step_goals is None
    # bf16: one round-to-nearest-even at upload; a value that would round to inf is refused
    half = data.EpisodeStore(A, G, device="cpu", step_goal_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="bf16"):
        half.add_episode(eps[0][0], eps[0][1], step_goals=np.full((1, G), 3.4e38, np.float32))
    for e, s in zip(eps, sg):
        half.add_episode(e[0], e[1], step_goals=s)
    half.finalize()
    assert half.step_goals.dtype == torch.bfloat16 and tuple(half.step_goals.shape) == (15, G)
    assert np.array_equal(half.step_goals.view(torch.int16).numpy().view(np.uint16), GR.bf16_bits(np.concatenate(sg)))
    for dt in (torch.float16, torch.float64, "bf16", None):
        with pytest.raises(ValueError, match="step_goal_dtype"):
            data.EpisodeStore(A, G, device="cpu", step_goal_dtype=dt)


def test_goal_keyword_refusals_need_no_device():
    eps = GR.make_store(W, A, G, seed=2)
    sg = GR.step_goal_table(eps, G)
    with_sg, without = data.EpisodeStore(A, G, device="cpu"), data.EpisodeStore(A, G, device="cpu")
    for e, s in zip(eps, sg):
        with_sg.add_episode(e[0], e[1], step_goals=s)
        without.add_episode(e[0], e[1])
    with_sg.finalize(), without.finalize()
    for cls in (data.WindowStream, data.WindowSweep):
        with pytest.raises(ValueError, match="step_goals"):
            cls(without, 8, W, goal="hindsight", goal_horizon=(0, 3))
        bad = [dict(goal="image"), dict(goal=None), dict(goal="hindsight"), dict(goal_horizon=(0, 3)), dict(goal="episode", goal_horizon=(0, 3)),
               dict(goal="hindsight", goal_horizon=(-1, 3)), dict(goal="hindsight", goal_horizon=(4, 3)), dict(goal="hindsight", goal_horizon=(0, 2 ** 31)),
               dict(goal="hindsight", goal_horizon=(0.0, 3)), dict(goal="hindsight", goal_horizon=(0, 3, 5)), dict(goal="hindsight", goal_horizon=(True, 3)),
               dict(goal="hindsight", goal_horizon="first"), dict(goal="hindsight", goal_horizon=(0, 3), hindsight_prob=-0.1),
               dict(goal="hindsight", goal_horizon=(0, 3), hindsight_prob=1.5), dict(goal="hindsight", goal_horizon=(0, 3), hindsight_prob=float("nan")),
               dict(goal="hindsight", goal_horizon=(0, 3), hindsight_prob="half"), dict(hindsight_prob=2.0)]
        if cls is data.WindowStream:                                                      # an int and "last" are the sweep's
            bad += [dict(goal="hindsight", goal_horizon=3), dict(goal="hindsight", goal_horizon="last")]
        else:
            bad += [dict(goal="hindsight", goal_horizon=-1), dict(goal="hindsight", goal_horizon=2 ** 31)]
        for kw in bad:
            with pytest.raises(ValueError):
                cls(with_sg, 8, W, **kw)
        ok = cls(with_sg, 8, W, goal="hindsight", goal_horizon=(0, 2 ** 31 - 1), hindsight_prob=0.25)
        assert ok.goal == "hindsight" and ok._goal_plan == (0, 2 ** 31 - 1, 2 ** 30)
        assert cls(with_sg, 8, W).goal == "episode" and cls(with_sg, 8, W)._goal_plan is None
    assert data.WindowSweep(with_sg, 8, W, goal="hindsight", goal_horizon="last")._goal_plan == (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 32)
    assert data.WindowSweep(with_sg, 8, W, goal="hindsight", goal_horizon=5, hindsight_prob=0)._goal_plan == (5, 5, 0)
    with pytest.raises(ValueError, match="ROCm"):
        data.WindowStream(with_sg, 8, W, goal="hindsight", goal_horizon=(0, 3)).batch(0)  # there is no CPU path
