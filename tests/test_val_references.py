"""CPU: the numpy references of the validation sweep and the masked action error (tests/val_refs.py) checked against what they restate, and the
host side of holding episodes out (data.split_episodes, the `episodes=` tables of data.WindowStream / data.WindowSweep)."""
import numpy as np
import pytest

import data_refs as R
import val_refs as V
from mode_diffusion_policy_amd import data

GEOMS = [(4, 3, 5), (10, 7, 512)]


@pytest.mark.parametrize("pad", ["none", "hold"])
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("W,A,G", GEOMS)
def test_counts_follow_stride_and_pad(W, A, G, stride, pad):
    lengths = R.episode_lengths(W)                                              # 1, W - 1, W, W + 3: two episodes shorter than a window
    n = V.window_counts(lengths, W, stride, pad)
    for L, got in zip(lengths, n):
        if pad == "hold":
            want = len(range(0, L, stride))                                     # every stride-th step starts a window
        else:
            want = len([p for p in range(0, L, stride) if p + W <= L])          # only windows inside the episode
        assert got == want, (L, got, want)
    assert (n[:2] == 0).all() if pad == "none" else (n > 0).all()
    if stride == 1:                                                             # stride 1 is the training stream's table
        assert np.array_equal(V.sweep_table(lengths, W, 1, pad), R.start_table(lengths, W, pad))


@pytest.mark.parametrize("pad", ["none", "hold"])
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("W,A,G", GEOMS)
def test_every_window_once_and_padding_only_at_the_end(W, A, G, stride, pad):
    eps = R.make_store(W, A, G, seed=W)
    lengths = [e[0].shape[0] for e in eps]
    begin = np.concatenate([[0], np.cumsum(lengths)])
    starts = V.sweep_table(lengths, W, stride, pad)
    n_total = int(starts[-1])
    B = 3 if n_total % 3 else 4
    assert n_total % B, "the case needs a partial last batch"
    nb = V.num_batches(n_total, B)
    seen, firsts = [], set()
    for i in range(nb):
        b = V.sweep_windows(eps, W, B, i, stride, pad)
        live = b["valid"] == 1
        assert live.all() if i < nb - 1 else (live.sum() == n_total - i * B and not live[-1])      # invalid rows exist in the last batch only
        assert np.array_equal(np.sort(np.unique(b["valid"])), [0, 1] if i == nb - 1 else [1])
        assert (b["action_mask"][~live] == 0).all() and (b["window"][~live] == n_total - 1).all()
        seen += list(b["window"][live])
        for j in np.nonzero(live)[0]:
            e, idx = int(b["episode"][j]), int(b["index"][j])
            assert begin[e] <= idx < begin[e + 1] and (idx - begin[e]) % stride == 0
            assert b["action_mask"][j].sum() == min(W, begin[e + 1] - idx) and (pad == "hold" or b["action_mask"][j].all())
            assert np.array_equal(b["actions"][j, 0], eps[e][0][idx - begin[e]]) and np.array_equal(b["latent_goal"][j], eps[e][1])
            firsts.add(idx)
    assert seen == list(range(n_total))                                          # each window number once and only once, in order
    assert len(firsts) == n_total                                                # and they are different windows
    if pad == "hold" and stride == 1:
        assert firsts == set(range(int(begin[-1])))                              # every step starts exactly one window


def test_an_episode_subset_never_yields_another_episode():
    W, A, G, B = 4, 3, 5, 3
    eps = R.make_store(W, A, G, seed=1)
    lengths = [e[0].shape[0] for e in eps]
    for ids in ([3], [0, 2], [1, 3]):
        starts = V.sweep_table(lengths, W, 1, "hold", ids)
        assert int(starts[-1]) == sum(lengths[e] for e in ids)
        got = []
        for i in range(V.num_batches(int(starts[-1]), B)):
            got += list(V.sweep_windows(eps, W, B, i, 1, "hold", episodes=ids)["episode"])
        assert set(got) == set(ids)
    lo, hi, scale = R.minmax(eps)
    b = V.sweep_windows(eps, W, 5, 0, 1, "hold", norm=(lo, scale), episodes=[2])
    assert b["actions"].min() >= -1 and b["actions"].max() <= 1 and (b["episode"] == 2).all()


def test_noise_seeds_belong_to_the_window():
    assert V.window_noise_seeds(7, [0, 1, 5]) == [R.noise_seeds(7, 6)[j] for j in (0, 1, 5)]


def _case(B, W, A, seed):
    rng = np.random.default_rng(seed)
    pred, target = rng.standard_normal((B, W, A)).astype(np.float32), rng.standard_normal((B, W, A)).astype(np.float32)
    mask = (rng.random((B, W)) < 0.7).astype(np.float32) * rng.random((B, W)).astype(np.float32)
    weight = rng.random(B).astype(np.float32)
    unit = rng.random(A) * 3 + 0.1
    return pred, target, mask, weight, unit


@pytest.mark.parametrize("B,W,A", [(1, 1, 1), (3, 4, 3), (64, 10, 7), (65, 10, 7), (130, 2, 5), (300, 10, 7)])
def test_ordered_action_error_agrees_with_a_plain_fp64_sum(B, W, A):
    pred, target, mask, weight, unit = _case(B, W, A, B + W)
    for kw in (dict(), dict(mask=mask), dict(weight=weight), dict(mask=mask, weight=weight, unit=unit)):
        got, want = V.action_error(pred, target, **kw), V.action_error_plain(pred, target, **kw)
        for g, w_, name in zip(got, want, ("sq", "ab", "cnt")):
            assert np.all(np.abs(g - w_) <= 1e-12 * np.abs(w_)), (kw.keys(), name)
    if B > 1:
        assert np.array_equal(V.action_error(pred, target)[2], np.full(W, float(B)))
    # two calls accumulate: the second call's sums are added to the first's
    first = V.action_error(pred, target, mask=mask)
    both = V.action_error(target, pred, weight=weight, into=first)
    for b_, f_, s_ in zip(both, first, V.action_error(target, pred, weight=weight)):
        assert np.array_equal(b_, f_ + s_)


def test_action_error_ignores_what_is_masked_out():
    B, W, A = 70, 4, 3
    pred, target, mask, weight, unit = _case(B, W, A, 5)
    mask[::3] = [0.0, -1.0, np.nan, 1.0]                                         # zero, negative and NaN all count as 0
    weight[1::5] = np.nan
    weight[2::7] = -2.0
    ref = V.action_error(pred, target, mask=mask, weight=weight, unit=unit)
    dirty = pred.copy()
    c = V._terms(pred, target, mask, weight, None)[0]
    dirty[c == 0] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(int((c == 0).sum())) % 3][:, None]
    assert (c == 0).sum() > B and not np.isfinite(dirty).all()
    got = V.action_error(dirty, target, mask=mask, weight=weight, unit=unit)
    for g, r in zip(got, ref):
        assert np.isfinite(g).all() and np.array_equal(g, r)
    for g, r in zip(V.action_error_plain(dirty, target, mask=mask, weight=weight, unit=unit), ref):
        assert np.isfinite(g).all() and np.all(np.abs(g - r) <= 1e-12 * np.abs(r))
    zero = V.action_error(dirty, target, mask=np.zeros((B, W), np.float32))
    assert all((z == 0).all() for z in zero)
    u0 = unit.copy(); u0[1] = 0.0                                                # a zero unit: that dimension contributes no error
    sq = V.action_error(pred, target, unit=u0)[0].reshape(W, A)
    assert (sq[:, 1] == 0).all() and (sq[:, 0] > 0).all()


def _store(W=4, A=3, G=5, n_extra=0):
    st = data.EpisodeStore(A, G, device="cpu")
    eps = R.make_store(W, A, G, seed=2)
    for e in eps:
        st.add_episode(e[0], e[1])
    for k in range(n_extra):
        st.add_episode(np.full((W + k, A), float(k), np.float32), np.zeros(G, np.float32))
    return st


def test_split_episodes_is_deterministic_disjoint_and_covering():
    st = _store(n_extra=6)                                                       # 10 episodes
    E = st.num_episodes
    for kw in (dict(val_fraction=0.3), dict(val_fraction=0.01), dict(val_fraction=0.5, seed=4), dict(val_episodes=[7, 2])):
        tr, va = data.split_episodes(st, **kw)
        tr2, va2 = data.split_episodes(st, **kw)
        assert np.array_equal(tr, tr2) and np.array_equal(va, va2)
        assert tr.dtype == va.dtype == np.int64 and list(tr) == sorted(tr) and list(va) == sorted(va)
        assert not set(tr) & set(va) and sorted(list(tr) + list(va)) == list(range(E))
    assert len(data.split_episodes(st, val_fraction=0.3)[1]) == 3 and len(data.split_episodes(st, val_fraction=0.01)[1]) == 1
    assert list(data.split_episodes(st, val_fraction=0.3, seed=5)[1]) == sorted(np.random.default_rng(5).permutation(E)[:3])
    assert list(data.split_episodes(st, val_episodes=[7, 2])[1]) == [2, 7]
    assert any(not np.array_equal(data.split_episodes(st, val_fraction=0.3, seed=s)[1], data.split_episodes(st, val_fraction=0.3)[1]) for s in (1, 2, 3))
    assert np.array_equal(data.split_episodes(st.finalize(None), val_fraction=0.3)[1], data.split_episodes(st, val_fraction=0.3)[1])
    for kw in (dict(), dict(val_fraction=0.2, val_episodes=[1]), dict(val_fraction=0.0), dict(val_fraction=1.0), dict(val_fraction=-0.5),
               dict(val_fraction=float("nan")), dict(val_episodes=[E]), dict(val_episodes=[-1]), dict(val_episodes=[1, 1]), dict(val_episodes=[]),
               dict(val_episodes=list(range(E))), dict(val_episodes=[0.5])):
        with pytest.raises(ValueError):
            data.split_episodes(st, **kw)


def test_episode_selection_builds_the_tables_of_the_reference():
    W = 4
    st = _store(W).finalize()
    lengths = list(st.lengths)
    assert lengths == R.episode_lengths(W)
    full = data.WindowStream(st, 5, W)
    assert np.array_equal(full.starts.numpy(), R.start_table(lengths, W, "hold")) and full.n_total == sum(lengths)
    assert np.array_equal(data.WindowStream(st, 5, W, episodes=np.arange(4)).starts.numpy(), full.starts.numpy())     # every episode: today's table
    for ids in ([3], [0, 2], np.array([1, 3])):
        for pad in ("hold", "none"):
            if pad == "none" and not any(lengths[e] >= W for e in ids):
                continue
            s = data.WindowStream(st, 5, W, pad=pad, episodes=ids)
            assert np.array_equal(s.starts.numpy(), V.sweep_table(lengths, W, 1, pad, ids)) and s.n_total == int(s.starts[-1])
            for stride in (1, 3):
                sw = data.WindowSweep(st, 5, W, stride=stride, pad=pad, episodes=ids)
                assert np.array_equal(sw.starts.numpy(), V.sweep_table(lengths, W, stride, pad, ids))
                assert len(sw) == V.num_batches(sw.n_total, 5)
    assert len(data.WindowSweep(st, 16, W)) == 1 and len(data.WindowSweep(st, 5, W)) == -(-sum(lengths) // 5)
    for make in (data.WindowStream, data.WindowSweep):
        for kw in (dict(pad="none", episodes=[0, 1]), dict(episodes=[]), dict(episodes=[4]), dict(episodes=[1, 1]), dict(episodes=[-1])):
            with pytest.raises(ValueError):                                      # nothing left to draw; unknown or repeated ids
                make(st, 5, W, **kw)
    for kw in (dict(stride=0), dict(stride=-1), dict(stride=1.5), dict(batch_size=0), dict(window=1366)):
        with pytest.raises(ValueError):
            data.WindowSweep(st, **{**dict(batch_size=5, window=W), **kw})
    sw = data.WindowSweep(st, 5, W)
    for bad in (-1, len(sw), 1.0):
        with pytest.raises(ValueError):
            sw.batch(bad)
