"""GPU: mode_data_sample_windows_ordered through data.WindowStream(order="epoch") / (episode_weights=) against the numpy restatement of
include/mode_hip.h (tests/order_refs.py).  Everything the ordered locate adds is an integer draw; the rows behind it are the copies and the three
unfused roundings of mode_data_sample_windows: every comparison is bit equality."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import data_refs as R  # noqa: E402
import goal_refs as GR  # noqa: E402
import hip_helpers as H  # noqa: E402
import order_refs as O  # noqa: E402
import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd import camera, data, rollout  # noqa: E402

BAD_ARG = -1
W = 4
LAST_STEP = 2 ** 32 - 1
CAMS = ((8, 8), (6, 6))


def _episodes(lengths, A, G, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((n, A)).astype(np.float32), rng.standard_normal(G).astype(np.float32), None, None) for n in lengths]


def _host_cases():
    """name -> (host episodes, pad, n): the issue's stores.  "fifteen" / "five" are data_refs.make_store at W = 4, A = 3, G = 8 (lengths 1, 3, 4,
    7) with both cameras; "long" one episode of 4097 steps (h = 7, long walks), "sixteen" n = 2^bits (no walk), "one" a single window."""
    small = R.make_store(W, 3, 8, seed=2, cams=CAMS)
    return {"fifteen": (small, "hold", 15), "five": (small, "none", 5), "long": (_episodes([4097], 2, 4, 5), "hold", 4097),
            "sixteen": (_episodes([5, 11], 3, 8, 6), "hold", 16), "one": (_episodes([1], 3, 8, 7), "hold", 1)}


HOST = _host_cases()
_STORES = {}


def store_of(name):
    """(EpisodeStore on the device, (lo, scale) of its normalisation) - built once per module."""
    if name not in _STORES:
        eps = HOST[name][0]
        st = data.EpisodeStore(eps[0][0].shape[1], eps[0][1].shape[0])
        for e in eps:
            st.add_episode(*e)
        st.finalize("minmax")
        lo, hi, scale = R.minmax(eps)
        _STORES[name] = (st, (lo, scale))
    return _STORES[name]


def batch_sizes(n):
    return (4, 7, 64) if n >= 64 else (4, 7)


def straddle_step(n, B):
    """The first step whose rows lie in two epochs; where B divides n, the first step of epoch 1."""
    t = 0
    while (t * B + B - 1) // n == 0:
        t += 1
    return t


def check_batch(got, ref, seed, step, what, shifts=False):
    B, Wn, A = ref["actions"].shape
    for k in ("index", "episode", "action_mask", "actions", "latent_goal", "u"):
        assert R.same_bits(got[k].cpu().numpy(), ref[k]), (what, k)
    for k in ("epoch", "position"):
        if k in ref:
            assert got[k].dtype == torch.int64 and R.same_bits(got[k].cpu().numpy(), ref[k]), (what, k)
        else:
            assert k not in got, (what, k)
    z = rollout.env_noise(R.noise_seeds(seed, B), [step] * B, Wn, A, 1.0, "cuda")
    assert torch.equal(got["noise"], z), (what, "noise")
    if shifts:
        for q, name in enumerate(("rgb_static", "rgb_gripper")):
            assert R.same_bits(got["shifts"][name].cpu().numpy(), ref["shifts"][q]), (what, "shifts", name)


def all_starts(st, stream):
    """Every store row that starts a window of `stream`, ascending."""
    begin, n_e = st.ep_begin.cpu().numpy().astype(np.int64), np.diff(stream.starts.cpu().numpy().astype(np.int64))
    return np.concatenate([begin[e] + np.arange(n_e[e]) for e in range(len(n_e))])


# ---------------------------------------------------------------------------------------------------------------- 1. epoch order, bit for bit
@pytest.mark.parametrize("name", list(HOST))
def test_epoch_order_matches_the_reference_bit_for_bit(name):
    eps, pad, n = HOST[name]
    st, norm = store_of(name)
    cams = eps[0][2] is not None
    tr = (camera.CameraTransform((8, 8), shift_pad=2), camera.CameraTransform((8, 8), shift_pad=3)) if cams else None
    seed = 11
    straddled = 0
    for B in batch_sizes(n):
        stream = data.WindowStream(st, B, W, seed=seed, pad=pad, order="epoch", camera_transforms=tr)
        assert stream.n_total == n
        for step in (0, 1, straddle_step(n, B), LAST_STEP):
            ref = O.sample_windows_ordered(eps, W, B, seed, step, pad, norm, shift_pads=(2, 3) if cams else (0, 0), order="epoch")
            got = stream.batch(step)
            check_batch(got, ref, seed, step, f"{name} B={B} step={step}", shifts=cams)
            straddled += len(set(ref["epoch"].tolist())) > 1
            assert stream.epoch_of(step) == int(ref["epoch"][0])
            if step == LAST_STEP:
                assert int(ref["epoch"][0]) == (LAST_STEP * B) // n and (n > 1 or int(ref["epoch"][0]) >= 2 ** 32)       # 64-bit P; ep_hi != 0 at n = 1
    assert straddled > 0 or n == 16


# ---------------------------------------------------------------------------------------------------------------- 2. exactly once per epoch
@pytest.mark.parametrize("name", ["fifteen", "five", "sixteen", "long"])
def test_an_epoch_visits_every_window_exactly_once(name):
    """The test that needs the feature: i.i.d. draws repeat windows (one pass of n draws misses about 37 % of them)."""
    eps, pad, n = HOST[name]
    st, _ = store_of(name)
    for B in batch_sizes(n):
        stream = data.WindowStream(st, B, W, seed=3, pad=pad, order="epoch", noise=False)
        want = all_starts(st, stream)
        assert len(want) == n
        for ep in (0, 1, 5):
            steps = range((ep * n) // B, ((ep + 1) * n - 1) // B + 1)                           # the steps that cover positions [ep n, (ep + 1) n)
            bs = [stream.batch(t) for t in steps]
            index, epoch, pos = (torch.cat([b[k] for b in bs]).cpu().numpy() for k in ("index", "epoch", "position"))
            rows = epoch == ep
            assert rows.sum() == n and np.array_equal(pos[rows], np.arange(n)), (name, B, ep)
            assert np.array_equal(np.sort(index[rows]), want), (name, B, ep)                      # every start, each once
            assert set(epoch[~rows].tolist()) <= {ep - 1, ep + 1}
        if n > 1:
            first = [tuple(torch.cat([stream.batch(t)["index"] for t in range((e * n) // B, ((e + 1) * n - 1) // B + 1)]).tolist()) for e in (0, 1)]
            assert first[0] != first[1]                                                          # another epoch, another order


# ---------------------------------------------------------------------------------------------------------------- 3. resume
@pytest.mark.parametrize("mode", ["epoch", "weights"])
def test_a_resumed_stream_returns_the_same_bits(mode):
    st, _ = store_of("fifteen")
    kw = dict(order="epoch") if mode == "epoch" else dict(episode_weights=(0.5, 1, 2, 3))
    s = data.WindowStream(st, 7, W, seed=2, **kw)
    b5 = s.batch(5)
    for t in (9, 0, LAST_STEP, 6):
        s.batch(t)
    again, fresh, other = s.batch(5), data.WindowStream(st, 7, W, seed=2, **kw).batch(5), s.batch(6)
    assert set(b5) == set(again) == set(fresh)
    for k in b5:
        assert torch.equal(b5[k], again[k]) and torch.equal(b5[k], fresh[k]), k
    assert not torch.equal(b5["noise"], other["noise"]) and not torch.equal(b5["index"], data.WindowStream(st, 7, W, seed=3, **kw).batch(5)["index"])


# ---------------------------------------------------------------------------------------------------------------- 4. weighted mixtures
WEIGHTED = [((0, 1, 0, 3), "hold", None),                     # zeros at the front and in the middle
            ((2, 1, 3, 0), "hold", None),                     # a trailing zero
            ((1, 1, 1, 5), "hold", [0, 1, 2]),                # episodes= leaves out an episode of positive weight
            ((0, 0.25, 0, 1e-3), "hold", [1, 3]),
            ((1, 1, 1, 1), "none", None)]                     # pad="none": episodes 0 and 1 have no start, whatever their weight


@pytest.mark.parametrize("w,pad,episodes", WEIGHTED)
def test_episode_weights_match_the_reference_bit_for_bit(w, pad, episodes):
    eps = HOST["fifteen"][0]
    st, norm = store_of("fifteen")
    seed = 11
    n_e = O.start_counts(R.episode_lengths(W), W, pad, episodes)
    live = {e for e in range(4) if w[e] > 0 and n_e[e] > 0}
    for B in (4, 7, 64):
        stream = data.WindowStream(st, B, W, seed=seed, pad=pad, episodes=episodes, episode_weights=w)
        for step in (0, 5, LAST_STEP):
            ref = O.sample_windows_ordered(eps, W, B, seed, step, pad, norm, episode_weights=w, episodes=episodes)
            check_batch(stream.batch(step), ref, seed, step, f"w={w} pad={pad} episodes={episodes} B={B} step={step}")
    stream = data.WindowStream(st, 64, W, seed=seed, pad=pad, episodes=episodes, episode_weights=w, noise=False)
    bs = [stream.batch(t) for t in range(200)]
    episode, index = (torch.cat([b[k] for b in bs]).cpu().numpy() for k in ("episode", "index"))
    assert set(episode.tolist()) == live                                                         # no episode without mass, in 12800 draws
    begin = np.concatenate([[0], np.cumsum(R.episode_lengths(W))])
    assert set(index.tolist()) <= {int(begin[e]) + p for e in live for p in range(n_e[e])}       # and only starts of the others
    share = np.array([w[e] if e in live else 0.0 for e in range(4)]) / sum(w[e] for e in live)
    count = np.bincount(episode, minlength=4)
    assert (np.abs(count - 12800 * share) <= 5 * np.sqrt(12800 * share * (1 - share)) + 1e-9).all(), (count, share)


# ---------------------------------------------------------------------------------------------------------------- 5. the default is unchanged
@pytest.mark.parametrize("name", ["fifteen", "five", "long"])
def test_default_stream_is_unchanged(name):
    eps, pad, n = HOST[name]
    st, norm = store_of(name)
    for B in batch_sizes(n):
        for step in (0, 5, LAST_STEP):
            ref = R.sample_windows(eps, W, B, 11, step, pad, norm)
            for kw in ({}, dict(order="iid", episode_weights=None)):
                got = data.WindowStream(st, B, W, seed=11, pad=pad, **kw).batch(step)
                assert set(got) == {"actions", "action_mask", "latent_goal", "index", "episode", "noise", "u"}
                check_batch(got, ref, 11, step, f"{name} B={B} step={step} {kw}")


# ---------------------------------------------------------------------------------------------------------------- 6. composition
def test_epoch_order_composes_with_hindsight_goals():
    eps = HOST["fifteen"][0]
    sg = GR.step_goal_table(eps, 8)
    st = data.EpisodeStore(3, 8)
    for e, s in zip(eps, sg):
        st.add_episode(e[0], e[1], step_goals=s)
    st.finalize("minmax")
    lo, hi, scale = R.minmax(eps)
    begin = np.concatenate([[0], np.cumsum(R.episode_lengths(W))])
    seed, B = 7, 7
    stream = data.WindowStream(st, B, W, seed=seed, order="epoch", goal="hindsight", goal_horizon=(0, 3), hindsight_prob=0.5)
    kinds = set()
    for step in (0, 2, LAST_STEP):
        b = stream.batch(step)
        base = O.sample_windows_ordered(eps, W, B, seed, step, "hold", (lo, scale), order="epoch")
        check_batch({k: v for k, v in b.items() if k != "latent_goal"} | {"latent_goal": torch.from_numpy(base["latent_goal"])}, base, seed, step, f"step={step}")
        ref = GR.relabel(begin, base["index"], base["episode"], seed, step, 0, 3, 2 ** 31)
        for k in ("goal_index", "goal_offset", "goal_kind"):
            assert R.same_bits(b[k].cpu().numpy(), ref[k]), (step, k)
        assert R.same_bits(b["latent_goal"].cpu().numpy(), GR.relabelled_goals(base["latent_goal"], np.concatenate(sg), ref)), step
        kinds |= set(ref["goal_kind"].tolist())
    assert kinds == {0.0, 1.0}


def test_epoch_order_composes_with_cameras():
    """rgb_obs of an epoch-ordered row is what order="iid" returns for a row of the same index (transforms without a shift: a row's frames then
    depend on its index alone), and, with shifts, the transform of the hand-gathered frames under the stream's own shift tables."""
    st, _ = store_of("fifteen")
    B, seed = 7, 4
    plain = (camera.CameraTransform((8, 8)), camera.CameraTransform((8, 8)))
    draws = [data.WindowStream(st, 64, W, seed=seed, camera_transforms=plain, noise=False).batch(t) for t in range(4)]
    iid = {"index": torch.cat([b["index"] for b in draws]), "rgb_obs": {k: torch.cat([b["rgb_obs"][k] for b in draws]) for k in ("rgb_static", "rgb_gripper")}}
    row_of = {int(i): j for j, i in enumerate(iid["index"].tolist())}
    assert len(row_of) == 15                                                                      # 256 i.i.d. draws see all 15 starts
    ep = data.WindowStream(st, B, W, seed=seed, order="epoch", camera_transforms=plain, noise=False)
    for step in (0, 2):
        b = ep.batch(step)
        assert b["shifts"] == {"rgb_static": None, "rgb_gripper": None}
        rows = torch.tensor([row_of[int(i)] for i in b["index"].tolist()], device="cuda")
        for k in ("rgb_static", "rgb_gripper"):
            assert b["rgb_obs"][k].shape == (B, 3, 8, 8) and torch.equal(b["rgb_obs"][k], iid["rgb_obs"][k][rows]), (step, k)
    tr = (camera.CameraTransform((8, 8), shift_pad=2), camera.CameraTransform((8, 8), shift_pad=3))
    b = data.WindowStream(st, B, W, seed=seed, order="epoch", camera_transforms=tr).batch(2)
    same = data.WindowStream(st, B, W, seed=seed, camera_transforms=tr).batch(2)
    idx = b["index"].long()
    sh = (b["shifts"]["rgb_static"], b["shifts"]["rgb_gripper"])
    assert torch.equal(sh[0], same["shifts"]["rgb_static"]) and torch.equal(sh[1], same["shifts"]["rgb_gripper"])      # keyed by (seed, t, j) in every mode
    assert not torch.equal(b["index"], same["index"])
    want = camera.preprocess_cameras(st.frames_static[idx], st.frames_gripper[idx], tr[0], tr[1], shifts=sh)
    assert torch.equal(b["rgb_obs"]["rgb_static"], want[0]) and torch.equal(b["rgb_obs"]["rgb_gripper"], want[1])


def test_diffusion_loss_on_an_epoch_ordered_batch_is_finite():
    from oracle.weights import make_inputs
    from test_gpu_train import build_train
    cfg, sd, m = build_train("c1e4", 210, "bf16")
    den = M.GCDenoiser(m, 0.5).train()
    B, Wn, A = 8, 10, 7
    st = data.EpisodeStore(A, cfg.goal_dim)
    for e in R.make_store(Wn, A, cfg.goal_dim, seed=3):                                           # episodes of 1, 9, 10 and 13 steps: n = 33
        st.add_episode(e[0], e[1])
    st.finalize("minmax")
    b = data.WindowStream(st, B, Wn, seed=7, order="epoch").batch(4)                              # positions 32 .. 39: the batch straddles epochs 0 and 1
    assert b["epoch"].tolist() == [0] + [1] * 7
    img = make_inputs(cfg, B, 31)["state_images"].cuda()
    sig = M.utils.rand_log_logistic((B,), loc=float(np.log(0.5)), scale=0.5, min_value=1e-3, max_value=80.0, u=b["u"])
    loss = M.diffusion_loss(den, {"state_images": img}, b["latent_goal"], b["actions"], action_mask=b["action_mask"], noise=b["noise"], sigmas=sig)
    loss.backward()
    assert torch.isfinite(loss) and float(loss.detach()) > 0
    m.zero_grad(set_to_none=True)


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_bad_descriptors_and_arguments_are_refused_before_any_launch():
    """The constructor's ValueErrors (tests/test_order_references.py has them all, on a store without a device) on a device store, and the C entry
    point's own refusals with the outputs left untouched."""
    st, _ = store_of("fifteen")
    for kw in (dict(order="shuffle"), dict(episode_weights=(1, 1, 1)), dict(episode_weights=(1, -1, 1, 1)), dict(episode_weights=(0, 0, 0, 0)),
               dict(episode_weights=(1e-30, 1, 1, 1)), dict(order="epoch", episode_weights=(1, 1, 1, 1))):
        with pytest.raises(ValueError):
            data.WindowStream(st, 7, W, **kw)
    B, A, G = 7, 3, 8
    stream = data.WindowStream(st, B, W, order="epoch")
    f32 = lambda *s: torch.full(s, H.CANARY, dtype=torch.float32, device="cuda")
    outs = dict(out_actions=f32(B, W, A), action_mask=f32(B, W), latent_goal=f32(B, G), index=torch.full((B,), -77, dtype=torch.int32, device="cuda"),
                episode=torch.full((B,), -77, dtype=torch.int32, device="cuda"))
    i64 = [torch.full((B + 2,), -77, dtype=torch.int64, device="cuda") for _ in range(2)]
    cut = torch.tensor([0, 1, 2, 3, 2 ** 32], dtype=torch.int64, device="cuda")

    def good(mode=L.MODE_ORDER_EPOCH, **over):
        s = L.ModeDataStreamDesc(actions=H.p(st.actions), ep_begin=H.p(st.ep_begin), starts=H.p(stream.starts), goals=H.p(st.goals), lo=H.p(st.lo),
                                 scale=H.p(st.scale), S=15, E=4, A=A, G=G, W=W, B=B, n_total=15, seed=1, step=2, **{k: H.p(v) for k, v in outs.items()})
        o = L.ModeDataOrderDesc(s=s, mode=mode, cut=H.p(cut), epoch=i64[0][1:].data_ptr(), position=i64[1][1:].data_ptr())
        for k, v in over.items():
            setattr(o.s if hasattr(s, k) else o, k, v)                                            # (o.s shares o's memory)
        return o

    lib = L.load()
    assert lib.mode_data_sample_windows_ordered(None, H.stream()) == BAD_ARG
    cases = [dict(mode=0), dict(mode=3), dict(mode=-1), dict(epoch=None), dict(position=None), dict(mode=L.MODE_ORDER_WEIGHTED, cut=None),
             dict(starts=None), dict(index=None), dict(n_total=0), dict(n_total=16), dict(B=0), dict(E=0)]
    for over in cases:
        assert lib.mode_data_sample_windows_ordered(C.byref(good(**over)), H.stream()) == BAD_ARG, over
    assert lib.mode_data_sample_windows_ordered(C.byref(good(B=65536)), H.stream()) == -2
    torch.cuda.synchronize()
    assert all(bool((v == H.CANARY).all()) for k, v in outs.items() if v.dtype == torch.float32) and bool((outs["index"] == -77).all())
    assert all(bool((t == -77).all()) for t in i64)
    assert lib.mode_data_sample_windows_ordered(C.byref(good()), H.stream()) == 0                 # the descriptor these were derived from is a good one
    torch.cuda.synchronize()
    ref = O.epoch_rows(1, 2, B, 15)
    assert i64[0][1:-1].tolist() == ref[0].tolist() and i64[1][1:-1].tolist() == ref[1].tolist()
    assert all(int(t[0]) == -77 and int(t[-1]) == -77 for t in i64)                               # the elements around the int64 outputs stay
    assert lib.mode_data_sample_windows_ordered(C.byref(good(mode=L.MODE_ORDER_WEIGHTED, epoch=None, position=None)), H.stream()) == 0
    torch.cuda.synchronize()
    assert set(outs["episode"].tolist()) <= {3}                                                   # cut = (0, 1, 2, 3, 2^32): episode 3 but for r1 < 3
