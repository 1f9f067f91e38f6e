"""GPU: mode_data_sweep_windows (through ctypes and through data.WindowSweep) against the numpy restatement of include/mode_hip.h
(tests/val_refs.py), bit for bit, every output between canary rows; the row belongs to its window whatever the batch size; and
data.WindowStream(episodes=) on the kernel the training stream already has."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import data_refs as R  # noqa: E402
import hip_helpers as H  # noqa: E402
import val_refs as V  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd import camera, data, rollout  # noqa: E402

BAD_ARG, UNSUPPORTED = -1, -2
KEYS = ("actions", "action_mask", "latent_goal", "index", "episode", "valid", "window", "noise")


def py_store(eps, normalize, cams=False):
    st = data.EpisodeStore(eps[0][0].shape[1], eps[0][1].shape[0])
    for e in eps:
        st.add_episode(*(e if cams else e[:2]))
    return st.finalize(normalize)


class Outs:
    """Guarded outputs of one launch (the int32 tables as raw canary-framed buffers)."""

    def __init__(self, B, W, A, G):
        self.actions, self.mask, self.goal, self.noise, self.valid = H.Guarded(B, W * A), H.Guarded(B, W), H.Guarded(B, G), H.Guarded(B, W * A), H.Guarded(B, 1)
        self.index, self.episode, self.window = (torch.full((B + 8,), -77, dtype=torch.int32, device="cuda") for _ in range(3))

    def ints(self, t):
        return t[4:-4]

    def intact(self):
        ok = all(g.intact() for g in (self.actions, self.mask, self.goal, self.noise, self.valid))
        return ok and all(bool((t[:4] == -77).all()) and bool((t[-4:] == -77).all()) for t in (self.index, self.episode, self.window))

    def untouched(self):
        return self.intact() and all(bool(torch.isnan(g.t).all()) for g in (self.actions, self.mask, self.goal, self.noise, self.valid)) and \
            all(bool((t == -77).all()) for t in (self.index, self.episode, self.window))

    def batch(self):
        return dict(actions=self.actions.t, action_mask=self.mask.t, latent_goal=self.goal.t, noise=self.noise.t, valid=self.valid.t.reshape(-1),
                    index=self.ints(self.index), episode=self.ints(self.episode), window=self.ints(self.window))


def desc(t, o, W, B, starts, n_total, stride=1, first=0, seed=0, draw=0, noise_scale=1.0, over=None):
    A, G = t["actions"].shape[1], t["goals"].shape[1]
    d = L.ModeDataSweepDesc(actions=H.p(t["actions"]), ep_begin=H.p(t["ep_begin"]), starts=H.p(starts), goals=H.p(t["goals"]), lo=H.p(t["lo"]),
                            scale=H.p(t["scale"]), S=t["actions"].shape[0], E=t["goals"].shape[0], A=A, G=G, W=W, B=B, n_total=n_total, stride=stride,
                            first=first, seed=seed, draw=draw, noise_scale=noise_scale, out_actions=H.p(o.actions.t), action_mask=H.p(o.mask.t),
                            latent_goal=H.p(o.goal.t), index=o.ints(o.index).data_ptr(), episode=o.ints(o.episode).data_ptr(), valid=H.p(o.valid.t),
                            window=o.ints(o.window).data_ptr(), noise=H.p(o.noise.t))
    for k, v in (over or {}).items():
        setattr(d, k, v)
    return d


def check_batch(got, ref, W, A, seed, draw, noise_scale, what):
    B = ref["index"].shape[0]
    for k in ("index", "episode", "window", "valid", "action_mask", "latent_goal"):
        assert np.array_equal(got[k].cpu().numpy().reshape(ref[k].shape), ref[k]), (what, k)
    a = got["actions"].cpu().numpy().reshape(B, W, A)
    assert np.array_equal(a.view(np.uint32), ref["actions"].view(np.uint32)), (what, "actions", float(np.abs(a - ref["actions"]).max()))
    z = rollout.env_noise(V.window_noise_seeds(seed, ref["window"]), [draw] * B, W, A, noise_scale, "cuda")
    assert torch.equal(got["noise"].reshape(B, W, A), z), (what, "noise")


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("pad", ["none", "hold"])
@pytest.mark.parametrize("W,A,G", [(4, 3, 5), (10, 7, 512)])
def test_sweep_matches_the_reference_bit_for_bit(W, A, G, pad, stride, norm):
    eps = R.make_store(W, A, G, seed=W)
    lo, hi, scale = R.minmax(eps)
    nrm = (lo, scale) if norm else None
    t = H.dev_store(eps, nrm)
    starts_h = V.sweep_table(t["lengths"], W, stride, pad)
    n_total = int(starts_h[-1])
    starts = torch.from_numpy(starts_h.astype(np.int32)).cuda()
    B = next(b for b in (7, 5, 4, 3, 2) if n_total % b)                          # a batch size that does not divide n_total
    seed, draw, ns = 11, 2, 80.0
    sw = data.WindowSweep(py_store(eps, "minmax" if norm else None), B, W, stride=stride, pad=pad, seed=seed)
    assert sw.n_total == n_total and len(sw) == V.num_batches(n_total, B)
    padded = 0
    for i in range(len(sw)):
        ref = V.sweep_windows(eps, W, B, i, stride, pad, nrm)
        padded += int((ref["action_mask"][ref["valid"] == 1] == 0).sum())
        o = Outs(B, W, A, G)
        L.check(L.load().mode_data_sweep_windows(C.byref(desc(t, o, W, B, starts, n_total, stride, i * B, seed, draw, ns)), H.stream()))
        torch.cuda.synchronize()
        assert o.intact()
        check_batch(o.batch(), ref, W, A, seed, draw, ns, f"ctypes batch {i}")
        b = sw.batch(i, draw, noise_scale=ns)
        assert sorted(b) == sorted(KEYS) and b["actions"].shape == (B, W, A) and b["valid"].shape == (B,) and b["window"].dtype == torch.int32
        check_batch(b, ref, W, A, seed, draw, ns, f"data.py batch {i}")
    assert ref["valid"][-1] == 0 and (padded > 0) == (pad == "hold")
    check_batch(sw.batch(0), V.sweep_windows(eps, W, B, 0, stride, pad, nrm), W, A, seed, 0, 1.0, "defaults")      # draw 0, unit noise


def _sweep_rows(sw, draw=0):
    """A whole sweep, concatenated and cut to its valid rows."""
    bs = [sw.batch(i, draw) for i in range(len(sw))]
    keep = torch.cat([b["valid"] for b in bs]) == 1
    return {k: torch.cat([b[k] for b in bs])[keep] for k in KEYS}


def test_a_row_belongs_to_its_window_not_to_its_batch():
    W, A, G = 10, 7, 512
    st = py_store(R.make_store(W, A, G, seed=3), "minmax")                       # 33 windows
    small, big = data.WindowSweep(st, 5, W, seed=2), data.WindowSweep(st, 16, W, seed=2)
    assert (len(small), len(big)) == (7, 3)
    a, b = _sweep_rows(small), _sweep_rows(big)
    for k in KEYS:
        assert a[k].shape[0] == 33 and torch.equal(a[k], b[k]), k
    assert torch.equal(a["window"], torch.arange(33, dtype=torch.int32, device="cuda"))
    # draw: other noise, nothing else; another seed: other noise too
    c, other = _sweep_rows(small, draw=1), _sweep_rows(data.WindowSweep(st, 5, W, seed=3))
    for k in KEYS:
        assert torch.equal(a[k], c[k]) == (k != "noise") and torch.equal(a[k], other[k]) == (k != "noise"), k
    assert abs(float(c["noise"].std()) - 1.0) < 0.1
    # two windows of one batch do not share their noise, and a batch is stateless: asked for again, the same bits
    assert not torch.equal(a["noise"][0], a["noise"][1])
    assert all(torch.equal(v, w) for v, w in zip(small.batch(3, 1).values(), small.batch(3, 1).values()))


def test_stream_with_an_episode_subset():
    W, A, G, B = 10, 7, 512, 37
    st = py_store(R.make_store(W, A, G, seed=5), "minmax")
    full, listed = data.WindowStream(st, B, W, seed=4), data.WindowStream(st, B, W, seed=4, episodes=[0, 1, 2, 3])
    for step in (0, 9):
        x, y = full.batch(step), listed.batch(step)
        assert all(torch.equal(x[k], y[k]) for k in ("actions", "action_mask", "latent_goal", "index", "episode", "noise", "u"))
    for ids in ([1, 3], [2], [0]):
        s = data.WindowStream(st, B, W, seed=4, episodes=ids)
        seen = torch.cat([s.batch(step)["episode"] for step in range(64)]).cpu().numpy()
        assert set(seen) == set(ids), (ids, set(seen))
    begin = st.ep_begin.cpu().numpy()
    b = data.WindowStream(st, B, W, seed=4, episodes=[1, 3]).batch(2)
    idx, ep = b["index"].cpu().numpy(), b["episode"].cpu().numpy()
    assert ((begin[ep] <= idx) & (idx < begin[ep + 1])).all()
    assert torch.equal(b["latent_goal"], st.goals[b["episode"].long()])


def test_frames_come_out_of_the_store_without_a_shift():
    W, A, G, B = 4, 3, 5, 4                                                      # 2 + 4 windows: two batches, two padding rows
    eps = R.make_store(W, A, G, seed=9, cams=((12, 10), (9, 9)))
    st = py_store(eps, "minmax", cams=True)
    tr = (camera.CameraTransform((8, 8), shift_pad=2), camera.CameraTransform((8, 8)))          # a shift pad is not used by a sweep
    sw = data.WindowSweep(st, B, W, stride=2, episodes=[1, 3], camera_transforms=tr, frame_dtype=torch.bfloat16)
    for i in range(len(sw)):
        b = sw.batch(i)
        ref = V.sweep_windows(eps, W, B, i, 2, "hold", R.minmax(eps)[::2], episodes=[1, 3])
        assert np.array_equal(b["index"].cpu().numpy(), ref["index"]) and "shifts" not in b
        idx = torch.from_numpy(ref["index"].astype(np.int64)).cuda()
        want = camera.preprocess_cameras(st.frames_static[idx], st.frames_gripper[idx], tr[0], tr[1], shifts=(None, None), dtype=torch.bfloat16)
        assert b["rgb_obs"]["rgb_static"].shape == (B, 3, 8, 8) and b["rgb_obs"]["rgb_static"].dtype == torch.bfloat16
        assert torch.equal(b["rgb_obs"]["rgb_static"], want[0]) and torch.equal(b["rgb_obs"]["rgb_gripper"], want[1])
    assert ref["valid"][-1] == 0
    with pytest.raises(ValueError, match="holds no frames"):
        data.WindowSweep(py_store(eps, None), B, W, camera_transforms=tr)


def test_bad_descriptors_are_refused_before_any_launch():
    W, A, G, B = 4, 3, 5, 7
    eps = R.make_store(W, A, G)
    lo, hi, scale = R.minmax(eps)
    t = H.dev_store(eps, (lo, scale))
    starts_h = V.sweep_table(t["lengths"], W, 1, "hold")
    n_total = int(starts_h[-1])
    starts = torch.from_numpy(starts_h.astype(np.int32)).cuda()
    lib = L.load()
    o = Outs(B, W, A, G)
    good = lambda **over: desc(t, o, W, B, starts, n_total, over=over)
    assert lib.mode_data_sweep_windows(None, H.stream()) == BAD_ARG
    cases = [(dict(**{k: None}), BAD_ARG) for k in ("actions", "ep_begin", "starts", "goals", "out_actions", "action_mask", "latent_goal", "index", "episode",
                                                    "valid", "window")]
    cases += [(dict(lo=None), BAD_ARG), (dict(scale=None), BAD_ARG)]
    cases += [(dict(**{k: v}), BAD_ARG) for k in ("S", "E", "A", "G", "W", "B", "n_total") for v in (0, -1)]
    cases += [(dict(n_total=16), BAD_ARG), (dict(E=16), BAD_ARG)]                 # more windows / episodes than steps
    cases += [(dict(stride=0), BAD_ARG), (dict(stride=-3), BAD_ARG), (dict(first=-1), BAD_ARG), (dict(first=n_total), BAD_ARG), (dict(first=2 ** 31 - 1), BAD_ARG)]
    cases += [(dict(B=65536), UNSUPPORTED), (dict(W=1366), UNSUPPORTED), (dict(G=4097), UNSUPPORTED)]
    for over, want in cases:
        assert lib.mode_data_sweep_windows(C.byref(good(**over)), H.stream()) == want, over
    torch.cuda.synchronize()
    assert o.untouched()
    assert lib.mode_data_sweep_windows(C.byref(good(first=n_total - 1, noise=None)), H.stream()) == 0      # the last window alone; noise is optional
    torch.cuda.synchronize()
    assert o.intact() and bool(torch.isnan(o.noise.t).all()) and not bool(torch.isnan(o.actions.t).any())
    assert o.valid.t.reshape(-1).tolist() == [1.0] + [0.0] * (B - 1) and o.ints(o.window).tolist() == [n_total - 1] * B
    assert float(o.mask.t[1:].abs().sum()) == 0.0 and float(o.mask.t[0, 0]) == 1.0
