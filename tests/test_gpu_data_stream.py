"""GPU: mode_data_sample_windows (through ctypes and through data.WindowStream) against the numpy restatement of include/mode_hip.h
(tests/data_refs.py).  Integers, masks, copied goals, normalised actions and the noise rows are compared bit for bit; every output lies between
canary rows (hip_helpers.Guarded)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import data_refs as R  # noqa: E402
import hip_helpers as H  # noqa: E402
from mode_diffusion_policy_amd import _lib as L  # noqa: E402
from mode_diffusion_policy_amd import camera, data, rollout  # noqa: E402

BAD_ARG, UNSUPPORTED = -1, -2
BATCHES = (1, 7, 64, 300)


class Outs:
    """Guarded outputs of one launch (int32 / fp64 tables as raw canary-framed buffers of their own dtype)."""

    def __init__(self, B, W, A, G, shifts=(False, False)):
        self.actions, self.mask, self.goal, self.noise = H.Guarded(B, W * A), H.Guarded(B, W), H.Guarded(B, G), H.Guarded(B, W * A)
        self.index, self.episode = self._ints(B), self._ints(B)
        self.u = torch.full((B + 4,), -7.0, dtype=torch.float64, device="cuda")
        self.shifts = [self._ints(2 * B) if s else None for s in shifts]

    @staticmethod
    def _ints(n):
        return torch.full((n + 8,), -77, dtype=torch.int32, device="cuda")

    def ints(self, t):
        return t[4:-4]

    def intact(self):
        ok = all(g.intact() for g in (self.actions, self.mask, self.goal, self.noise))
        for t in (self.index, self.episode, *[s for s in self.shifts if s is not None]):
            ok = ok and bool((t[:4] == -77).all()) and bool((t[-4:] == -77).all())
        return ok and bool((self.u[:2] == -7.0).all()) and bool((self.u[-2:] == -7.0).all())

    def untouched(self):
        return self.intact() and all(bool(torch.isnan(g.t).all()) for g in (self.actions, self.mask, self.goal, self.noise)) and \
            bool((self.index == -77).all()) and bool((self.episode == -77).all()) and bool((self.u == -7.0).all())


def desc(t, o, W, B, seed, step, starts, n_total, pads=(0, 0), **over):
    A, G = t["actions"].shape[1], t["goals"].shape[1]
    d = L.ModeDataStreamDesc(actions=H.p(t["actions"]), ep_begin=H.p(t["ep_begin"]), starts=H.p(starts), goals=H.p(t["goals"]), lo=H.p(t["lo"]),
                             scale=H.p(t["scale"]), S=t["actions"].shape[0], E=t["goals"].shape[0], A=A, G=G, W=W, B=B, n_total=n_total, seed=seed, step=step,
                             out_actions=H.p(o.actions.t), action_mask=H.p(o.mask.t), latent_goal=H.p(o.goal.t), index=o.ints(o.index).data_ptr(),
                             episode=o.ints(o.episode).data_ptr(), noise=H.p(o.noise.t), u=o.u[2:].data_ptr())
    for q in range(2):
        d.shifts[q] = None if o.shifts[q] is None else o.ints(o.shifts[q]).data_ptr()
        d.shift_pad[q] = pads[q]
    for k, v in over.items():
        setattr(d, k, v)
    return d


def check_batch(got, ref, W, A, seed, step, what):
    """got: dict of device tensors (either path); ref: data_refs.sample_windows."""
    B = ref["index"].shape[0]
    for k in ("index", "episode", "action_mask", "latent_goal"):
        assert np.array_equal(got[k].cpu().numpy().reshape(ref[k].shape), ref[k]), (what, k)
    a = got["actions"].cpu().numpy().reshape(B, W, A)
    assert np.array_equal(a.view(np.uint32), ref["actions"].view(np.uint32)), (what, "actions", float(np.abs(a - ref["actions"]).max()))
    assert np.array_equal(got["u"].cpu().numpy(), ref["u"]), (what, "u")
    z = rollout.env_noise(R.noise_seeds(seed, B), [step] * B, W, A, 1.0, "cuda")
    assert torch.equal(got["noise"].reshape(B, W, A), z), (what, "noise")


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("pad", ["none", "hold"])
@pytest.mark.parametrize("W,A,G", [(4, 3, 5), (10, 7, 512)])
def test_batches_match_the_reference_bit_for_bit(W, A, G, pad, norm):
    eps = R.make_store(W, A, G, seed=W)
    lo, hi, scale = R.minmax(eps)
    t = H.dev_store(eps, (lo, scale) if norm else None)
    starts_h = R.start_table(t["lengths"], W, pad)
    starts = torch.from_numpy(starts_h.astype(np.int32)).cuda()
    st = data.EpisodeStore(A, G)
    for e in eps:
        st.add_episode(e[0], e[1])
    st.finalize("minmax" if norm else None)
    seed, step = 11, 5
    padded = 0
    for B in BATCHES:
        ref = R.sample_windows(eps, W, B, seed, step, pad, (lo, scale) if norm else None)
        padded += int((ref["action_mask"] == 0).sum())
        o = Outs(B, W, A, G)
        L.check(L.load().mode_data_sample_windows(C.byref(desc(t, o, W, B, seed, step, starts, int(starts_h[-1]))), H.stream()))
        torch.cuda.synchronize()
        assert o.intact()
        check_batch(dict(index=o.ints(o.index), episode=o.ints(o.episode), action_mask=o.mask.t, latent_goal=o.goal.t, actions=o.actions.t,
                         u=o.u[2:-2], noise=o.noise.t), ref, W, A, seed, step, f"ctypes B={B}")
        b = data.WindowStream(st, B, W, seed=seed, pad=pad).batch(step)
        assert b["actions"].shape == (B, W, A) and b["action_mask"].shape == (B, W) and b["latent_goal"].shape == (B, G) and b["u"].dtype == torch.float64
        assert "rgb_obs" not in b
        check_batch(b, ref, W, A, seed, step, f"data.py B={B}")
    assert (padded > 0) == (pad == "hold")
    # noise=False: neither noise nor u is produced; optional outputs may be absent in the descriptor
    b = data.WindowStream(st, 7, W, seed=seed, pad=pad, noise=False).batch(step)
    assert "noise" not in b and "u" not in b and np.array_equal(b["index"].cpu().numpy(), R.sample_windows(eps, W, 7, seed, step, pad)["index"])


def test_rows_depend_on_seed_step_and_row_only():
    W, A, G = 10, 7, 512
    st = data.EpisodeStore(A, G)
    for e in R.make_store(W, A, G, seed=3):
        st.add_episode(e[0], e[1])
    st.finalize()
    s64, s7 = data.WindowStream(st, 64, W, seed=2), data.WindowStream(st, 7, W, seed=2)
    b9, b5 = s64.batch(9), s64.batch(5)
    fresh5, small5 = data.WindowStream(st, 64, W, seed=2).batch(5), s7.batch(5)
    other = data.WindowStream(st, 64, W, seed=3).batch(5)
    for k in ("actions", "action_mask", "latent_goal", "index", "episode", "noise", "u"):
        assert torch.equal(b5[k], fresh5[k]), k                                   # batch(5) after batch(9) == batch(5) of a fresh stream
        assert torch.equal(b5[k][:7], small5[k]), k                               # rows [:7] of B = 64 == the B = 7 batch
    assert not torch.equal(b5["index"], b9["index"]) and not torch.equal(b5["noise"], b9["noise"]) and not torch.equal(b5["u"], b9["u"])
    assert not torch.equal(b5["index"], other["index"]) and not torch.equal(b5["noise"], other["noise"])


def test_frames_come_out_of_the_store_with_the_streams_shifts():
    """12 x 10 and 9 x 9 uint8 frames -> 8 x 8 with shift_pad = 2: rgb_obs == camera.preprocess_cameras on the hand-gathered frames."""
    W, A, G, B, seed, step = 4, 3, 5, 37, 4, 6
    eps = R.make_store(W, A, G, seed=9, cams=((12, 10), (9, 9)))
    st = data.EpisodeStore(A, G)
    for e in eps:
        st.add_episode(*e)
    st.finalize()
    tr = (camera.CameraTransform((8, 8), shift_pad=2), camera.CameraTransform((8, 8), shift_pad=2))
    b = data.WindowStream(st, B, W, seed=seed, camera_transforms=tr).batch(step)
    ref = R.sample_windows(eps, W, B, seed, step, "hold", R.minmax(eps)[::2], shift_pads=(2, 2))
    assert np.array_equal(b["index"].cpu().numpy(), ref["index"])
    sh = [b["shifts"]["rgb_static"], b["shifts"]["rgb_gripper"]]
    for q in range(2):
        assert np.array_equal(sh[q].cpu().numpy(), ref["shifts"][q]) and int(sh[q].min()) >= 0 and int(sh[q].max()) <= 4
    assert not torch.equal(sh[0], sh[1])
    idx = torch.from_numpy(ref["index"].astype(np.int64)).cuda()
    want = camera.preprocess_cameras(st.frames_static[idx], st.frames_gripper[idx], tr[0], tr[1], shifts=(sh[0], sh[1]))
    assert b["rgb_obs"]["rgb_static"].shape == (B, 3, 8, 8)
    assert torch.equal(b["rgb_obs"]["rgb_static"], want[0]) and torch.equal(b["rgb_obs"]["rgb_gripper"], want[1])
    # without a shift pad no shift table is drawn, and the frames are the unshifted transform
    t0 = (camera.CameraTransform((8, 8)), camera.CameraTransform((8, 8), shift_pad=2))
    b0 = data.WindowStream(st, B, W, seed=seed, camera_transforms=t0, frame_dtype=torch.bfloat16).batch(step)
    assert b0["shifts"]["rgb_static"] is None and torch.equal(b0["shifts"]["rgb_gripper"], sh[1])
    want0 = camera.preprocess_cameras(st.frames_static[idx], st.frames_gripper[idx], t0[0], t0[1], shifts=(None, sh[1]), dtype=torch.bfloat16)
    assert torch.equal(b0["rgb_obs"]["rgb_static"], want0[0]) and torch.equal(b0["rgb_obs"]["rgb_gripper"], want0[1])


def test_bad_descriptors_are_refused_before_any_launch():
    W, A, G, B = 4, 3, 5, 7
    eps = R.make_store(W, A, G)
    lo, hi, scale = R.minmax(eps)
    t = H.dev_store(eps, (lo, scale))
    starts_h = R.start_table(t["lengths"], W, "hold")
    starts = torch.from_numpy(starts_h.astype(np.int32)).cuda()
    lib = L.load()
    o = Outs(B, W, A, G, shifts=(True, False))
    def good(**over):
        d = desc(t, o, W, B, 0, 0, starts, int(starts_h[-1]), pads=(2, 0))
        for k, v in over.items():
            setattr(d, k, v)
        return d
    assert lib.mode_data_sample_windows(None, H.stream()) == BAD_ARG
    cases = [(dict(**{k: None}), BAD_ARG) for k in ("actions", "ep_begin", "starts", "goals", "out_actions", "action_mask", "latent_goal", "index", "episode")]
    cases += [(dict(lo=None), BAD_ARG), (dict(scale=None), BAD_ARG)]
    cases += [(dict(**{k: v}), BAD_ARG) for k in ("S", "E", "A", "G", "W", "B", "n_total") for v in (0, -1)]
    cases += [(dict(n_total=16), BAD_ARG), (dict(E=16), BAD_ARG)]                 # more starts / episodes than steps
    cases += [(dict(B=65536), UNSUPPORTED), (dict(W=1366), UNSUPPORTED), (dict(G=4097), UNSUPPORTED)]       # 1366 * 3 = 4098 > 4096
    for over, want in cases:
        assert lib.mode_data_sample_windows(C.byref(good(**over)), H.stream()) == want, over
    d = good(); d.shift_pad[0] = -1
    assert lib.mode_data_sample_windows(C.byref(d), H.stream()) == BAD_ARG
    d = good(); d.shift_pad[0] = 0                                                # a shift table without a pad
    assert lib.mode_data_sample_windows(C.byref(d), H.stream()) == BAD_ARG
    torch.cuda.synchronize()
    assert o.untouched() and bool((o.shifts[0] == -77).all())
    assert lib.mode_data_sample_windows(C.byref(good()), H.stream()) == 0         # the descriptor these were derived from is a good one
    torch.cuda.synchronize()
    assert o.intact() and not o.untouched() and int(o.ints(o.shifts[0]).min()) >= 0 and int(o.ints(o.shifts[0]).max()) <= 4
    # the Python side raises ValueError for the same limits before touching the device
    st = data.EpisodeStore(A, G)
    for e in eps:
        st.add_episode(e[0], e[1])
    st.finalize()
    for kw in (dict(batch_size=0), dict(batch_size=65536), dict(window=1366)):
        with pytest.raises(ValueError):
            data.WindowStream(st, **{**dict(batch_size=B, window=W), **kw})
    with pytest.raises(ValueError, match="holds no frames"):
        data.WindowStream(st, B, W, camera_transforms=(camera.CameraTransform(8), camera.CameraTransform(8)))
