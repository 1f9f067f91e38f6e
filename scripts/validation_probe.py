"""Cost of device-side validation (data.WindowSweep, validation.Validator, csrc/data_stream.hip) on the MI355X, at the C2 geometry: B = 128, W = 10,
A = 7, G = 512, bf16, 10-step DDIM; a store of ``--episodes`` episodes of 48..80 steps, a quarter of them held out.

  per batch   (s) ``ChunkedRolloutPolicy.denoise_actions`` at B = 128 on pre-staged inputs - the sampler alone;
              (s1) / (s2) the pieces of (a): ``predict`` on a pre-staged sweep batch, then with the sweep's launch per batch;
              (a) ``Validator.run()`` per batch of the sweep, stored features looked up by ``batch["index"]`` as ``embed``; (b) the same with the
              CALVIN cameras in the sweep (static 200 x 200 and gripper 84 x 84 uint8 -> 224 x 224 bf16: one more launch per batch; ``embed`` still
              looks the stored features up, the encoders are not what is measured); (c) the same validation written with torch indexing on the
              device and a ``.item()`` per batch.  Host clock around a whole pass plus a device synchronise, divided by the number of batches; the
              arms alternate over ``--rounds`` rounds in ONE process; medians of the rounds.
  launches    ``WindowSweep.batch`` without and with cameras, and ``validation.action_error``, each alone: ``--iters`` back-to-back calls.

    python scripts/validation_probe.py [--rounds 9] [--passes 3] [--iters 200]      -> profiles/validation.txt"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import data, rollout, validation  # noqa: E402

B, W, A, G = 128, 10, 7, 512
CAMS = ((200, 200), (84, 84))
OUT = (224, 224)


def build_store(dev, episodes, cams, seed=0):
    rng, frng = np.random.default_rng(seed), np.random.default_rng(seed + 1)     # the same episodes with and without cameras
    st = data.EpisodeStore(A, G, device=dev)
    for _ in range(episodes):
        L = int(rng.integers(48, 81))
        fr = [frng.integers(0, 256, (L, h, w, 3), dtype=np.uint8) for h, w in CAMS] if cams else [None, None]
        st.add_episode(rng.standard_normal((L, A)).astype(np.float32), rng.standard_normal(G).astype(np.float32), *fr)
    return st.finalize("minmax")


def torch_validation(st, val_ids, policy, feats, unit):
    """The same pass with torch indexing on the device and one read-back per batch (pad='hold', stride 1)."""
    dev = st.device
    n_e = torch.zeros(st.num_episodes, dtype=torch.long, device=dev)
    n_e[torch.as_tensor(val_ids, device=dev)] = torch.as_tensor(st.lengths[val_ids], device=dev)
    starts = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), n_e.cumsum(0)])
    n_total, begin = int(st.lengths[val_ids].sum()), st.ep_begin.long()
    sq = cnt = 0.0
    for i in range(-(-n_total // B)):
        g = torch.arange(i * B, (i + 1) * B, device=dev)
        valid = (g < n_total).float()
        g = g.clamp(max=n_total - 1)
        ep = torch.searchsorted(starts, g, right=True) - 1
        idx = begin[ep] + g - starts[ep]
        last = begin[ep + 1] - 1
        rows = idx[:, None] + torch.arange(W, device=dev)
        c = (rows <= last[:, None]).float() * valid[:, None]
        acts = (st.actions[torch.minimum(rows, last[:, None])] - st.lo) * st.scale - 1
        x = torch.randn(B, W, A, device=dev) * policy.sigma_max
        pred = policy.denoise_actions({"state_images": feats[idx]}, st.goals[ep], x=x)
        e = (pred - acts).double() * unit
        sq += (c[:, :, None] * e * e).sum().item()
        cnt += c.sum().item()
    return sq / (A * cnt)


def wall(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / n * 1e6, (time.perf_counter() - t0) / n * 1e6


def report(title, got, unit):
    print(f"\n== {title}")
    print(f"{'arm':64s} {'wall (calls + synchronise), ' + unit:>40s} {'host enqueue, ' + unit:>36s}")
    for k, v in got.items():
        e, w = [x[0] for x in v], [x[1] for x in v]
        print(f"{k:64s} {statistics.median(w):14.1f} [{min(w):10.1f} .. {max(w):10.1f}] {statistics.median(e):12.1f} [{min(e):10.1f} .. {max(e):10.1f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--episodes", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("validation_probe.py measures on an MI355X: no device found, nothing measured")
    import bench
    dev = torch.device("cuda:0")
    print("command: python scripts/validation_probe.py " + " ".join(sys.argv[1:]))
    print(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}")
    _, den = bench.build_model(dev)
    den.eval()
    inner = den.inner_model
    stores = {cams: build_store(dev, args.episodes, cams) for cams in (False, True)}
    st = stores[False]
    _, val_ids = data.split_episodes(st, val_fraction=0.25, seed=0)
    feats = torch.randn(st.num_steps, inner.n_img_tokens, inner.obs_dim, device=dev)
    embed = lambda b: {"state_images": feats[b["index"].long()]}
    tr = (M.CameraTransform(OUT), M.CameraTransform(OUT))
    sweeps = {False: data.WindowSweep(st, B, W, episodes=val_ids), True: data.WindowSweep(stores[True], B, W, episodes=val_ids, camera_transforms=tr,
                                                                                          frame_dtype=torch.bfloat16)}
    vals = {cams: M.Validator(den, sw, embed) for cams, sw in sweeps.items()}
    nb = len(vals[False])
    assert len(vals[True]) == nb
    pol = rollout.ChunkedRolloutPolicy(den)
    b0 = vals[False].batch(0)
    emb0, goal0 = {"state_images": embed(b0)["state_images"].clone()}, b0["latent_goal"].clone()
    unit = vals[False].unit

    def bare():
        for _ in range(nb):
            pol.denoise_actions(emb0, goal0)

    def staged_predict():                                                        # (a) without the sweep and error launches
        for _ in range(nb):
            vals[False].predict(b0)

    def no_error():                                                              # (a) without the error launch
        for i in range(nb):
            vals[False].predict(vals[False].batch(i))
    arms = {"(s) denoise_actions alone, pre-staged inputs": bare,
            "(s1) predict(batch 0): embed by index + sampler on its noise": staged_predict,
            "(s2) batch(i) + predict: (s1) + the sweep launch": no_error,
            "(a) Validator.run(), no cameras": lambda: vals[False].run(),
            "(b) Validator.run(), cameras in the sweep": lambda: vals[True].run(),
            "(c) torch indexing + .item() per batch": lambda: torch_validation(st, val_ids, pol, feats, unit)}
    for fn in arms.values():
        for _ in range(2):
            fn()
    print(f"validation set: {len(val_ids)} of {st.num_episodes} episodes, {sweeps[False].n_total} windows, {nb} batches of {B}; "
          f"mse (a) {float(vals[False].run()['mse']):.6f}, (c, other noise) {arms['(c) torch indexing + .item() per batch']():.6f}")
    got = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            e, w = wall(fn, args.passes)
            got[k].append((e / nb, w / nb))
    report(f"per batch: B = {B}, W = {W}, A = {A}, C2 denoiser {inner.engine.compute_dtype}, 10-step DDIM; median of {args.rounds} alternating rounds of "
           f"{args.passes} passes of {nb} batches [min .. max]", got, "us per batch")
    sq, ab = (torch.zeros(W * A, dtype=torch.float64, device=dev) for _ in range(2))
    cnt = torch.zeros(W, dtype=torch.float64, device=dev)
    pred = torch.randn(B, W, A, device=dev)
    solo = {"WindowSweep.batch, no cameras (1 launch)": lambda: sweeps[False].batch(0, noise_scale=80.0),
            "WindowSweep.batch, cameras (2 launches)": lambda: sweeps[True].batch(0, noise_scale=80.0),
            "validation.action_error (1 launch)": lambda: validation.action_error(pred, b0["actions"], sq, ab, cnt, mask=b0["action_mask"], weight=b0["valid"],
                                                                                    unit=unit)}
    for fn in solo.values():
        wall(fn, 10)
    got = {k: [] for k in solo}
    for _ in range(args.rounds):
        for k, fn in solo.items():
            got[k].append(wall(fn, args.iters))
    report(f"the new launches alone; median of {args.rounds} alternating rounds of {args.iters} back-to-back calls [min .. max]", got, "us per call")


if __name__ == "__main__":
    main()
