"""Cost of the held-out denoising loss per noise level (validation.LevelValidator, csrc/data_stream.hip: mode_val_noise_levels, mode_level_error) on
the MI355X, in the protocol and on the held-out set of scripts/validation_probe.py: the C2 geometry, B = 128, W = 10, A = 7, G = 512, bf16; a store
of ``--episodes`` episodes of 48..80 steps, a quarter of them held out; K = 16 levels (the default density quantiles).

  per batch   (d) the denoiser evaluation alone, ``den(state, noised, goal, sigma)`` with one sigma per row, on pre-staged inputs;
              (d1) ``predict`` on a pre-staged batch (embed by index + the evaluation), (d2) with the sweep and prep launches per batch;
              (a) ``LevelValidator.run(draws=1)`` per batch of the sweep, stored features looked up by ``batch["index"]`` as ``embed``; (b) the same
              with the CALVIN cameras in the sweep (one more launch per batch; the encoders are not what is measured); (c) the same pass written
              with torch indexing on the device and a ``.item()`` per batch.  Host clock around a whole pass plus a device synchronise, divided by
              the number of batches; the arms alternate over ``--rounds`` rounds in ONE process; medians of the rounds with their ranges.
  full pass   ``LevelValidator.run()`` (K draws: every window at every level) next to one ``Validator.run()`` (10-step DDIM) on the same windows.
  launches    ``validation.noise_levels`` and ``validation.level_error``, each alone: ``--iters`` back-to-back calls.

    python scripts/level_loss_probe.py [--rounds 9] [--passes 3] [--iters 200] > profiles/level_loss.txt"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mode_diffusion_policy_amd as M  # noqa: E402
import validation_probe as VP  # noqa: E402
from mode_diffusion_policy_amd import data, validation  # noqa: E402

B, W, A = VP.B, VP.W, VP.A


def torch_level_pass(st, val_ids, den, feats, sigmas, draw):
    """The same pass (one draw) with torch indexing on the device and one read-back per batch (pad='hold', stride 1)."""
    dev, K = st.device, sigmas.shape[0]
    n_e = torch.zeros(st.num_episodes, dtype=torch.long, device=dev)
    n_e[torch.as_tensor(val_ids, device=dev)] = torch.as_tensor(st.lengths[val_ids], device=dev)
    starts = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), n_e.cumsum(0)])
    n_total, begin = int(st.lengths[val_ids].sum()), st.ep_begin.long()
    sq, cnt = torch.zeros(K, dtype=torch.float64, device=dev), torch.zeros(K, dtype=torch.float64, device=dev)
    seen = 0.0
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
        level = (g + draw) % K
        sigma = sigmas[level]
        x = acts + torch.randn(B, W, A, device=dev) * sigma[:, None, None]
        pred = den({"state_images": feats[idx]}, x, st.goals[ep], sigma)
        e = (pred - acts).double()
        sq.index_add_(0, level, (c[:, :, None] * e * e).sum((1, 2)))
        cnt.index_add_(0, level, c.sum(1).double())
        seen += c.sum().item()
    return sq / (A * cnt.clamp_min(1)), seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--episodes", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("level_loss_probe.py measures on an MI355X: no device found, nothing measured")
    import bench
    dev = torch.device("cuda:0")
    print("command: python scripts/level_loss_probe.py " + " ".join(sys.argv[1:]))
    print(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}")
    _, den = bench.build_model(dev)
    den.eval()
    inner = den.inner_model
    stores = {cams: VP.build_store(dev, args.episodes, cams) for cams in (False, True)}
    st = stores[False]
    _, val_ids = data.split_episodes(st, val_fraction=0.25, seed=0)
    feats = torch.randn(st.num_steps, inner.n_img_tokens, inner.obs_dim, device=dev)
    embed = lambda b: {"state_images": feats[b["index"].long()]}
    tr = (M.CameraTransform(VP.OUT), M.CameraTransform(VP.OUT))
    sweeps = {False: data.WindowSweep(st, B, W, episodes=val_ids), True: data.WindowSweep(stores[True], B, W, episodes=val_ids, camera_transforms=tr,
                                                                                          frame_dtype=torch.bfloat16)}
    vals = {cams: M.LevelValidator(den, sw, embed) for cams, sw in sweeps.items()}
    sampler = M.Validator(den, sweeps[False], embed)
    nb, K = len(vals[False]), vals[False].num_levels
    assert len(vals[True]) == nb
    b0 = vals[False].batch(0)
    emb0 = {"state_images": embed(b0)["state_images"].clone()}

    @torch.no_grad()
    def bare():
        for _ in range(nb):
            den(emb0, b0["noised"], b0["latent_goal"], b0["sigma"])

    def staged_predict():                                                        # (a) without the sweep, prep and error launches
        for _ in range(nb):
            vals[False].predict(b0)

    def no_error():                                                              # (a) without the error launch
        for i in range(nb):
            vals[False].predict(vals[False].batch(i))
    torch_pass = torch.no_grad()(lambda: torch_level_pass(st, val_ids, den, feats, vals[False].sigmas, 0))
    arms = {"(d) denoiser evaluation alone, pre-staged inputs": bare,
            "(d1) predict(batch 0): embed by index + the evaluation": staged_predict,
            "(d2) batch(i) + predict: (d1) + the sweep and prep launches": no_error,
            "(a) LevelValidator.run(draws=1), no cameras": lambda: vals[False].run(draws=1),
            "(b) LevelValidator.run(draws=1), cameras in the sweep": lambda: vals[True].run(draws=1),
            "(c) torch indexing + .item() per batch": torch_pass}
    for fn in arms.values():
        for _ in range(2):
            fn()
    res = vals[False].run()
    print(f"validation set: {len(val_ids)} of {st.num_episodes} episodes, {sweeps[False].n_total} windows, {nb} batches of {B}, K = {K} levels; "
          f"loss (a, K draws) {float(res['loss']):.6f}, steps per level {float(res['count_per_level'][0]):.0f}; (c) sees {torch_pass()[1]:.0f} steps per draw")
    print("sigma          " + " ".join(f"{float(s):9.4f}" for s in res["sigmas"]))
    print("loss_per_level " + " ".join(f"{float(s):9.4f}" for s in res["loss_per_level"]))
    got = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            e, w = VP.wall(fn, args.passes)
            got[k].append((e / nb, w / nb))
    VP.report(f"per batch: B = {B}, W = {W}, A = {A}, C2 denoiser {inner.engine.compute_dtype}, one evaluation per window; median of {args.rounds} alternating "
              f"rounds of {args.passes} passes of {nb} batches [min .. max]", got, "us per batch")
    full = {f"LevelValidator.run(): K = {K} draws, {K * nb} batches": lambda: vals[False].run(),
            f"Validator.run(): 10-step DDIM, {nb} batches": lambda: sampler.run()}
    for fn in full.values():
        fn()
    got = {k: [] for k in full}
    for _ in range(args.rounds):
        for k, fn in full.items():
            got[k].append(VP.wall(fn, 1))
    VP.report(f"one full pass over the same {sweeps[False].n_total} windows; median of {args.rounds} alternating rounds of 1 pass [min .. max]", got, "us per pass")
    sq, cnt = torch.zeros(K, W * A, dtype=torch.float64, device=dev), torch.zeros(K, W, dtype=torch.float64, device=dev)
    pred = torch.randn(B, W, A, device=dev)
    solo = {"validation.noise_levels (1 launch, 3 allocations)": lambda: validation.noise_levels(b0["actions"], b0["noise"], b0["window"], vals[False].sigmas, 3),
            "validation.level_error (1 launch)": lambda: validation.level_error(pred, b0["actions"], b0["level"], sq, cnt, mask=b0["action_mask"],
                                                                               weight=b0["valid"])}
    for fn in solo.values():
        VP.wall(fn, 10)
    got = {k: [] for k in solo}
    for _ in range(args.rounds):
        for k, fn in solo.items():
            got[k].append(VP.wall(fn, args.iters))
    VP.report(f"the new launches alone; median of {args.rounds} alternating rounds of {args.iters} back-to-back calls [min .. max]", got, "us per call")


if __name__ == "__main__":
    main()
