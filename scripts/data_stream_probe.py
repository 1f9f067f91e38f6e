"""Cost of the training batch stream (data.EpisodeStore / data.WindowStream, csrc/data_stream.hip) on the MI355X.

  batch()    B = 128, W = 10, A = 7, G = 512, CALVIN cameras (static 200 x 200 and gripper 84 x 84 uint8 -> 224 x 224 bf16, shifts pad 10), a store of
             ``--episodes`` episodes: (a) ``WindowStream.batch`` - two launches; (b) the same batch assembled with torch indexing on the device
             (randint, searchsorted, clamped gathers, randn / rand, a frame gather, then the HIP camera transform); (c) assembled on the host with numpy
             from host copies of the store, pinned, copied, then the HIP camera transform.  The same three without cameras.  Per call: host clock
             around ``--iters`` back-to-back calls (enqueue) and around them plus a device synchronise (wall); the variants alternate over
             ``--rounds`` rounds in ONE process; medians of the rounds.
  agent step the step ``bench.py --mode agent`` times (two FiLM-ResNet-50s at 224 x 224 under bf16 autocast -> GCDenoiser.loss on the C2 model ->
             backward -> AdamW), (a) fed a pre-staged batch as the benchmark feeds it, (b) fed by the stream: batch(t), sigma from the batch's u,
             the masked loss.  Host clock around ``--steps`` steps plus a synchronise, alternating rounds, medians.

    python scripts/data_stream_probe.py [--iters 100] [--rounds 7] [--steps 10] [--skip-agent]      -> profiles/data_stream.txt"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import data, utils  # noqa: E402

B, W, A, G = 128, 10, 7, 512
CAMS = ((200, 200), (84, 84))
OUT, PAD = (224, 224), 10


def build_store(dev, episodes, cams, seed=0):
    """The store and host copies of what it holds (for the host-assembled variant)."""
    rng = np.random.default_rng(seed)
    st = data.EpisodeStore(A, G, device=dev)
    host = dict(actions=[], goals=[], frames=[[], []])
    for _ in range(episodes):
        L = int(rng.integers(48, 81))
        a, g = rng.standard_normal((L, A)).astype(np.float32), rng.standard_normal(G).astype(np.float32)
        fr = [rng.integers(0, 256, (L, h, w, 3), dtype=np.uint8) for h, w in CAMS] if cams else [None, None]
        st.add_episode(a, g, *fr)
        host["actions"].append(a); host["goals"].append(g)
        for q in range(2 if cams else 0):
            host["frames"][q].append(fr[q])
    st.finalize("minmax")
    host["actions"], host["goals"] = np.concatenate(host["actions"]), np.stack(host["goals"])
    host["frames"] = [np.concatenate(f) if f else None for f in host["frames"]]
    host["begin"], host["lo"], host["scale"] = st.ep_begin.cpu().numpy().astype(np.int64), st.lo.cpu().numpy(), st.scale.cpu().numpy()
    return st, host


def torch_batch(st, tr):
    """The batch with torch indexing on the device (pad='hold': every step is a start)."""
    dev = st.device
    S = st.actions.shape[0]
    idx = torch.randint(0, S, (B,), device=dev)
    ep = torch.searchsorted(st.ep_begin.long(), idx, right=True) - 1
    last = st.ep_begin.long()[ep + 1] - 1
    rows = idx[:, None] + torch.arange(W, device=dev)
    mask = (rows <= last[:, None]).float()
    acts = (st.actions[torch.minimum(rows, last[:, None])] - st.lo) * st.scale - 1
    out = dict(actions=acts, action_mask=mask, latent_goal=st.goals[ep], index=idx.int(), episode=ep.int(), noise=torch.randn(B, W, A, device=dev),
               u=torch.rand(B, dtype=torch.float64, device=dev))
    if tr is not None:
        sh = tuple(t.draw_shifts(B, dev) for t in tr)
        out["rgb_obs"] = M.preprocess_cameras(st.frames_static[idx], st.frames_gripper[idx], tr[0], tr[1], shifts=sh, dtype=torch.bfloat16)
    return out


def host_batch(st, host, tr, rng):
    """The batch assembled on the host (numpy), pinned and copied; the camera transform stays on the device."""
    dev = st.device
    S = host["actions"].shape[0]
    idx = rng.integers(0, S, B)
    ep = np.searchsorted(host["begin"], idx, side="right") - 1
    last = host["begin"][ep + 1] - 1
    rows = idx[:, None] + np.arange(W)
    mask = (rows <= last[:, None]).astype(np.float32)
    acts = (host["actions"][np.minimum(rows, last[:, None])] - host["lo"]) * host["scale"] - np.float32(1)
    parts = dict(actions=acts, action_mask=mask, latent_goal=host["goals"][ep], index=idx.astype(np.int32), episode=ep.astype(np.int32),
                 noise=rng.standard_normal((B, W, A), dtype=np.float32), u=rng.random(B))
    if tr is not None:
        parts["f0"], parts["f1"] = host["frames"][0][idx], host["frames"][1][idx]
    out = {k: torch.from_numpy(np.ascontiguousarray(v)).pin_memory().to(dev, non_blocking=True) for k, v in parts.items()}
    if tr is not None:
        sh = tuple(torch.from_numpy(rng.integers(0, 2 * PAD + 1, (B, 2)).astype(np.int32)).pin_memory().to(dev, non_blocking=True) for _ in tr)
        out["rgb_obs"] = M.preprocess_cameras(out.pop("f0"), out.pop("f1"), tr[0], tr[1], shifts=sh, dtype=torch.bfloat16)
    return out


def clock(fn, iters):
    """(enqueue us per call, wall us per call) of `iters` back-to-back calls."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        fn(i)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / iters * 1e6, (time.perf_counter() - t0) / iters * 1e6


def batch_section(dev, episodes, iters, rounds):
    for cams in (True, False):
        st, host = build_store(dev, episodes, cams)
        tr = (M.CameraTransform(OUT, shift_pad=PAD), M.CameraTransform(OUT, shift_pad=PAD)) if cams else None
        stream = data.WindowStream(st, B, W, seed=0, pad="hold", camera_transforms=tr, frame_dtype=torch.bfloat16)
        rng = np.random.default_rng(1)
        arms = {"(a) WindowStream.batch": lambda i: stream.batch(i), "(b) torch indexing on the device": lambda i: torch_batch(st, tr),
                "(c) host numpy, pinned, copied": lambda i: host_batch(st, host, tr, rng)}
        for fn in arms.values():
            clock(fn, 5)
        got = {k: [] for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                got[k].append(clock(fn, iters if k[1] != "c" else max(iters // 5, 5)))
        print(f"\n== batch(): B = {B}, W = {W}, A = {A}, G = {G}, {st.num_episodes} episodes / {st.num_steps} steps, "
              f"{'cameras 200 x 200 + 84 x 84 uint8 -> 224 x 224 bf16, shifts pad 10' if cams else 'no cameras'}; us per call, median of {rounds} "
              f"alternating rounds of {iters} calls [min .. max]")
        print(f"{'variant':36s} {'wall (calls + synchronise)':>36s} {'host enqueue':>34s}")
        for k, v in got.items():
            e, w = [x[0] for x in v], [x[1] for x in v]
            print(f"{k:36s} {statistics.median(w):12.1f} [{min(w):9.1f} .. {max(w):9.1f}] {statistics.median(e):12.1f} [{min(e):9.1f} .. {max(e):9.1f}]")
        del st, host, stream


def agent_section(dev, episodes, steps, rounds):
    import bench
    from mode_diffusion_policy_amd.optim import FlatAdamW, FusedAdamW
    from mode_diffusion_policy_amd.perceptual_encoders import FiLMResNet50Policy, embed_visual_obs
    Ba = 64
    _, den = bench.build_model(dev)
    den.train()
    m = den.inner_model
    torch.manual_seed(0)
    enc_s, enc_g = FiLMResNet50Policy(512).to(dev).train(), FiLMResNet50Policy(512).to(dev).train()
    for enc in (enc_s, enc_g):
        for n_, p_ in enc.named_parameters():
            if n_.startswith("film"):
                torch.nn.init.normal_(p_, std=0.02)
    fuse = m.engine.compute_dtype == "bf16"
    opt = FusedAdamW(m, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05, fuse_expert_step=fuse)
    opt_e = FlatAdamW(list(enc_s.parameters()) + list(enc_g.parameters()), lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05)
    st, _ = build_store(dev, episodes, True)
    tr = (M.CameraTransform(OUT, shift_pad=PAD), M.CameraTransform(OUT, shift_pad=PAD))
    stream = data.WindowStream(st, Ba, W, seed=0, pad="hold", camera_transforms=tr, frame_dtype=torch.float32)
    g = torch.Generator().manual_seed(1)
    rgb_s, rgb_g = torch.randn(Ba, 1, 3, 224, 224, generator=g).to(dev), torch.randn(Ba, 1, 3, 224, 224, generator=g).to(dev)
    goal = torch.randn(Ba, 1, 512, generator=g).to(dev)
    acts, noise = torch.randn(Ba, 10, 7, generator=g).to(dev), torch.randn(Ba, 10, 7, generator=g).to(dev)
    dens = dict(loc=math.log(0.5), scale=0.5, min_value=1e-3, max_value=80.0)
    t = [0]

    def finish(loss):
        loss.backward()
        opt.step(overlap=not fuse)
        opt_e.step()
        opt_e.zero_grad(set_to_none=True)

    def staged():
        sig = utils.rand_log_logistic((Ba,), device=dev, **dens)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            emb = embed_visual_obs(enc_s, enc_g, rgb_s, rgb_g, goal.squeeze(1))
            loss, _ = den.loss(emb, acts, goal, noise, sig)
        finish(loss)

    def streamed():
        b = stream.batch(t[0])
        t[0] += 1
        sig = utils.rand_log_logistic((Ba,), u=b["u"], **dens)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            emb = embed_visual_obs(enc_s, enc_g, b["rgb_obs"]["rgb_static"].unsqueeze(1), b["rgb_obs"]["rgb_gripper"].unsqueeze(1), b["latent_goal"])
            loss, _ = den.loss(emb, b["actions"], b["latent_goal"].unsqueeze(1), b["noise"], sig, action_mask=b["action_mask"])
        finish(loss)
    arms = {"(a) pre-staged batch (the benchmark's feed)": staged, "(b) WindowStream.batch(t) + masked loss": streamed}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            got[k].append(((t1 - t0) / steps * 1e3, (time.perf_counter() - t0) / steps * 1e3))
    print(f"\n== agent training step, B = {Ba} (2 x FiLM-ResNet-50 at 224 x 224, bf16 autocast -> C2 denoiser, bf16 -> backward -> AdamW; fused expert step "
          f"{'on' if fuse else 'off'}); ms per step, median of {rounds} alternating rounds of {steps} steps [min .. max]")
    print(f"{'feed':46s} {'wall (steps + synchronise)':>32s} {'host enqueue':>30s}")
    for k, v in got.items():
        e, w = [x[0] for x in v], [x[1] for x in v]
        print(f"{k:46s} {statistics.median(w):10.3f} [{min(w):8.3f} .. {max(w):8.3f}] {statistics.median(e):10.3f} [{min(e):8.3f} .. {max(e):8.3f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--episodes", type=int, default=32)
    ap.add_argument("--skip-agent", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("data_stream_probe.py measures on an MI355X: no device found, nothing measured")
    dev = torch.device("cuda:0")
    print("command: python scripts/data_stream_probe.py " + " ".join(sys.argv[1:]))
    print(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}")
    batch_section(dev, args.episodes, args.iters, args.rounds)
    if not args.skip_agent:
        agent_section(dev, args.episodes, args.steps, args.rounds)


if __name__ == "__main__":
    main()
