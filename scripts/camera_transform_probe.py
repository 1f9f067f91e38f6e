"""Cost of the camera transform (camera.CameraTransform, csrc/frame_prep.hip) on the MI355X against the torch sequence a user would write
(permute, float, F.interpolate(antialias=True), round, scale, normalise, cast), and of a replanning step of a VectorEnvPolicy that takes the
cameras' uint8 frames against today's float-frame path.

  kernel     CALVIN geometry (static 200 x 200 and gripper 84 x 84 uint8 -> 224 x 224), both cameras per call: rollout (bf16 out) at B = 1 and
             B = 32, training (bf16 out, RandomShiftsAug pad 10) at B = 64.  Device events around ``--iters`` back-to-back calls, the two
             variants alternating over ``--rounds`` rounds; median of the rounds.  Bytes: what the transform must move (uint8 source + output).
  end to end every environment replans at every step (all reset before each step) on the benchmarked model (C2 geometry, bf16, 10-step DDIM) with
             two FiLM-ResNet-50 encoders: (a) uint8 frames, camera_transforms; (b) float-frame policy fed the torch sequence's output, the
             sequence inside the timed region; (c) float-frame policy fed pre-made fp32 frames.  Host clock around step + device synchronise.
  --count-launches   a run of its own: device kernels of ONE call of each variant, from torch.profiler's kernel trace.

    python scripts/camera_transform_probe.py [--iters 200] [--rounds 7] [--steps 40] [--skip-e2e]      -> profiles/camera_transform.txt
    python scripts/camera_transform_probe.py --count-launches"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mode_diffusion_policy_amd as M  # noqa: E402
from mode_diffusion_policy_amd import rollout  # noqa: E402

SRC = {"rgb_static": (200, 200), "rgb_gripper": (84, 84)}
OUT = (224, 224)
COPY_RATE = 6.29e12          # measured device copy rate of the MI355X, bytes / s (profiles/)


def torch_transform(u8, t, dtype):
    """The sequence a user writes today for one camera: uint8 (B, T, H, W, 3) -> (B, T, 3, OH, OW)."""
    B, T = u8.shape[:2]
    x = u8.reshape(B * T, *u8.shape[2:]).permute(0, 3, 1, 2).float()
    x = F.interpolate(x, size=t.size, mode="bilinear", align_corners=False, antialias=True).round_().clamp_(0, 255)
    mean = torch.tensor(t.mean, device=u8.device).view(1, 3, 1, 1)
    std = torch.tensor(t.std, device=u8.device).view(1, 3, 1, 1)
    return ((x / 255.0 - mean) / std).to(dtype).view(B, T, 3, *t.size)


def torch_shift(x, shifts, pad):
    """RandomShiftsAug as the integer crop of the edge-replicated image (what the kernel computes), per frame."""
    B, T, C, H, W = x.shape
    p = F.pad(x.view(B * T, C, H, W).float(), (pad,) * 4, mode="replicate")
    iy = shifts[:, 1].view(-1, 1).long() + torch.arange(H, device=x.device)
    ix = shifts[:, 0].view(-1, 1).long() + torch.arange(W, device=x.device)
    n = torch.arange(B * T, device=x.device).view(-1, 1, 1, 1)
    c = torch.arange(C, device=x.device).view(1, -1, 1, 1)
    return p[n, c, iy.view(B * T, 1, H, 1), ix.view(B * T, 1, 1, W)].to(x.dtype).view(B, T, C, H, W)


def frames(B, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randint(0, 256, (B, 1, *hw, 3), dtype=torch.uint8, generator=g).to(dev) for k, hw in SRC.items()}


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel_section(dev, iters, rounds):
    print(f"== transform alone: static 200 x 200 + gripper 84 x 84 uint8 -> 224 x 224 bf16, both cameras per call; us per call, device events around {iters} "
          f"back-to-back calls, median of {rounds} alternating rounds [min .. max]")
    print(f"{'case':34s} {'HIP 1 launch':>24s} {'torch sequence':>26s} {'MB moved':>9s} {'HIP share of 6.29 TB/s':>23s}")
    for name, B, pad in (("rollout B = 1", 1, 0), ("rollout B = 32", 32, 0), ("training B = 64, shifts pad 10", 64, 10)):
        f = frames(B, dev)
        ts = {k: M.CameraTransform(OUT, shift_pad=pad) for k in SRC}
        sh = tuple(ts[k].draw_shifts(B, dev) for k in SRC) if pad else (None, None)
        outs = tuple(torch.empty(B, 1, 3, *OUT, dtype=torch.bfloat16, device=dev) for _ in SRC)

        def hip():
            M.preprocess_cameras(f["rgb_static"], f["rgb_gripper"], ts["rgb_static"], ts["rgb_gripper"], shifts=sh, out=outs)

        def seq():
            res = []
            for k, s in zip(SRC, sh):
                x = torch_transform(f[k], ts[k], torch.bfloat16)
                res.append(torch_shift(x, s, pad) if pad else x)
            return res
        for fn in (hip, seq):
            event_ms(fn, 10)
        got = {"hip": [], "seq": []}
        for _ in range(rounds):
            got["hip"].append(event_ms(hip, iters) * 1e3)
            got["seq"].append(event_ms(seq, max(iters // 4, 10)) * 1e3)
        nbytes = sum(B * (hw[0] * hw[1] * 3 + 3 * OUT[0] * OUT[1] * 2) for hw in SRC.values())
        h, s = statistics.median(got["hip"]), statistics.median(got["seq"])
        share = nbytes / COPY_RATE / (h * 1e-6)
        note = "  (launch-bound)" if B == 1 else ""
        print(f"{name:34s} {h:8.1f} [{min(got['hip']):6.1f} .. {max(got['hip']):6.1f}] {s:9.1f} [{min(got['seq']):7.1f} .. {max(got['seq']):7.1f}] "
              f"{nbytes / 1e6:9.2f} {100 * share:21.1f} %{note}")


def e2e_section(dev, steps, rounds):
    from vector_env_frames_probe import W, build
    import bench
    den, encs = build(dev)
    ts = {k: M.CameraTransform(OUT) for k in SRC}
    print(f"\n== replanning step of a VectorEnvPolicy, every environment replans (C2 geometry, bf16, 10-step DDIM, two FiLM-ResNet-50 at 224 x 224, bf16 autocast); "
          f"ms per step, host clock around step + device synchronise, median over {rounds} alternating rounds of {steps} steps [min .. max of the rounds' medians]")
    for B in (1, 32):
        f = frames(B, dev, seed=B)
        goal = torch.randn(B, bench.C2["goal_dim"], generator=torch.Generator().manual_seed(B)).to(dev)
        kw = dict(act_window_size=W, multistep=W, action_dim=7, sigma_max=80.0, static_resnet=encs[0], gripper_resnet=encs[1])
        pa, pb = rollout.VectorEnvPolicy(den, B, camera_transforms=ts, **kw), rollout.VectorEnvPolicy(den, B, **kw)
        floats = {"rgb_obs": {k: torch_transform(f[k], ts[k], torch.float32) for k in SRC}}

        def a():
            pa.reset(); pa.step({"rgb_obs": f}, goal)

        def b():
            pb.reset(); pb.step({"rgb_obs": {k: torch_transform(f[k], ts[k], torch.float32) for k in SRC}}, goal)

        def c():
            pb.reset(); pb.step(floats, goal)
        cases = {"(a) uint8 frames, camera_transforms": a, "(b) float policy, torch sequence in the timed region": b, "(c) float policy, pre-made fp32 frames": c}
        for fn in cases.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        meds = {k: [] for k in cases}
        for _ in range(rounds):
            for k, fn in cases.items():
                t = []
                for _ in range(steps):
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    t.append((time.perf_counter() - t0) * 1e3)
                meds[k].append(statistics.median(t))
        print(f"\nB = {B}")
        for k, v in meds.items():
            print(f"  {k:54s} {statistics.median(v):8.3f} [{min(v):7.3f} .. {max(v):7.3f}]")
        del pa, pb


def count_launches(dev):
    from torch.profiler import ProfilerActivity, profile
    print("== device kernels of ONE call (torch.profiler kernel trace, a run of its own), both cameras")
    for name, B, pad in (("rollout B = 1", 1, 0), ("rollout B = 32", 32, 0), ("training B = 64, shifts pad 10", 64, 10)):
        f = frames(B, dev)
        ts = {k: M.CameraTransform(OUT, shift_pad=pad) for k in SRC}
        sh = tuple(ts[k].draw_shifts(B, dev) for k in SRC) if pad else (None, None)

        def hip():
            M.preprocess_cameras(f["rgb_static"], f["rgb_gripper"], ts["rgb_static"], ts["rgb_gripper"], shifts=sh, dtype=torch.bfloat16)

        def seq():
            for k, s in zip(SRC, sh):
                x = torch_transform(f[k], ts[k], torch.bfloat16)
                if pad:
                    torch_shift(x, s, pad)
        counts = {}
        for label, fn in (("HIP", hip), ("torch sequence", seq)):
            fn(); torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            counts[label] = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and not e.name.startswith("Memcpy") and not e.name.startswith("Memset"))
        print(f"{name:34s} HIP {counts['HIP']:3d} kernel(s)   torch sequence {counts['torch sequence']:3d} kernels")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--count-launches", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("camera_transform_probe.py measures on an MI355X: no device found, nothing measured")
    dev = torch.device("cuda:0")
    print("command: python scripts/camera_transform_probe.py " + " ".join(sys.argv[1:]))
    if args.count_launches:
        count_launches(dev)
        return
    kernel_section(dev, args.iters, args.rounds)
    if not args.skip_e2e:
        e2e_section(dev, args.steps, args.rounds)


if __name__ == "__main__":
    main()
