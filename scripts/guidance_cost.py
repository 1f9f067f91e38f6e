#!/usr/bin/env python
"""Cost record of classifier-free guidance: the guided 10-step DDIM chunk at batch B against the unguided chunk at B and at 2B, at the benchmarked
model size (c2: embed_dim 1024, 12 layers, 8 heads, 4 experts top-2, bf16), B in {1, 32, 128}.

The guided chain runs 2B rows between its embedding and its head, so the expectation to confirm or refute is: guided at B costs what unguided costs
at 2B, within the spread that REPEATING the unguided 2B measurement shows.  There is no threshold; the table is the result.

Method: every variant is one hipGraph replay per chunk.  All variants of a batch size are captured and warmed first; then ROUNDS rounds, each timing every
variant in turn (interleaved, so drift hits all alike) over a window of enough replays to last >= WINDOW seconds, between two device events.  The
unguided-2B variant is measured twice per round as two separate entries (2B and 2B'): their difference is the spread of repeating one measurement.
Reported: median / min / max over the rounds of the per-chunk time.  No profiler attached.  The output is section 3 of profiles/guidance.txt.

    python scripts/guidance_cost.py [--out FILE] [--rounds 7] [--window 2.0]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mode_diffusion_policy_amd as M  # noqa: E402
from oracle.weights import get_config, make_inputs, make_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--batches", default="1,32,128")
    ap.add_argument("--scale", type=float, default=2.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guidance_cost.py measures on the GPU: no device found")
    cfg = get_config("c2")
    m = M.MoDeDiT(obs_dim=cfg.obs_dim, goal_dim=cfg.goal_dim, device="cuda", goal_conditioned=True, action_dim=cfg.action_dim, embed_dim=cfg.embed_dim,
                  embed_pdrob=0, attn_pdrop=0.3, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=1, obs_seq_len=1,
                  action_seq_len=cfg.action_seq_len, num_experts=cfg.num_experts, top_k=cfg.top_k, compute_dtype="bf16")
    m.load_state_dict(make_state_dict(cfg, 1))
    m = m.to("cuda").eval()
    plain, guided = M.GCDenoiser(m, 0.5).eval(), M.GCDenoiser(m, 0.5, guidance_scale=a.scale).eval()
    sig = M.get_sigmas_exponential(10, 1e-3, 80.0, "cuda")
    lines = [f"# guided vs unguided 10-step DDIM chunk, c2 bf16, w = {a.scale}; per-chunk time in ms: median [min .. max] over {a.rounds} interleaved rounds of >= {a.window} s",
             f"# device: {torch.cuda.get_device_name(0)}",
             f"{'B':>4} {'unguided B':>24} {'unguided 2B':>24} {'unguided 2B (repeat)':>24} {'guided B':>24} {'guided / unguided 2B':>22} {'repeat / unguided 2B':>22}"]
    for B in [int(b) for b in a.batches.split(",")]:
        inp = {b: {k: v.cuda() for k, v in make_inputs(cfg, b, 7).items()} for b in (B, 2 * B)}
        call = lambda den, b: M.sample_ddim(den, {"state_images": inp[b]["state_images"]}, inp[b]["x0"], inp[b]["goals"], sig, disable=True)
        variants = [("unguided B", plain, B), ("unguided 2B", plain, 2 * B), ("unguided 2B (repeat)", plain, 2 * B), ("guided B", guided, B)]
        reps = {}
        for name, den, b in variants:                                         # capture + warm-up, and the replays a window needs
            for _ in range(3):
                call(den, b)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                call(den, b)
            e1.record(); torch.cuda.synchronize()
            reps[name] = max(10, int(a.window / (e0.elapsed_time(e1) / 10 / 1e3)) + 1)
        times = {name: [] for name, _, _ in variants}
        for _ in range(a.rounds):
            for name, den, b in variants:
                call(den, b)                                                    # the variant's graph was not the last one replayed: one untimed call
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps[name]):
                    call(den, b)
                e1.record(); torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / reps[name])
        med = {k: statistics.median(v) for k, v in times.items()}
        cell = lambda k: f"{med[k]:8.3f} [{min(times[k]):6.3f} .. {max(times[k]):6.3f}]"
        lines.append(f"{B:>4} {cell('unguided B'):>24} {cell('unguided 2B'):>24} {cell('unguided 2B (repeat)'):>24} {cell('guided B'):>24} "
                     f"{med['guided B'] / med['unguided 2B']:>22.4f} {med['unguided 2B (repeat)'] / med['unguided 2B']:>22.4f}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
