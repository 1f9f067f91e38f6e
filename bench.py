"""bench.py — MoDE denoising hot path on MI355X.

Metric (BASELINE.json): denoise-steps/sec at B=128 with the 10-step DDIM chunk, full MoDE denoiser (12 layers, d=1024, 8 heads,
4 experts top-2, obs_dim 2048, goal_dim 512), bf16 MFMA compute with fp32 accumulate / fp32 router, synthetic CALVIN-shaped
inputs, random-init weights (no datasets or checkpoints are reachable).

A bench "step" = ONE 10-step DDIM chunk over one batch of B=128 action chunks (sample_ddim o GCDenoiser o MoDeDiT, i.e. 10
denoiser forwards + 10 fused EDM/DDIM updates, replayed as one hipGraph).  value = n_gpus * steps * 10 / wall  [denoise-steps/s].
Multi-GPU (inference): replicas only — each rank denoises its own B=128 batch, no data-path collective.

A plain run measures the headline and nothing else: set-up (including the training state's device allocation, which the headline has always
been measured on top of: main), warm-up, the timed steps, the --dump-outputs file, the JSON line.  --full adds,
after the timed steps and in the same invocation, everything else this file measures: the dominant kernel's roofline and the sustained MFMA
rate, the per-kernel breakdown, the rollout / B=1 / sampler / encoder legs, the data-parallel *training* step (configs[2]/[3]: fwd + bwd +
gradient exchange + fused AdamW, on every rank: train_* / dp_mode / rccl_ranks; also stand-alone: --mode train), the agent's legs and the
CPU baseline.  In --mode rollout it adds the agent's replanning call.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 1 --steps 20 --warmup 3 --full
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

C2 = dict(obs_dim=2048, goal_dim=512, embed_dim=1024, n_layers=12, n_heads=8, num_experts=4, top_k=2)
B_PER_GPU = 128
N_SAMPLING_STEPS = 10
SIGMA_DATA, SIGMA_MIN, SIGMA_MAX = 0.5, 1e-3, 80.0
MFMA_BF16_PEAK_TFLOPS = 2500.0          # dense bf16 MFMA peak, MI355X_MICROARCH.md (AMD's 5 PF figure is 2:1 sparse)
HBM_PEAK_GBS = 8000.0


def flops_per_denoise_step(B, L=12, D=1024, H=8, T=14, E=4, k=2, O=2048, G=512, A=7, A_len=10):
    """Algorithmic FLOPs of one denoiser forward on the whole batch (SURVEY.md §8d / BASELINE.md §4)."""
    N = B * T
    hd = D // H
    per_layer = 6 * N * D * D + 4 * B * H * T * T * hd + 2 * N * D * D + (4 * B * D * D + 4 * B * D * E) + k * 24 * N * D * D
    return L * per_layer + 2 * B * (2 * O * D + G * D + A_len * A * D + D * D + A_len * D * A)


def flops_executed_per_chunk(B, steps=N_SAMPLING_STEPS, L=12, D=1024, H=8, T=14, E=4, k=2, O=2048, G=512, A=7, A_len=10):
    """FLOPs the timed region actually EXECUTES for one `steps`-step DDIM chunk.  The counted figure above prices the router
    on B rows and the observation / sigma embeddings once per denoise step; the fused sampler runs the router + sigma-embedding on ONE row per
    noise level once per SCHEDULE (outside the chunk: the schedule state is rebuilt only when sigmas / weights change) and the observation + goal
    embeddings once per CHUNK.  Reported beside the counted fraction as `e2e_mfma_frac_executed`."""
    N = B * T
    hd = D // H
    per_layer = 6 * N * D * D + 4 * B * H * T * T * hd + 2 * N * D * D + k * 24 * N * D * D
    per_step = L * per_layer + 2 * B * (A_len * A * D + A_len * D * A)
    per_chunk = 2 * B * (2 * O * D + G * D)
    return steps * per_step + per_chunk


def _dry_run_layers():
    """MODE_BENCH_DRYRUN_LAYERS=n: a PLUMBING run of this file with an n-layer model (the world-2 test on one GPU, where the collective is gloo through
    host memory).  The JSON line then carries "dry_run": true and is not a measurement of BASELINE's configuration."""
    return int(os.environ.get("MODE_BENCH_DRYRUN_LAYERS", "0"))


def build_model(device, dtype="bf16"):
    import mode_diffusion_policy_amd as M
    torch.manual_seed(0)
    m = M.MoDeDiT(obs_dim=C2["obs_dim"], goal_dim=C2["goal_dim"], device=str(device), goal_conditioned=True, action_dim=7,
                  embed_dim=C2["embed_dim"], embed_pdrob=0, attn_pdrop=0.3, n_layers=_dry_run_layers() or C2["n_layers"], n_heads=C2["n_heads"],
                  goal_seq_len=1, obs_seq_len=1, action_seq_len=10, mlp_pdrop=0.1, goal_drop=0.1, num_experts=C2["num_experts"],
                  top_k=C2["top_k"], compute_dtype=dtype)
    return M, M.GCDenoiser(m.to(device).eval(), SIGMA_DATA).eval()


def synthetic_inputs(device, B):
    g = torch.Generator(device="cpu").manual_seed(0)
    img = torch.randn(B, 2, C2["obs_dim"], generator=g).to(device)
    goal = torch.randn(B, 1, C2["goal_dim"], generator=g).to(device)
    x0 = (torch.randn(B, 10, 7, generator=g) * SIGMA_MAX).to(device)
    return img, goal, x0


class PowerSampler:
    """Socket power and shader clock of THIS process's GPU, sampled from the amdgpu hwmon files while a timed region runs.  The expert GEMMs
    run the socket into its power cap (LABNOTES.md section 8: 1377 W of 1400 W, 1.8-1.9 GHz instead of the 2.4 GHz the 2.5 PF/s peak is quoted at),
    so the clock under load belongs next to every fraction-of-peak this file reports.  Best effort: every field is None when sysfs is not
    readable (other driver, container without /sys)."""

    def __init__(self, device_index=0, period_s=0.02):
        import glob
        self.dir, self.period, self.pw, self.ck, self._t, self._stop = None, period_s, [], [], None, False
        try:
            import ctypes
            buf = ctypes.create_string_buffer(64)
            if ctypes.CDLL("libamdhip64.so").hipDeviceGetPCIBusId(buf, 64, int(device_index)) != 0:
                raise OSError("hipDeviceGetPCIBusId")
            bdf = buf.value.decode().lower()
            hits = glob.glob(f"/sys/bus/pci/devices/{bdf}/hwmon/hwmon*")
            if hits:
                self.dir = hits[0]
        except Exception:
            self.dir = None

    def _read(self, name):
        try:
            with open(os.path.join(self.dir, name)) as f:
                return int(f.read().strip())
        except Exception:
            return None

    def _loop(self):
        while not self._stop:
            w = self._read("power1_input")
            if w is None:
                w = self._read("power1_average")
            c = self._read("freq1_input")
            if w is not None:
                self.pw.append(w / 1e6)
            if c is not None:
                self.ck.append(c / 1e6)
            time.sleep(self.period)

    def __enter__(self):
        if self.dir:
            import threading
            self._t = threading.Thread(target=self._loop, daemon=True)
            self._t.start()
        return self

    def __exit__(self, *exc):
        self._stop = True
        if self._t:
            self._t.join()

    def summary(self):
        cap = self._read("power1_cap") if self.dir else None
        avg = lambda v: round(sum(v) / len(v), 1) if v else None
        return {"socket_w_avg": avg(self.pw), "socket_w_max": round(max(self.pw), 1) if self.pw else None, "cap_w": cap / 1e6 if cap else None,
                "sclk_mhz_avg": avg(self.ck), "sclk_mhz_min": round(min(self.ck), 1) if self.ck else None, "samples": len(self.pw),
                "source": "amdgpu hwmon power1_input / freq1_input, 20-ms samples over the timed region" if self.dir else None}


def sustained_mfma_peak(device, seconds=1.2):
    """What the socket sustains in bf16 MFMA at its power cap: register-resident v_mfma_f32_16x16x32_bf16 on every SIMD (mode_probe_mfma_burn,
    csrc/probe.hip), back-to-back launches for `seconds`, rate of the last block.  The datasheet peak (2.5 PF/s at 2.4 GHz) is what every `frac`
    of this file is quoted against; this number says how much of it the box delivers under load (LABNOTES.md section 8)."""
    import ctypes as C
    from mode_diffusion_policy_amd import _lib as L
    lib = L.load()
    seed = torch.tensor([12345], dtype=torch.int32, device=device)
    ncu = torch.cuda.get_device_properties(device).multi_processor_count
    fl = C.c_double(0.0)
    st = torch.cuda.current_stream().cuda_stream
    iters = 4000                                              # ~0.55 ms per launch
    L.check(lib.mode_probe_mfma_burn(seed.data_ptr(), None, ncu, iters, C.byref(fl), st))
    torch.cuda.synchronize()
    t_end = time.perf_counter() + seconds
    rate = 0.0
    with PowerSampler(device.index or 0, period_s=0.01) as ps:
        while time.perf_counter() < t_end:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                lib.mode_probe_mfma_burn(seed.data_ptr(), None, ncu, iters, None, st)
            e1.record(); torch.cuda.synchronize()
            rate = fl.value * 100 / (e0.elapsed_time(e1) * 1e-3) / 1e12
    return {"tflops": round(rate, 1), "frac_of_datasheet_peak": round(rate / MFMA_BF16_PEAK_TFLOPS, 4), "power": ps.summary(),
            "what": "register-resident v_mfma_f32_16x16x32_bf16 on all SIMDs, sustained (last 100-launch block of a 1.2-s burst)"}


def dominant_kernel_roofline(den, device, reps=240):
    """Dominant kernel = grouped bf16 MFMA GEMM with SwishGLU epilogue (expert up-projection: 47 % of all FLOPs).  Launch it in
    isolation at the benchmark's exact shape (3584 gathered rows = 1792 tokens x top-2, K = 1024, 2 x 4096 weight rows per expert),
    cycling through the 12 layers' weights, as one hipGraph replay timed with HIP events on the stream it is launched on."""
    import ctypes as C
    from mode_diffusion_policy_amd import _lib as L
    from mode_diffusion_policy_amd.engine import capture_graph
    m = den.inner_model
    eng = m.engine
    lib = L.load()
    D, E, k, T = 1024, 4, 2, 14
    N = B_PER_GPU * T
    idx = torch.tensor([[1, 2]], dtype=torch.int32, device=device)
    w = torch.tensor([[0.6, 0.4]], dtype=torch.float32, device=device)
    meta = eng.dispatch(idx, w, 1, 1, N, N)
    ml = eng.meta_layout(N)
    mp = meta.data_ptr()
    u = torch.randn(N, D, device=device).to(torch.bfloat16)
    Hb = torch.empty(N * k, 4 * D, dtype=torch.bfloat16, device=device)
    ss = torch.rand(N, D // 64, device=device) + 0.5          # per-64-column sums of squares of the fused ln_2 (the chain's variant of the kernel)
    descs = []
    for l in range(m.num_layers):
        kp = {**eng.arena.w, **eng.arena.wl}
        d = L.ModeGemmDesc(dtype=L.MODE_BF16, epilogue=L.EPI_SWIGLU, out_dtype=L.MODE_BF16, M=N * k, N=4 * D, K=D, A=u.data_ptr(), lda=D,
                           W=kp[f"l{l}.w1"].data_ptr(), ldw=D, w_expert_stride=8 * D * D, bias=kp[f"l{l}.b1"].data_ptr(),
                           bias_expert_stride=8 * D, resid=None, ldr=0, C=Hb.data_ptr(), ldc=4 * D, a_rows=mp + 4 * ml.perm,
                           expert_offsets=mp + 4 * ml.offsets, num_experts=E, row_ss=ss.data_ptr(), row_ss_n=D // 64, row_eps=1e-6,
                           flags=L.GEMM_UNIFORM_GROUPS)                   # the sampler's hint: every sample routes alike (dit.hip sets it the same way)
        descs.append(d)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(4):                                        # warm-up: clocks, code objects, L2/MALL state of a steady layer loop
        for d in descs:
            L.check(lib.mode_gemm(C.byref(d), st))
    torch.cuda.synchronize()
    # the `reps` launches are recorded into one hipGraph and replayed between two events on the replay stream: back-to-back launches like in
    # the sampler's chain, no host launch gaps inside the timed region
    g = torch.cuda.CUDAGraph()
    with capture_graph(g):
        cst = torch.cuda.current_stream().cuda_stream
        for i in range(reps):
            L.check(lib.mode_gemm(C.byref(descs[i % len(descs)]), cst))
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    with PowerSampler(device.index or 0, period_s=0.005) as ps:   # the same graph replayed for ~0.3 s: power and clock of the kernel on its own
        for _ in range(20):
            g.replay()
        torch.cuda.synchronize()
    flops = 2.0 * (N * k) * D * (8 * D)
    ach = flops / (us * 1e-6) / 1e12
    # HBM bytes per launch: NOT a literal - read from the machine-readable summary scripts/pmc_summary.py writes from the separate
    # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this very command (FETCH_SIZE doubled: gfx950 correction, MI355X_MICROARCH.md "HBM");
    # null when the summary is absent or was taken on another kernel.
    traffic, src = None, None
    for fn in ("r06_gemm_pmc.json", "r05_gemm_pmc.json", "r04_gemm_pmc.json", "r03_gemm_pmc.json", "r02_gemm_pmc.json"):                 # the newest committed collection that sampled THIS kernel
        try:
            pj = json.load(open(os.path.join(ROOT, "profiles", fn)))
            ent = pj["kernels"].get("expert_up_projection")
            if ent and ent.get("kernel_substr", "").startswith("gemm_pp_kernel<4, true, 3"):
                traffic, src = ent["hbm_bytes_per_launch"], f"profiles/{fn} (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, separate passes)"
                break
        except Exception:
            pass
    return {"bound": "mfma", "kernel": "gemm_pp_kernel<SWIGLU, bf16, 224x256> (grouped expert up-projection + fused ln_2 scale + SwiGLU, M=3584 K=1024 N=2x4096)",
            "achieved": round(ach, 1), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / MFMA_BF16_PEAK_TFLOPS, 4),
            # algorithmic bytes per launch (2 of 4 experts active under uniform sigma): A 3.7 MB + W1 33.6 MB + H 29.4 MB = 66.6 MB (LABNOTES.md section 4)
            "traffic": traffic, "traffic_source": src, "algorithmic_bytes": 66.6e6, "avg_launch_us": round(us, 2), "flops_per_launch": flops,
            "power": ps.summary()}


def layer_kernel_breakdown(den, device, reps=120):
    """The six kernels of one transformer block at the benchmark shape (B=128, N=1792 tokens), each timed in isolation as a hipGraph of `reps`
    launches cycling the 12 layers' weights (HIP events on the replay stream): {name: {us, frac, bound}}; frac against the roof that bounds it."""
    import ctypes as C
    from mode_diffusion_policy_amd import _lib as L
    from mode_diffusion_policy_amd.engine import capture_graph
    m = den.inner_model
    eng = m.engine
    lib = L.load()
    D, E, k, T, H = 1024, 4, 2, 14, 8
    B = B_PER_GPU
    N, NK = B * T, B * T * 2
    bf = torch.bfloat16
    idx = torch.tensor([[1, 2]], dtype=torch.int32, device=device); w = torch.tensor([[0.6, 0.4]], dtype=torch.float32, device=device)
    meta = eng.dispatch(idx, w, 1, 1, N, N); ml = eng.meta_layout(N); mp = meta.data_ptr()
    kp = {**eng.arena.w, **eng.arena.wl}
    h = torch.randn(N, D, device=device).to(bf); qkv = torch.empty(N, 3 * D, dtype=bf, device=device); yat = torch.randn(N, D, device=device).to(bf)
    x = torch.randn(N, D, device=device); xo = torch.empty(N, D, device=device); h2 = torch.empty(N, D, dtype=bf, device=device)
    ss = torch.rand(N, D // 64, device=device) + 0.5
    Hb = torch.randn(NK, 4 * D, device=device).to(bf) * 0.1
    S = 4
    Y = torch.empty(S, NK, D, dtype=bf, device=device)
    cond = torch.randn(1, D, device=device)
    st_of = lambda: torch.cuda.current_stream().cuda_stream
    Ly = m.num_layers

    def g(**kw):
        base = dict(dtype=L.MODE_BF16, epilogue=L.EPI_NONE, out_dtype=L.MODE_BF16, M=N, N=D, K=D, A=h.data_ptr(), lda=D, W=None, ldw=D, C=None, ldc=D)
        base.update(kw)
        return L.ModeGemmDesc(**base)
    qkv_d = [g(epilogue=L.EPI_BIAS, N=3 * D, W=kp[f"l{l}.wqkv"].data_ptr(), bias=kp[f"l{l}.bqkv"].data_ptr(), C=qkv.data_ptr(), ldc=3 * D) for l in range(Ly)]
    cpr_d = [g(epilogue=L.EPI_RESIDUAL_NORM, out_dtype=L.MODE_F32, A=yat.data_ptr(), W=kp[f"l{l}.wo"].data_ptr(), resid=x.data_ptr(), ldr=D, C=xo.data_ptr(),
               C2=h2.data_ptr(), ldc2=D, gain=kp["ln2_g"][l].data_ptr(), row_ss_out=ss.data_ptr()) for l in range(Ly)]
    up_d = [g(epilogue=L.EPI_SWIGLU, M=NK, N=4 * D, W=kp[f"l{l}.w1"].data_ptr(), w_expert_stride=8 * D * D, bias=kp[f"l{l}.b1"].data_ptr(),
              bias_expert_stride=8 * D, C=Hb.data_ptr(), ldc=4 * D, a_rows=mp + 4 * ml.perm, expert_offsets=mp + 4 * ml.offsets, num_experts=E,
              row_ss=ss.data_ptr(), row_ss_n=D // 64, row_eps=1e-6, flags=L.GEMM_UNIFORM_GROUPS) for l in range(Ly)]
    dn_d = [g(M=NK, N=D, K=4 * D, A=Hb.data_ptr(), lda=4 * D, W=kp[f"l{l}.w2"].data_ptr(), ldw=4 * D, w_expert_stride=4 * D * D, C=Y.data_ptr(),
              expert_offsets=mp + 4 * ml.offsets, num_experts=E, split_k=S, split_stride=NK * D, flags=L.GEMM_UNIFORM_GROUPS) for l in range(Ly)]

    def gemm(ds):
        return lambda i, st: L.check(lib.mode_gemm(C.byref(ds[i % Ly]), st))

    def attn(i, st):
        L.check(lib.mode_attn_block_fwd(qkv.data_ptr(), kp["qn_g"][i % Ly].data_ptr(), kp["kn_g"][i % Ly].data_ptr(), yat.data_ptr(), L.MODE_BF16, B, T, H, D // H,
                                        1e-6, 0, 0.0, st))

    def comb(i, st):
        l = i % Ly
        L.check(lib.mode_moe_combine_norm_fused_fwd(xo.data_ptr(), ss.data_ptr(), D // 64, kp["ln2_g"][l].data_ptr(), Y.data_ptr(), L.MODE_BF16, S, NK * D,
                                                    mp + 4 * ml.pos, mp + 4 * ml.posw, N, D, k, kp["ln1_g"][(l + 1) % Ly].data_ptr(), cond.data_ptr(), N, 1e-6,
                                                    x.data_ptr(), h.data_ptr(), L.MODE_BF16, st))
    def qkv_attn(i, st):
        l = i % Ly
        qa = L.ModeQkvAttnDesc(dtype=L.MODE_BF16, B=B, T=T, H=H, D=D, h=h.data_ptr(), ldh=D, wqkv=kp[f"l{l}.wqkv"].data_ptr(), ldw=D, bqkv=kp[f"l{l}.bqkv"].data_ptr(),
                               q_gain=kp["qn_g"][l].data_ptr(), k_gain=kp["kn_g"][l].data_ptr(), eps=1e-6, y=yat.data_ptr(), ldy=D)
        L.check(lib.mode_qkv_attn_fwd(C.byref(qa), st))
    MB = 1e6
    attn_flops = 4.0 * B * H * T * T * (D // H)
    # the chain runs QKV projection + attention as ONE launch at this batch (round 4, qkv_attn.hip); the two kernels it replaces are timed for reference
    # ("unfused:" entries, not part of sum_us)
    items = [("qkv_gemm+attention", qkv_attn, "mfma", 2.0 * N * D * 3 * D + attn_flops),
             ("unfused:qkv_gemm", gemm(qkv_d), "mfma", 2.0 * N * D * 3 * D),
             ("unfused:attention", attn, "hbm", (N * 3 * D + N * D) * 2.0),
             ("c_proj_gemm+resid+ln2", gemm(cpr_d), "mfma", 2.0 * N * D * D),
             ("expert_up_gemm+swiglu", gemm(up_d), "mfma", 2.0 * NK * D * 8 * D),
             ("expert_down_gemm_4slices", gemm(dn_d), "mfma", 2.0 * NK * 4 * D * D),
             ("combine+ln1", comb, "hbm", N * D * (4 + 4 + 2) + S * NK * D * 2.0 + N * 16 * 4)]
    out = {}
    for name, fn, bound, work in items:
        for i in range(Ly):
            fn(i, st_of())
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with capture_graph(gr):
            cst = st_of()
            for i in range(reps):
                fn(i, cst)
        gr.replay(); torch.cuda.synchronize()
        us = 1e9
        for _ in range(3):                                                    # best of three replays (clock ramps / other kernels' tails between the legs)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); gr.replay(); e1.record(); torch.cuda.synchronize()
            us = min(us, e0.elapsed_time(e1) * 1e3 / reps)
        peak = MFMA_BF16_PEAK_TFLOPS * 1e12 if bound == "mfma" else HBM_PEAK_GBS * 1e9
        out[name] = {"us": round(us, 2), "bound": bound, "frac": round(work / (us * 1e-6) / peak, 4)}
    out["sum_us"] = round(sum(v["us"] for n_, v in out.items() if not n_.startswith("unfused:")), 1)
    return out


def _cpu_cores():
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:                                            # container CPU quota (cgroup v2): "max" or "<quota> <period>"
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            cores = max(1, min(cores, int(int(q) / int(per))))
    except Exception:
        pass
    return cores


def cpu_baseline():
    """BASELINE.md section 3 protocol: the CPU restatement (oracle/mode_oracle.py: pure-torch fp32, parity-pinned to the reference) on this box's
    host cores, `torch.set_num_threads(cores)`: 1 warm-up + 3 timed runs of the full 10-step DDIM chunk, median, at C1 (B=8) and C2 (B=128).
    Bounded: if one C2 chunk takes longer than 25 s only ONE timed C2 run follows the warm-up (the protocol line says so)."""
    from oracle import mode_oracle as O
    from oracle.weights import param_spec
    cores = _cpu_cores()
    torch.set_num_threads(cores)
    legs = {}
    for leg, kw, B in (("c1", dict(obs_dim=512, goal_dim=512, embed_dim=256, n_layers=2, n_heads=8, num_experts=2, top_k=1), 8), ("c2", C2, B_PER_GPU)):
        cfg = O.DiTConfig(**kw)
        g = torch.Generator().manual_seed(0)
        sd = {}
        for name, shape in param_spec(cfg):
            if name.endswith(".g"):
                sd[name] = torch.ones(shape)
            elif name.endswith("bias") or name == "pos_emb":
                sd[name] = torch.zeros(shape)
            else:
                sd[name] = torch.randn(shape, generator=g) * (shape[-1] ** -0.5)
        img = torch.randn(B, 2, cfg.obs_dim, generator=g); goal = torch.randn(B, 1, cfg.goal_dim, generator=g)
        x0 = torch.randn(B, 10, 7, generator=g) * SIGMA_MAX
        sig = O.get_sigmas_exponential(N_SAMPLING_STEPS, SIGMA_MIN, SIGMA_MAX)
        times = []
        with torch.no_grad():
            t0 = time.perf_counter(); O.sample_ddim(sd, cfg, SIGMA_DATA, img, x0, goal, sig); warm = time.perf_counter() - t0
            for _ in range(3 if warm <= 25.0 else 1):
                t0 = time.perf_counter(); O.sample_ddim(sd, cfg, SIGMA_DATA, img, x0, goal, sig); times.append(time.perf_counter() - t0)
        med = sorted(times)[len(times) // 2]
        legs[leg] = {"denoise_steps_per_s": round(N_SAMPLING_STEPS / med, 4), "ms_per_denoise_step": round(med / N_SAMPLING_STEPS * 1e3, 2),
                     "timed_chunks": len(times), "warmup_chunk_s": round(warm, 2)}
    model = ""
    try:
        model = [l.split(":")[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
    except Exception:
        pass
    c2 = legs["c2"]
    return {"value": c2["denoise_steps_per_s"], "unit": "denoise-steps/s", "cores": cores, "kind": "port",
            "sample": f"1 warm-up + {c2['timed_chunks']} timed full 10-step DDIM chunks (median) of the config-2 model at B=128 (GCDenoiser.forward + DDIM update per step), fp32, "
                      f"oracle/mode_oracle.py with torch.set_num_threads({cores}); cpu: {model}",
            "c1_b8": legs["c1"], "c2_b128": c2}


def prealloc_train_state(den, device, world, B=B_PER_GPU):
    """Allocate the training step's device state - both Adam moments (5.5 GB), the gradient arena, the activation stash, the backward workspaces - BEFORE
    the inference legs run, with one training step at lr = 0 (weights, bf16 shadow: bit-identical afterwards; moments and step count are reset).

    Why (profiles/r06_train_gap.txt; VERDICT r05 #1a): the same training leg measured 10.3-10.5 ms per step in a fresh process and 11.0-11.5 ms at the end
    of the default run.  Bisected on one box: not clocks, not the MFMA burn, not the caching allocator (empty_cache() changes nothing) - the step is slow
    exactly when its ~14 GB of state is FIRST allocated after the sampler / per-kernel / extra legs have churned device memory, and fast (10.2-10.3 ms) after
    the very same legs when the state was allocated at process start.  A training job allocates its state once at start-up, so that is what the bench does.
    Returns the optimizer object for train_leg(opt=...)."""
    import math
    from mode_diffusion_policy_amd.optim import FusedAdamW
    from mode_diffusion_policy_amd.utils import rand_log_logistic
    m = den.inner_model
    was_training = den.training
    den.train()
    fuse = world == 1 and os.environ.get("MODE_FUSE_EXPERT_STEP", "1") == "1" and m.engine.compute_dtype == "bf16"
    opt = FusedAdamW(m, lr=0.0, betas=(0.9, 0.95), weight_decay=0.0, fuse_expert_step=fuse)
    g = torch.Generator(device="cpu").manual_seed(99)
    img = torch.randn(B, m.n_img_tokens, m.obs_dim, generator=g).to(device); goal = torch.randn(B, 1, m.goal_dim, generator=g).to(device)
    acts = torch.randn(B, m.action_seq_len, m.action_dim, generator=g).to(device); noise = torch.randn(B, m.action_seq_len, m.action_dim, generator=g).to(device)
    probe = m.engine.arena.flat[:4096].clone()
    sig = rand_log_logistic((B,), loc=math.log(SIGMA_DATA), scale=0.5, min_value=SIGMA_MIN, max_value=SIGMA_MAX, device=device)
    loss, _ = den.loss({"state_images": img}, acts, goal, noise, sig)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(probe, m.engine.arena.flat[:4096]), "the lr = 0 allocation step moved the weights"
    opt.reset_state()
    den.train(was_training)
    return opt


def train_leg(den, device, world, rank, dist, steps=10, warmup=3, B=B_PER_GPU, zero1=None, comm_dtype=None, opt=None, fuse=None, local_only=False):
    """BASELINE configs[2]/[3]: the score-matching training step of `den` (fwd + bwd + fused AdamW) on B samples per rank, data parallel over
    `world` ranks - ONE implementation shared by `--mode train`, by the default run's extra legs (N = 1) and by the N > 1 default run, so that a
    SCALE record evidences the gradient exchange.  All ranks must call it together.  Every rank owns its own shard of the synthetic batch; the
    gradient arena is exchanged in flat per-block slices behind the backward's block events (RCCL when `dist` is up).  Default exchange: the plain
    overlapped all-reduce - what the reference's DDP does (mode/training_calvin.py:92-103); `zero1` ("bf16" | "fp32"; or MODE_DP_ZERO1 when the argument
    is None) selects the sharded-optimizer variant instead; MODE_DP_COMM = fp32 | bf16 the wire dtype.  The number of ranks the collective library
    actually connected is checked BEFORE anything is timed.  Timed like the contract says: barrier + synchronize on both sides, MAX over ranks.
    Returns the keys merged into the JSON line."""
    import math
    from mode_diffusion_policy_amd.ddp import ArenaGradReducer
    from mode_diffusion_policy_amd.optim import FusedAdamW
    from mode_diffusion_policy_amd.utils import rand_log_logistic
    m = den.inner_model
    was_training = den.training
    den.train()
    g = torch.Generator(device="cpu").manual_seed(1234 + rank)                 # every rank gets its own shard of the synthetic batch
    A_len, A = m.action_seq_len, m.action_dim
    img = torch.randn(B, m.n_img_tokens, m.obs_dim, generator=g).to(device); goal = torch.randn(B, 1, m.goal_dim, generator=g).to(device)
    acts = torch.randn(B, A_len, A, generator=g).to(device); noise = torch.randn(B, A_len, A, generator=g).to(device)
    # single process: the expert matrices (88 % of the parameters) are updated in the epilogue of their weight-gradient GEMMs (ModeAdamWFuse) - no
    # gradient store / re-read for them and no optimizer pass beside the backward; world > 1 exchanges gradients, so it keeps the two-pass update
    # `fuse=False` at world == 1: the two-pass update every N > 1 rank runs - the anchor a scaling curve divides by (train_twopass_* keys)
    # `local_only`: this rank's step WITHOUT the exchange inside an N > 1 run (every rank on its own: the in-run N = 1 anchor, scaling_vs_twopass_n1)
    if local_only:
        world, dist = 1, None
    want_fuse = world == 1 and os.environ.get("MODE_FUSE_EXPERT_STEP", "1") == "1" and m.engine.compute_dtype == "bf16"
    fuse = want_fuse if fuse is None else (bool(fuse) and want_fuse)
    if opt is None:
        opt = FusedAdamW(m, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05, fuse_expert_step=fuse)   # mode_agent.yaml:24-29, two groups as mode_agent.py:365-384
    else:                                                                      # the optimizer whose state prealloc_train_state() placed at process start
        opt.reset_state()
        opt.set_fuse_expert_step(fuse)
        for gi, grp in enumerate(opt.param_groups):
            grp["lr"], grp["weight_decay"] = 1e-4, (0.05 if gi == 0 else 0.0)
    if os.environ.get("MODE_ADAMW_WS"):                                        # A/B in the PROBE build only (scripts/probe/build_trws_variant.sh; the shipped library ignores the key): 0 = ring kernel, 1 = wave-specialised
        m.engine.lib.mode_set_option(b"adamw_ws", int(os.environ["MODE_ADAMW_WS"]))
    for opt_key in ("train_dn_split", "fuse_swiglu_bwd", "gemm_tr_cfg"):              # A/B of library options inside the training leg: MODE_OPT_<KEY>=<int>
        if os.environ.get("MODE_OPT_" + opt_key.upper()):
            m.engine.lib.mode_set_option(opt_key.encode(), int(os.environ["MODE_OPT_" + opt_key.upper()]))
    if os.environ.get("MODE_ADAMW_BLOCKS"):
        m.engine.lib.mode_set_option(b"adamw_blocks", int(os.environ["MODE_ADAMW_BLOCKS"]))
    # gradient exchange dtype: fp32 like the reference's DDP (default), or MODE_DP_COMM=bf16 = half the bytes on the xGMI links
    comm = torch.bfloat16 if (comm_dtype or os.environ.get("MODE_DP_COMM", "fp32")) == "bf16" else torch.float32
    red = ArenaGradReducer.for_model(m, comm_dtype=comm) if dist is not None else None      # also with ONE rank under RCCL: same code path as N > 1
    # data-parallel step (world > 1): summed all-reduce + full optimizer pass by default (the mode closest to the reference's DDP); ZeRO-1 on request -
    # per block slice reduce-scatter of the gradients, AdamW on this rank's shard, all-gather of the bf16 compute shadow ("fp32": of the fp32 masters)
    z1 = zero1 if zero1 is not None else os.environ.get("MODE_DP_ZERO1", "0")
    ranks = 1
    if dist is not None:                                                       # before any timed or exchanged step: did every rank join the communicator?
        one = torch.ones(1, device=device)
        dist.all_reduce(one)
        ranks = int(round(float(one.item())))
        if ranks != world:
            raise RuntimeError(f"collective library connected {ranks} ranks, WORLD_SIZE is {world}")
    z1 = None if (z1 in ("0", "", "none") or red is None or world == 1) else z1
    if z1 == "bf16" and m.engine.compute_dtype != "bf16":
        z1 = "fp32"
    n_ev = 8 * steps + max(warmup, 1) + 2
    ev_bwd = [torch.cuda.Event(enable_timing=True) for _ in range(n_ev)]
    ev_end = [torch.cuda.Event(enable_timing=True) for _ in range(n_ev)]
    it = [0]
    # the rest of the optimizer pass: overlapped per block with the backward (which then keeps the ring kernels for its other large GEMMs, "bwd_coexec"), or -
    # with the expert matrices out of it, 0.4 ms of HBM time - after the backward, which then runs its big data-gradient GEMM on the persistent kernel
    overlap = os.environ.get("MODE_OPT_OVERLAP", "0" if fuse else "1") == "1"
    # process-wide library option (include/mode_hip.h): per-block optimizer passes / collectives share the CUs with the backward chain -> ring kernels
    m.engine.lib.mode_set_option(b"bwd_coexec", 1 if (overlap and not fuse) else 0)

    def step():
        sig = rand_log_logistic((B,), loc=math.log(SIGMA_DATA), scale=0.5, min_value=SIGMA_MIN, max_value=SIGMA_MAX, device=device)
        loss, _ = den.loss({"state_images": img}, acts, goal, noise, sig)
        loss.backward()
        ev_bwd[it[0]].record()                                                 # the backward chain's last kernel
        opt.step(reducer=red, overlap=overlap, zero1=z1)                       # per block: exchange (RCCL) -> AdamW underneath the remaining backward
        ev_end[it[0]].record()
        it[0] += 1
        return loss
    for _ in range(max(warmup, 1)):
        loss = step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss.detach()).all()
    # Timed blocks of `steps` steps until the two fastest agree within 5 % (at most 8; all listed), the fastest reported.  (Rounds 1-2 saw 2-4x slower
    # blocks in some processes and blamed the box; round 3 found the cause - the training node leaked every step's activation stash, LABNOTES.md section 4
    # "Round 3" - and with the leak fixed 800 consecutive steps stay within 0.5 %.  The block list stays in the line as the evidence.)
    blocks = []
    for _ in range(8):
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        el = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el], device=device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        blocks.append(el)
        srt = sorted(blocks)
        if len(blocks) >= 3 and srt[1] <= 1.05 * srt[0]:                       # >= 3 blocks, and the two fastest agree on the steady state (every rank sees the same MAX-reduced times)
            break
    best = min(range(len(blocks)), key=lambda i: blocks[i])
    elapsed = blocks[best]
    ev_lo = it[0] - (len(blocks) - best) * steps                               # events of the reported block
    if z1:
        opt.gather_state(red)                                                  # leave exact masters / moments on every rank
    m.engine.lib.mode_set_option(b"bwd_coexec", 0)
    den.train(was_training)
    ms = elapsed / steps * 1e3
    d = m.engine.dims
    fl = 3.0 * flops_per_denoise_step(B, L=d.L, D=d.D, H=d.H, T=d.T, E=d.E, k=d.k, O=d.O, G=d.G, A=d.A_dim, A_len=d.A_len)   # fwd + bwd ~ 3x forward
    backend = dist.get_backend() if dist is not None else None
    # How to read a SCALE curve: the bytes one rank puts on its xGMI links per step for this leg (ring algorithms: all-reduce 2 (N-1)/N x payload,
    # reduce-scatter and all-gather (N-1)/N each) and the time they need at ~300 GB/s of ring bandwidth per GPU (7 links x ~153 GB/s peak; rings are
    # per-link bound).  A leg can only scale if dp_budget_ms fits under the backward (~2/3 of the single-GPU step): the fp32 all-reduce of 686 M
    # parameters does NOT at N = 8 (4.8 GB, ~16 ms against an ~11.7-ms step); the bf16 wire and the ZeRO-1 legs (2.4 GB, ~8 ms) are the ones that can.
    n_par = sum(p_.numel() for p_ in m.parameters())
    gb = 2 if comm == torch.bfloat16 else 4
    frac = (world - 1) / world if world > 1 else 0.0
    if z1:
        wire = frac * n_par * gb + frac * n_par * (2 if z1 == "bf16" else 4)      # reduce-scatter of the gradients + all-gather of the updated weights
    else:
        wire = 2.0 * frac * n_par * gb
    exposed = round(sum(ev_bwd[i].elapsed_time(ev_end[i]) for i in range(ev_lo, ev_lo + steps)) / steps, 3)
    return {"fused_expert_step": bool(fuse), "fused_side_stream": bool(fuse and opt.fused_side_stream), "optimizer_overlap": bool(overlap), "dp_wire_gb": round(wire / 1e9, 3), "dp_budget_ms": round(wire / 300e9 * 1e3, 2), "exposed_exchange_ms": exposed,
            "train_ms_per_step": round(ms, 3), "train_samples_per_s": round(world * B / (ms * 1e-3), 1), "train_global_batch": B * world,
            "train_mfma_frac": round(fl / (ms * 1e-3) / (MFMA_BF16_PEAK_TFLOPS * 1e12), 4), "train_tflops_per_gpu": round(fl / (ms * 1e-3) / 1e12, 1),
            "dp_mode": ("zero1:" + z1) if z1 else ("allreduce" if (red is not None and world > 1) else "single"),
            "dp_comm_dtype": "bf16" if comm == torch.bfloat16 else "fp32",
            # what is NOT hidden behind the backward: gradient exchange + optimizer (+ weight all-gather) still running after its last kernel
            "exposed_exchange_and_optimizer_ms": exposed,
            "train_ms_per_step_blocks": [round(b / steps * 1e3, 3) for b in blocks],
            "rccl_ranks": ranks if backend == "nccl" else None, "dp_backend": backend, "dp_ranks": ranks, "train_steps": steps}


def agent_replan_measure(den, device):
    """The rollout as the AGENT runs it (mode_agent.py:584-637): raw 224 x 224 frames of two cameras -> two FiLM-ResNet-50s (eval, autocast bf16) -> 10-step DDIM
    chunk; replanning call latency with the encoders captured in a hipGraph (GraphedVisualEncoder) and eager, for 1 and 32 environments."""
    from mode_diffusion_policy_amd import rollout as RO
    from mode_diffusion_policy_amd.perceptual_encoders import FiLMResNet50Policy, embed_visual_obs
    agent_extra = {}
    enc_s, enc_g = FiLMResNet50Policy(512).to(device).eval(), FiLMResNet50Policy(512).to(device).eval()
    for key, nb in (("agent_b1", 1), ("agent_b32", 32)):
        gen = torch.Generator().manual_seed(3)
        frames = {"rgb_obs": {"rgb_static": torch.randn(nb, 1, 3, 224, 224, generator=gen).to(device),
                              "rgb_gripper": torch.randn(nb, 1, 3, 224, 224, generator=gen).to(device)}}
        lg = torch.randn(nb, 512, generator=gen).to(device)
        pol = RO.ChunkedRolloutPolicy(den, multistep=1, static_resnet=enc_s, gripper_resnet=enc_g)
        plain = RO.ChunkedRolloutPolicy(den, multistep=1)

        def eager_call():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                tok = embed_visual_obs(enc_s, enc_g, frames["rgb_obs"]["rgb_static"], frames["rgb_obs"]["rgb_gripper"], lg)
            return plain.step({"state_images": tok["state_images"].float()}, lg)
        for name, fn in (("graphed", lambda: pol.step(frames, lg)), ("eager", eager_call)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            agent_extra[f"{key}_replan_ms_{name}_encoders"] = round((time.perf_counter() - t1) / 20 * 1e3, 3)
    return agent_extra


def extra_measurements(M, den, device):
    """Driver-timed numbers of the other inference configurations, in the same process as the headline run (rank 0, N = 1 only):
    configs[4] rollout (B=32 environments) and the reference's real rollout case B=1.  (The training leg is `train_leg`, run by every N.)"""
    import math
    out = {}
    sig = M.get_sigmas_exponential(N_SAMPLING_STEPS, SIGMA_MIN, SIGMA_MAX).to(device)
    m = den.inner_model
    weight_bytes = 767e6                                             # bf16 weights touched per denoise step under uniform sigma
    for key, batch in (("rollout", 32), ("b1", 1)):
        img, goal, x0 = synthetic_inputs(device, batch)
        state = {"state_images": img}
        if key == "rollout":                                         # MoDEAgent's inference setup: routing cached per noise level (mode_agent.py:639-644)
            for s_ in sig[:-1]:
                m.precompute_experts_for_inference(s_)
        for _ in range(3):
            out_x = M.sample_ddim(den, state, x0, goal, sig, disable=True)
        torch.cuda.synchronize()
        assert torch.isfinite(out_x).all()
        n = 30
        t0 = time.perf_counter()
        for _ in range(n):
            M.sample_ddim(den, state, x0, goal, sig, disable=True)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / n * 1e3
        out[f"{key}_ms_per_chunk"] = round(ms, 3)
        out[f"{key}_hbm_frac"] = round(weight_bytes * N_SAMPLING_STEPS / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)
        out[f"{key}_mfma_frac"] = round(flops_per_denoise_step(batch) * N_SAMPLING_STEPS / (ms * 1e-3) / (MFMA_BF16_PEAK_TFLOPS * 1e12), 4)
        if key == "rollout":
            out["rollout_action_chunks_per_s"] = round(batch / (ms * 1e-3), 1)
    # the fused BatchNorm + FiLM + residual + ReLU pass of the FiLM-ResNet encoders at a ResNet-50 stage-1 shape
    # (B = 128 frames, 256 channels, 56 x 56, bf16): algorithmic bytes = x + residual read, y written (forward); + dy read, dx / d residual written
    # and x / residual / dy read a second time by the reduction pass (backward)
    from mode_diffusion_policy_amd import perceptual_encoders as PE
    xe = torch.randn(128, 256, 56, 56, device=device).to(torch.bfloat16); re_ = torch.randn_like(xe)
    bn = torch.nn.BatchNorm2d(256).to(device).eval()
    gq, bq = torch.randn(128, 256, device=device) * 0.1, torch.randn(128, 256, device=device) * 0.1
    x1 = xe.clone().requires_grad_(True); r1 = re_.clone().requires_grad_(True)
    for _ in range(3):
        ye = PE.bn_film_act(x1, bn, relu=True, residual=r1, post_film=(gq, bq))
        ye.backward(xe)
    torch.cuda.synchronize()
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    nrep = 20
    e0.record()
    for _ in range(nrep):
        with torch.no_grad():
            PE.bn_film_act(xe, bn, relu=True, residual=re_, post_film=(gq, bq))
    e1.record()
    for _ in range(nrep):
        ye = PE.bn_film_act(x1, bn, relu=True, residual=r1, post_film=(gq, bq))
        ye.backward(xe)
    e2.record(); torch.cuda.synchronize()
    nbytes = xe.numel() * 2
    fwd_us = e0.elapsed_time(e1) * 1e3 / nrep
    fb_us = e1.elapsed_time(e2) * 1e3 / nrep
    out["encoder_bn_film_fwd_us"] = round(fwd_us, 1)
    out["encoder_bn_film_fwd_hbm_frac"] = round(3 * nbytes / (fwd_us * 1e-6) / (HBM_PEAK_GBS * 1e9), 4)
    out["encoder_bn_film_fwd_bwd_us"] = round(fb_us, 1)
    out["encoder_bn_film_fwd_bwd_hbm_frac"] = round((3 + 8) * nbytes / (fb_us * 1e-6) / (HBM_PEAK_GBS * 1e9), 4)
    del xe, re_, x1, r1, ye
    # the non-DDIM samplers of MoDEAgent.sample_loop (mode_agent.py:798-839): host recurrences around ONE hipGraph replay per denoiser call
    # (sigma is a device scalar of the captured chain: MoDeDiT.denoise_graphed) - B = 128, 10 model evaluations per chunk
    from mode_diffusion_policy_amd import samplers as S
    img, goal, x0 = synthetic_inputs(device, B_PER_GPU)
    for name, fn in (("euler", S.sample_euler), ("dpmpp_2m", S.sample_dpmpp_2m)):
        for _ in range(2):
            xs = fn(den, {"state_images": img}, x0, goal, sig, disable=True)
        torch.cuda.synchronize()
        assert torch.isfinite(xs).all()
        n = 10
        t0 = time.perf_counter()
        for _ in range(n):
            fn(den, {"state_images": img}, x0, goal, sig, disable=True)
        torch.cuda.synchronize()
        out[f"sampler_{name}_denoise_steps_per_s"] = round(n * N_SAMPLING_STEPS / (time.perf_counter() - t0), 1)
    # the same samplers through the rollout policy (MoDEAgent.denoise_actions' path): the WHOLE sampler call as one hipGraph replay
    from mode_diffusion_policy_amd import rollout as RO
    for name in ("euler", "dpmpp_2m", "heun"):               # heun: 2 n - 1 = 19 denoiser evaluations per chunk (two-stage solver on the fused chain)
        evals = 2 * N_SAMPLING_STEPS - 1 if name == "heun" else N_SAMPLING_STEPS
        for key, nb in ((f"sampler_{name}_policy_" + ("denoiser_evals_per_s" if name == "heun" else "denoise_steps_per_s"), B_PER_GPU),
                        (f"sampler_{name}_policy_b1_ms_per_chunk", 1)):
            im, gl, _ = synthetic_inputs(device, nb)
            pol = RO.ChunkedRolloutPolicy(den, sampler_type=name, num_sampling_steps=N_SAMPLING_STEPS, sigma_min=SIGMA_MIN, sigma_max=SIGMA_MAX, multistep=1)
            for _ in range(3):
                pol.denoise_actions({"state_images": im}, gl)
            torch.cuda.synchronize()
            n = 10
            t0 = time.perf_counter()
            for _ in range(n):
                pol.denoise_actions({"state_images": im}, gl)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            out[key] = round(n * evals / el, 1) if nb > 1 else round(el / n * 1e3, 3)
    return out


def train_bench(args, world, rank, device, dist):
    """BASELINE configs 3/4: score-matching training step of the full model, B=128 per GPU (global 128*N), AdamW included,
    gradient arena exchanged over ranks in flat slices (RCCL), 1/world folded into the fused AdamW pass."""
    M, den = build_model(device, args.dtype)
    t = train_leg(den, device, world, rank, dist, steps=args.steps, warmup=args.warmup)
    if rank == 0:
        res = {"metric": "train-samples/sec (score-matching step, B=128 per GPU, AdamW)", "value": t["train_samples_per_s"],
               "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": t["train_ms_per_step"],
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
               "config": {"workload": "configs[2]/[3]: score-matching training step of the full MoDE denoiser (12 layers, d=1024, 4 experts top-2), "
                                      "B=128 per GPU, log-logistic sigma, multinomial routing, dropouts on, fused AdamW, router unfrozen",
                          "global_batch": B_PER_GPU * world, "parallelism": f"dp{world} {t['dp_mode']} ({t['dp_comm_dtype']} gradient exchange)"}}
        res.update(t)
        print(json.dumps(res), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def agent_bench(args, world, rank, device, dist):
    """SURVEY section 8(f) rank 1 end to end: the reference AGENT's training step - two FiLM-ResNet-50 encoders (static + gripper camera, 224 x 224,
    conditioned on the latent goal, mode_agent.py:548-567, conf/model/mode_agent.yaml resnet_type '50', calvin_transforms.yaml) feeding the denoiser's
    score-matching loss, everything under torch.autocast(bfloat16) like the reference's trainer (conf/config_calvin.yaml:37), backward THROUGH the
    denoiser into both encoders, AdamW on all of it (fused arena AdamW for the denoiser, torch AdamW for the encoders).  Convolutions: the library's own GEMM /
    implicit-GEMM kernels (the 3-channel stem: MIOpen); BatchNorm / FiLM / ReLU / residual between them: the fused HIP pass (csrc/encoder_ops.hip).  One rank."""
    M, den = build_model(device, args.dtype)
    res = agent_step_measure(den, device, args.agent_batch, args.steps, args.warmup, bool(args.miopen_benchmark))
    print(json.dumps(res), flush=True)


def agent_step_measure(den, device, B, steps, warmup, miopen_benchmark=False, opt=None):
    """The measurement behind `--mode agent` (also a leg of the default run, on the headline's model): returns the JSON record."""
    import math
    from mode_diffusion_policy_amd.optim import FusedAdamW
    from mode_diffusion_policy_amd.perceptual_encoders import FiLMResNet50Policy, embed_visual_obs
    from mode_diffusion_policy_amd.utils import rand_log_logistic
    torch.backends.cudnn.benchmark = bool(miopen_benchmark)
    m = den.inner_model
    was_training = den.training
    den.train()
    torch.manual_seed(0)
    enc_s, enc_g = FiLMResNet50Policy(512).to(device).train(), FiLMResNet50Policy(512).to(device).train()
    for enc in (enc_s, enc_g):                                                 # the reference zero-initialises FiLM: give the modulation something to do
        for n_, p_ in enc.named_parameters():
            if n_.startswith("film"):
                torch.nn.init.normal_(p_, std=0.02)
    g = torch.Generator().manual_seed(1)
    rgb_s = torch.randn(B, 1, 3, 224, 224, generator=g).to(device); rgb_g = torch.randn(B, 1, 3, 224, 224, generator=g).to(device)
    goal = torch.randn(B, 1, 512, generator=g).to(device)
    acts = torch.randn(B, 10, 7, generator=g).to(device); noise = torch.randn(B, 10, 7, generator=g).to(device)
    fuse = os.environ.get("MODE_FUSE_EXPERT_STEP", "1") == "1" and m.engine.compute_dtype == "bf16"     # single process: expert matrices updated inside the backward (train_leg)
    if opt is None:
        opt = FusedAdamW(m, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05, fuse_expert_step=fuse)
    else:                                                                      # the default run's start-up optimizer state (prealloc_train_state)
        opt.reset_state(); opt.set_fuse_expert_step(fuse)
        for gi, grp in enumerate(opt.param_groups):
            grp["lr"], grp["weight_decay"] = 1e-4, (0.05 if gi == 0 else 0.0)
    enc_params = list(enc_s.parameters()) + list(enc_g.parameters())
    if os.environ.get("MODE_BENCH_FLAT_ADAMW", "1") == "1":                     # the encoders' 51 M parameters as ONE mode_adamw_step launch (optim.FlatAdamW)
        from mode_diffusion_policy_amd.optim import FlatAdamW
        opt_e = FlatAdamW(enc_params, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05)
    else:
        opt_e = torch.optim.AdamW(enc_params, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05,
                                  **({"fused": True} if os.environ.get("MODE_BENCH_TORCH_FUSED_ADAMW") == "1" else {}))   # (A/B: torch's foreach / fused multi-tensor kernels; the reference uses the default)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    enc_ms = [0.0, 0.0]
    def step(timed=False):
        sig = rand_log_logistic((B,), loc=math.log(0.5), scale=0.5, min_value=1e-3, max_value=80.0, device=device)
        if timed:
            ev[0].record()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            emb = embed_visual_obs(enc_s, enc_g, rgb_s, rgb_g, goal.squeeze(1))
            if timed:
                ev[1].record()
            loss, _ = den.loss(emb, acts, goal, noise, sig)
        loss.backward()
        opt.step(overlap=not fuse)
        opt_e.step()
        opt_e.zero_grad(set_to_none=True)
        return loss
    for _ in range(max(warmup, 2)):                                             # includes MIOpen's per-shape algorithm search
        loss = step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss.detach()).all()
    blocks, host = [], []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(steps):
            step()
        host.append((time.perf_counter() - t0) / steps * 1e3)                    # the loop returned: everything is enqueued
        torch.cuda.synchronize(); blocks.append((time.perf_counter() - t0) / steps * 1e3)
    step(timed=True); torch.cuda.synchronize()
    enc_fwd_ms = ev[0].elapsed_time(ev[1])
    ms = min(blocks)
    n_enc = sum(p_.numel() for e in (enc_s, enc_g) for p_ in e.parameters())
    res = {"metric": "agent-train-samples/sec (2x FiLM-ResNet-50 @224 + MoDE denoiser, B per GPU, AdamW)", "value": round(B / (ms * 1e-3), 1), "unit": "samples/s",
           "n_gpus": 1, "steps": steps, "warmup": warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "bf16 (torch.autocast for the encoders, bf16 MFMA chain for the denoiser)", "data": "synthetic",
           "config": {"workload": "SURVEY 8(f)-1: MoDEAgent training step - embed_visual_obs (2 x FiLMResNet50Policy, 224 x 224 RGB, latent-goal FiLM) -> "
                                  "GCDenoiser.loss (12 layers, d=1024, 4 experts top-2) -> backward through both -> AdamW", "global_batch": B,
                      "parallelism": "single GPU"},
           "agent_ms_per_step_blocks": [round(b, 3) for b in blocks], "host_enqueue_ms_per_step": round(min(host), 3), "encoders_forward_ms": round(enc_fwd_ms, 3), "encoder_params": n_enc, "fused_expert_step": bool(fuse),
           "encoder_optimizer": type(opt_e).__name__,
           "peak_memory_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), "miopen_benchmark": bool(miopen_benchmark)}
    den.train(was_training)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--full", action="store_true", help="sample / rollout: after the headline, run every other measurement of this file "
                    "(roofline, per-kernel breakdown, rollout / B=1 / sampler / encoder legs, training and agent legs, CPU baseline)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="skip the training state's start-up allocation and, with --full, the sustained MFMA "
                    "rate, the per-kernel breakdown and the train / rollout / B=1 / agent legs")
    ap.add_argument("--miopen-benchmark", action="store_true", help="--mode agent: torch.backends.cudnn.benchmark = True (MIOpen's exhaustive per-shape search; the "
                    "reference's trainer runs with benchmark=False, mode/training_calvin.py:96)")
    ap.add_argument("--agent-batch", type=int, default=64, help="--mode agent: samples per step (the reference's config_calvin.yaml batch_size is 64 per GPU)")
    ap.add_argument("--mode", default="sample", choices=["sample", "train", "rollout", "agent"],
                    help="sample (default, BASELINE metric): 10-step DDIM chunks at B=128; train: configs[2]/[3] score-matching steps "
                         "(fwd+bwd+AdamW, DP all-reduce); rollout: configs[4], B=32 environments, router pre-cached per noise level")
    ap.add_argument("--dump-outputs", metavar="DIR", help="sample / rollout: write the action chunk the LAST timed step returned to DIR/actions.npy "
                    "(float32, rank 0), so that two builds can be compared output for output on the same seeded inputs")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.mode not in ("sample", "rollout"):
        ap.error("--dump-outputs is implemented for --mode sample and rollout")
    extras = args.full and not args.no_extras

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # MODE_BENCH_SHARE_GPU=1 + MODE_BENCH_BACKEND=gloo: every rank on cuda:0 with a host-side collective - the world-2 dry run of this whole file on a
    # ONE-GPU box (tests/test_gpu_train_dropin.py; two RCCL ranks cannot share a device).  Never set by the driver.
    share = os.environ.get("MODE_BENCH_SHARE_GPU", "0") == "1"
    backend = os.environ.get("MODE_BENCH_BACKEND", "nccl")
    device = torch.device("cuda", 0 if share else local)
    torch.cuda.set_device(device)
    dist = None
    if "RANK" in os.environ and "MASTER_ADDR" in os.environ:       # launched by torch.distributed.run (also with one rank)
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # RCCL prints a version banner to STDOUT when the communicator comes up; keep stdout = the one JSON line of the contract
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=device)
            else:
                dist.init_process_group(backend)
            dist.barrier()
            torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)

    if args.mode == "train":
        return train_bench(args, world, rank, device, dist)
    if args.mode == "agent":
        return agent_bench(args, world, rank, device, dist)
    M, den = build_model(device, args.dtype)
    rollout = args.mode == "rollout"
    # the training leg's device state is allocated NOW, as a training job does at start-up (prealloc_train_state: why); MODE_BENCH_PREALLOC_TRAIN=0 = A/B.
    # Also without --full, where no training leg follows: the headline has always been measured on top of this allocation (0.2 s), and without it
    # the same build reads about 1 % lower (same box, runs alternated: 639.5 vs 645.0 denoise-steps/s over four pairs; a bare 14-GiB torch.empty
    # recovers part of it, an MFMA burn of the same length none - device-memory placement, not clocks)
    train_opt = None
    if not rollout and args.dtype == "bf16" and not args.no_extras and os.environ.get("MODE_BENCH_PREALLOC_TRAIN", "1") == "1":
        train_opt = prealloc_train_state(den, device, world)
    batch = 32 if rollout else B_PER_GPU
    img, goal, x0 = synthetic_inputs(device, batch)
    sig = M.get_sigmas_exponential(N_SAMPLING_STEPS, SIGMA_MIN, SIGMA_MAX).to(device)
    state = {"state_images": img}
    if rollout:                                     # MoDEAgent's inference setup: routing decisions cached per noise level (mode_agent.py:318-341)
        for s_ in sig[:-1]:
            den.inner_model.precompute_experts_for_inference(s_)

    def chunk():
        return M.sample_ddim(den, state, x0, goal, sig, disable=True)

    for _ in range(max(args.warmup, 1)):
        out = chunk()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all(), "non-finite actions"

    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    with PowerSampler(device.index or 0) as psamp:
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = chunk()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "actions.npy"), out.detach().float().cpu().numpy())

    n_gpus = world
    denoise_steps = n_gpus * args.steps * N_SAMPLING_STEPS
    value = denoise_steps / elapsed
    if rollout:
        agent_extra = {}
        if rank == 0 and extras:
            agent_extra = agent_replan_measure(den, device)
        if rank == 0:
            print(json.dumps({
                "metric": "action-chunks/sec (B=32 envs, 10-step DDIM per chunk)", "value": round(n_gpus * args.steps * batch / elapsed, 1),
                "unit": "action-chunks/s", "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": args.dtype, "data": "synthetic",
                "config": {"workload": "configs[4]: inference rollout, 32 environments x one 10-action chunk x 10 denoise steps per call, hipGraph-captured "
                                       "sampler, routing pre-cached per noise level, full MoDE denoiser", "global_batch": batch * n_gpus,
                           "parallelism": f"replicas x{n_gpus} (no data-path collective)"},
                "latency_ms_per_chunk_call": round(elapsed / args.steps * 1e3, 3),
                "e2e_tflops_per_gpu": round(flops_per_denoise_step(batch) * args.steps * N_SAMPLING_STEPS / elapsed / 1e12, 1), **agent_extra}), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    res = {
        **({"dry_run": True, "dry_run_layers": _dry_run_layers()} if _dry_run_layers() else {}),
        "metric": "denoise-steps/sec (B=128, 10-step chunk)", "value": round(value, 2), "unit": "denoise-steps/s", "n_gpus": n_gpus,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": "configs[1]: full MoDE denoiser (12 layers, d=1024, 8 heads, 4 experts top-2, obs 2048, goal 512), "
                               "B=128 per GPU, one step = one 10-step DDIM chunk (sample_ddim o GCDenoiser o MoDeDiT), eval, "
                               "uniform sigma per step, random-init weights",
                   "global_batch": B_PER_GPU * n_gpus, "denoise_steps_per_step": N_SAMPLING_STEPS,
                   "parallelism": f"replicas x{n_gpus} (no data-path collective)"},
        "action_chunks_per_s": round(value * B_PER_GPU / N_SAMPLING_STEPS, 1),
        "ms_per_denoise_step": round(elapsed / (args.steps * N_SAMPLING_STEPS) * 1e3, 4),
    }
    if rank == 0:
        fl = flops_per_denoise_step(B_PER_GPU)
        res["e2e_tflops_per_gpu"] = round(fl * args.steps * N_SAMPLING_STEPS / elapsed / 1e12, 1)
        res["e2e_mfma_frac"] = round(res["e2e_tflops_per_gpu"] / MFMA_BF16_PEAK_TFLOPS, 4)
        # the same time against the FLOPs the timed region executes (router / sigma-embedding hoisted per schedule, observation embeddings per chunk)
        res["e2e_mfma_frac_executed"] = round(flops_executed_per_chunk(B_PER_GPU) * args.steps / elapsed / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4)
        res["power"] = psamp.summary()                       # rank 0's socket over the timed region
        if args.full and args.dtype == "bf16":
            res["roofline"] = dominant_kernel_roofline(den, device)
            if n_gpus == 1 and extras:
                sp = sustained_mfma_peak(device)
                res["roofline"]["sustained_mfma_peak"] = sp           # context for `frac`: `peak` stays the datasheet figure
                res["roofline"]["frac_of_sustained_peak"] = round(res["roofline"]["achieved"] / sp["tflops"], 4) if sp["tflops"] else None
            if n_gpus == 1 and extras:
                res["layer_kernels"] = layer_kernel_breakdown(den, device)
                res.update(extra_measurements(M, den, device))
    # configs[2]/[3] in the same invocation: the data-parallel training step (ALL ranks: it holds the path's one collective).  The headline above
    # is replicas of the sampler (no collective); this leg is what a multi-GPU record can show the gradient exchange with.  Last of the GPU legs:
    # it updates the weights.  Order at N > 1: (1) the plain overlapped all-reduce - what the reference's DDP does (mode/training_calvin.py:92-103) -
    # under the train_* keys; (2) only after that has come back, the ZeRO-1 variant under zero1_* keys.  Each leg runs under its own watchdog: the
    # multi-rank RCCL path has only ever run with ONE rank on RCCL and with two on gloo (tests/test_gpu_train_dropin.py), so if a leg raises or does
    # not come back, everything measured before it is still printed - with the reason.  Progress goes to stderr as each leg completes.
    train_failed = False
    if rank == 0:
        print(f"[bench] headline done: {res['value']} {res['unit']} on {n_gpus} GPU(s)", file=sys.stderr, flush=True)
    if args.dtype == "bf16" and extras:
        forced = os.environ.get("MODE_DP_ZERO1")                                # an explicit choice runs as the one and only leg (A/B runs)
        legs = [("train", forced if forced is not None else "0", None)]
        if world > 1 and forced is None and os.environ.get("MODE_BENCH_ZERO1_LEG", "1") == "1":
            legs.append(("zero1", "bf16", None))
        if world > 1 and forced is None and os.environ.get("MODE_BENCH_BF16WIRE_LEG", "1") == "1":
            legs.append(("bf16wire", "0", "bf16"))       # the plain all-reduce again with bf16 on the links (torch's bf16_compress_hook): half the bytes, summed in bf16
        # The anchor of a scaling curve: the world = 1 "train" leg runs the fused-epilogue optimizer, a single-process mode - every N > 1 rank
        # runs the TWO-PASS update.  So N = 1 also prints the two-pass step (train_twopass_*: the number an N > 1 line divides by), and every N > 1 run times
        # that same step on each rank WITHOUT the exchange (train_twopass_local_*) and prints scaling_vs_twopass_n1 = N x local / leg for each leg.
        # The >= 6x claim at N = 8 is the bf16wire leg's (the only leg whose wire time fits under the step).
        if forced is None and os.environ.get("MODE_BENCH_TWOPASS_LEG", "1") == "1":
            legs.append(("twopass", "0", None))
        limit = float(os.environ.get("MODE_TRAIN_LEG_TIMEOUT", "240"))
        for leg, z1, wire in legs:
            wd = None
            if world > 1:
                import threading

                def _bail(leg=leg):
                    if rank == 0:
                        res[f"{leg}_leg_error"] = f"no result after {limit:.0f} s (collective did not complete): reported without this leg"
                        print(json.dumps(res), flush=True)
                    os._exit(0)
                wd = threading.Timer(limit, _bail)
                wd.daemon = True
                wd.start()
            try:
                nst = int(os.environ.get("MODE_BENCH_TRAIN_STEPS", "10"))
                if leg == "twopass":
                    out = train_leg(den, device, world, rank, dist, steps=nst, opt=train_opt, fuse=False, local_only=True)
                    if world > 1:                                               # every rank ran alone: MAX over ranks, like every other time of this file
                        t = torch.tensor([out["train_ms_per_step"]], device=device, dtype=torch.float64)
                        dist.all_reduce(t, op=dist.ReduceOp.MAX)
                        out["train_ms_per_step"] = round(float(t.item()), 3)
                    pre = "train_twopass_" if world == 1 else "train_twopass_local_"
                    res.update({pre + "ms_per_step": out["train_ms_per_step"], pre + "ms_per_step_blocks": out["train_ms_per_step_blocks"],
                                pre + "samples_per_s": round(B_PER_GPU / (out["train_ms_per_step"] * 1e-3), 1), pre + "optimizer_overlap": out["optimizer_overlap"],
                                pre + "what": "the two-pass AdamW step (gradients stored, per-block optimizer pass beside the backward) - the code every N > 1 rank runs"
                                              + ("" if world == 1 else ", here on each rank WITHOUT the gradient exchange (MAX over ranks)")})
                    if world > 1:
                        for lg in ("train", "zero1", "bf16wire"):
                            k = "train_ms_per_step" if lg == "train" else f"{lg}_ms_per_step"
                            if k in res:
                                res[("" if lg == "train" else lg + "_") + "scaling_vs_twopass_n1"] = round(world * out["train_ms_per_step"] / res[k], 3)
                        res["scaling_claim_leg"] = "bf16wire"
                else:
                    out = train_leg(den, device, world, rank, dist, zero1=z1, comm_dtype=wire, steps=nst, opt=train_opt)
                    if leg == "train":
                        res.update(out)
                    else:                                                       # further sets of keys, after the headline and the all-reduce leg
                        res.update({(f"{leg}_" + k[len("train_"):] if k.startswith("train_") else f"{leg}_" + k): v for k, v in out.items()})
                if rank == 0:
                    print(f"[bench] {leg} leg done: {out['train_ms_per_step']} ms/step, {out['train_samples_per_s']} samples/s, mode {out['dp_mode']}, "
                          f"{out['dp_ranks']} rank(s) on {out['dp_backend']}", file=sys.stderr, flush=True)
            except Exception as e:                                              # noqa: BLE001
                if world == 1:
                    raise
                train_failed = True
                res[f"{leg}_leg_error"] = repr(e)[:400]
            finally:
                if wd is not None:
                    wd.cancel()
            if train_failed:
                break
    # the path's neighbours, driver-timed in the same process (N = 1 only; after everything above, each in its own try: the headline and the
    # training leg are never at stake) - the replanning call as the agent makes it (cameras -> two FiLM-ResNet-50s -> 10-step chunk) and the agent's training step
    if rank == 0 and n_gpus == 1 and args.dtype == "bf16" and extras and _dry_run_layers() == 0 and not train_failed:
        try:
            res.update(agent_replan_measure(den, device))
        except Exception as e:                                                  # noqa: BLE001
            res["agent_replan_error"] = repr(e)[:300]
        try:
            # a clean caching allocator for the host-bound agent step: behind the training legs its free lists are long and fragmented, and the ~3 000
            # allocator calls of one encoder forward + backward get slower (same box: 27.8 ms per step without the flush, 25.1 with it)
            import gc
            gc.collect(); torch.cuda.empty_cache()
            a = agent_step_measure(den, device, 64, 5, 2, opt=train_opt)
            res.update({"agent_train_ms_per_step": a["ms_per_step"], "agent_train_samples_per_s": a["value"], "agent_train_batch": 64,
                        "agent_train_host_enqueue_ms": a["host_enqueue_ms_per_step"]})
        except Exception as e:                                                  # noqa: BLE001
            res["agent_train_error"] = repr(e)[:300]
    if rank == 0:
        if n_gpus == 1 and args.full and not args.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline()
        print(json.dumps(res), flush=True)
    if train_failed:                                                        # the other ranks may be stuck in a collective: no final barrier
        sys.stdout.flush()
        os._exit(0)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
