"""numpy restatement of the bf16-moment AdamW step's rounding (include/mode_hip.h, "AdamW with bf16 moments"): the per-element hash, the stochastic
rounding fp32 -> bf16, and the expected outputs of one mode_adamw_step_lp launch.  No device, no torch: everything is uint32 / uint64 arithmetic."""
import functools

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
EXP = np.uint32(0x7F800000)
BF16_MAX_BITS = 0x7F7F                                                     # largest finite bf16 (0x7f7f0000 as fp32 bits)


def lowbias32(x):
    """hash_u32 of csrc/mode_common.h on a uint32 array (arithmetic modulo 2^32 carried out in uint64)."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def stream_seed(seed, stream):
    """mode_stream_seed of csrc/mode_common.h."""
    x = (int(seed) & 0xFFFFFFFF) ^ ((0x9E3779B9 * ((int(stream) + 1) & 0xFFFFFFFF)) & 0xFFFFFFFF)
    return int(lowbias32(np.array([x], dtype=np.uint64))[0])


def round_hash(round_seed, step, idx):
    """r of every element index in `idx` (any integer array; 64-bit indices allowed): a function of (round_seed, step, index) only."""
    idx = np.asarray(idx, dtype=np.uint64)
    key = np.uint64(stream_seed(round_seed, step))
    inner = lowbias32((idx & M32) ^ key).astype(np.uint64)
    return lowbias32((inner + (idx >> np.uint64(32)) * np.uint64(0x9E3779B9)) & M32)


def sr_bf16(u, r16):
    """Stochastic rounding of fp32 bits `u` (uint32 array) with the 16-bit fields `r16` to bf16 bits (uint16 array)."""
    u = np.asarray(u, dtype=np.uint32)
    r16 = np.asarray(r16, dtype=np.uint32)
    assert int(r16.max(initial=0)) <= 0xFFFF
    special = (u & EXP) == EXP
    nan = special & ((u & np.uint32(0x007FFFFF)) != 0)
    t = (u.astype(np.uint64) + r16.astype(np.uint64)).astype(np.uint64)    # cannot carry out of 32 bits for a non-special u: at most 0xff7fffff + 0xffff
    t = np.where((t & np.uint64(0x7F800000)) == np.uint64(0x7F800000), u.astype(np.uint64), t)
    out = np.where(special, u.astype(np.uint64) >> np.uint64(16), t >> np.uint64(16))
    out = np.where(nan, out | np.uint64(0x40), out)
    return (out & np.uint64(0xFFFF)).astype(np.uint16)


def rne_bf16(u):
    """Round-to-nearest-even of finite fp32 bits to bf16 bits (what a plain cast does): the scheme this feature does NOT use."""
    u = np.asarray(u, dtype=np.uint32).astype(np.uint64)
    return (((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint16)


def expand(b):
    """bf16 bits (uint16 array) -> the fp32 values they denote, exactly."""
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def round_moments(m32, v32, round_seed, step, elem_base=0):
    """Stored bf16 bits of the unrounded fp32 moments `m32`, `v32` of one launch whose first element is element `elem_base` of the moment buffer."""
    m32, v32 = np.asarray(m32, dtype=np.float32).reshape(-1), np.asarray(v32, dtype=np.float32).reshape(-1)
    r = round_hash(round_seed, step, np.arange(m32.size, dtype=np.uint64) + np.uint64(elem_base))
    return sr_bf16(f32_bits(m32), r & np.uint32(0xFFFF)), sr_bf16(f32_bits(v32), r >> np.uint32(16))


def expected_step(fp32_out, round_seed, step, elem_base=0):
    """Expected buffers of one mode_adamw_step_lp launch from the outputs of the fp32 kernel (mode_adamw_step, same hyper-parameters and scale) run
    on the EXPANDED bf16 moments: `fp32_out` maps 'p', 'lp', 'ema' (bit patterns the bf16-moment launch must reproduce unchanged - the weights never
    see a rounded moment) and 'm', 'v' (float32 arrays: this step's unrounded moments).  Returns the same dict with 'm' / 'v' as stored bf16 bits."""
    out = dict(fp32_out)
    out["m"], out["v"] = round_moments(fp32_out["m"], fp32_out["v"], round_seed, step, elem_base)
    return out


def decay_inputs(n=65536, seed=0):
    """Log-normal second moments, rounded to bf16 (RNE) so that the optimizer's buffer can hold them: (bf16 bits, their fp32 values)."""
    rng = np.random.default_rng(seed)
    v0 = np.exp(rng.normal(-9.0, 2.0, n)).astype(np.float32)
    b = rne_bf16(f32_bits(v0))
    return b, expand(b)


@functools.lru_cache(maxsize=None)
def decay_case(n=65536, beta2=0.999, steps=200, round_seed=0):
    """The decay experiment both test files share, computed once: (initial bf16 bits, their fp32 values, bf16 bits after `steps` steps)."""
    b0, v0 = decay_inputs(n)
    out = decay_reference(b0, beta2, steps, round_seed)
    for a in (b0, v0, out):
        a.setflags(write=False)
    return b0, v0, out


def decay_reference(b0, beta2, steps, round_seed, elem_base=0, stochastic=True):
    """v <- v * beta2 (g = 0: the kernel's fma(v, b2, 0 * 0) is the fp32 product) for `steps` steps over bf16 storage; returns the final bf16 bits."""
    b = np.asarray(b0, dtype=np.uint16).copy()
    b2 = np.float32(beta2)
    idx = np.arange(b.size, dtype=np.uint64) + np.uint64(elem_base)
    for step in range(1, steps + 1):
        v = expand(b) * b2                                                 # one fp32 multiply, round-to-nearest: what the device computes
        if stochastic:
            b = sr_bf16(f32_bits(v), round_hash(round_seed, step, idx) >> np.uint32(16))
        else:
            b = rne_bf16(f32_bits(v))
    return b
