"""References for the warm-started replans of rollout.VectorEnvPolicy (tests/test_vector_env_warm.py, tests/test_gpu_vector_env_warm.py): the
environment noise stream of include/mode_hip.h and the warm-start latent formula, restated in numpy fp64."""
import numpy as np

from oracle import mode_oracle as O


def np_noise(seed, draw, n_el):
    """include/mode_hip.h's stream, restated: the hash in numpy uint32 (oracle's lowbias32), Box-Muller in float64."""
    k = np.uint32(O.stream_seed(seed, draw))                        # mode_stream_seed(seed, draw)
    e = np.arange(n_el, dtype=np.uint32)
    h1, h2 = O._lowbias32(k ^ (np.uint32(2) * e)), O._lowbias32(k ^ (np.uint32(2) * e + np.uint32(1)))
    u1 = ((h1 >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (h2 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def shift_hold_index(W, shift):
    """Row of the previous plan that row w of the warm latent starts from: the plan advanced by ``shift``, its last row held."""
    return np.minimum(np.arange(W) + shift, W - 1)


def warm_latents(plan, seed, draw, shift, sigma_start):
    """x0[w, a] = plan[min(w + shift, W - 1), a] + sigma_start * z[w * A + a] in fp64, sigma_start taken as the fp32 value the kernel receives.
    Returns (x0, z), both [W, A]."""
    plan = np.asarray(plan, dtype=np.float64)
    W, A = plan.shape
    z = np_noise(seed, draw, W * A).reshape(W, A)
    return plan[shift_hold_index(W, shift)] + float(np.float32(sigma_start)) * z, z
