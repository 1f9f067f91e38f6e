"""Size contract of the HIP path for long action chunks and wide actions, checked on the host (no GPU): T <= 64 tokens per sample and
action_dim <= 32 are accepted by the inference and training chains; anything beyond, or an inconsistent token count, is refused."""
import ctypes as C

import pytest

from mode_diffusion_policy_amd import _lib as L


def _dims(A_len, A_dim, T, **kw):
    base = dict(D=1024, H=8, L=12, E=4, k=2, T=T, A_len=A_len, A_dim=A_dim, O=2048, G=512, n_img=2, use_noise_token=1,
                router_normalize=1, eps=1e-6)
    base.update(kw)
    return L.ModeDims(**base)


@pytest.mark.parametrize("dtype", [L.MODE_BF16, L.MODE_F32])
@pytest.mark.parametrize("A_len,A_dim,T", [(20, 14, 24), (60, 32, 64), (13, 7, 17), (32, 16, 36)])
def test_long_chunks_and_wide_actions_are_accepted(A_len, A_dim, T, dtype):
    lib = L.load()
    d = _dims(A_len, A_dim, T)
    for B in (1, 2, 128):
        assert lib.mode_dit_workspace_bytes(C.byref(d), B, A_len, dtype) > 0, (B, A_len, A_dim, T)
    sl = L.ModeStashLayout()
    assert lib.mode_dit_train_stash_layout(C.byref(d), 4, dtype, C.byref(sl)) == 0


def test_workspace_grows_with_the_chunk():
    lib = L.load()
    short = lib.mode_dit_workspace_bytes(C.byref(_dims(10, 7, 14)), 128, 10, L.MODE_BF16)
    long_ = lib.mode_dit_workspace_bytes(C.byref(_dims(60, 32, 64)), 128, 60, L.MODE_BF16)
    assert long_ > 4 * short


@pytest.mark.parametrize("A_len,A_dim,T", [(61, 7, 65), (20, 33, 24), (20, 14, 25), (60, 32, 63)])
def test_beyond_the_limits_is_refused(A_len, A_dim, T):
    lib = L.load()
    d = _dims(A_len, A_dim, T)
    assert lib.mode_dit_workspace_bytes(C.byref(d), 8, A_len, L.MODE_BF16) == 0
    sl = L.ModeStashLayout()
    assert lib.mode_dit_train_stash_layout(C.byref(d), 8, L.MODE_BF16, C.byref(sl)) != 0
