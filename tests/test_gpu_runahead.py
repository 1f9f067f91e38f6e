"""Weight run-ahead on the GPU (csrc/runahead.h; ModeGemmDesc::touch0 / touch1; the "weight_runahead" option).  A touch is a load whose data nobody
uses, so the only thing it may change is nothing: every output must be bit-equal with and without a range, equal to another tile geometry, and
no byte outside the output's valid region may change.  The touched buffers are allocated at exactly the range's size and must keep their contents.

  * mode_gemm on the forced ping-pong geometry ("gemm_cfg" 17), SwiGLU, bf16: M = 448, K = 128, N = 128 (ceil(CUs / 2) + 32) value columns and as many
    gate columns, one expert, identity rows - more output tiles than compute units, so a workgroup walks two tiles (the touches go out behind its first
    operand fill and are in flight while the operand stream, the epilogue between the tiles and its stores run); and one K-sliced NONE launch with one
    tile per workgroup (M = 225, K = 512, four slices: eight workgroups).  Ranges of 0, 129 and 2,097,152 bytes, alone and as a pair.
  * the chain: a 2-layer model, D = 256, 4 experts top-2, one routing row, at B = 200 (5,600 sorted rows: the smallest batch whose expert GEMMs the
    uniform-routing dispatch sends to the ping-pong kernel) and at B = 264 (7,392 rows: two tiles per workgroup in the up-projection) -
    "weight_runahead" 0 and 1 bit-equal, and equal to the chain with the fused QKV + attention launch off.
(The fused QKV + attention kernel issues no touches: there is no issuing form of it to test.)"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from mode_diffusion_policy_amd import _lib as L  # noqa: E402

from hip_helpers import CANARY, p, stream  # noqa: E402

BF = torch.bfloat16
SPARE_ROWS, SPARE_COLS, LEAD = 3, 8, 64
TOUCH_SIZES = (0, 129, 2097152)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


class Padded:
    """[slabs, rows + SPARE_ROWS, cols + SPARE_COLS] bf16 between LEAD sentinel elements, everything pre-filled with the sentinel."""

    def __init__(self, rows, cols, slabs=1):
        self.rows, self.cols, self.ld, self.slabs = rows, cols, cols + SPARE_COLS, slabs
        self.slab = (rows + SPARE_ROWS) * self.ld
        self.buf = torch.full((2 * LEAD + slabs * self.slab,), CANARY, dtype=BF, device="cuda")
        self.t = self.buf[LEAD: LEAD + slabs * self.slab].view(slabs, rows + SPARE_ROWS, self.ld)
        assert self.t.data_ptr() % 16 == 0
        self.valid = self.t[:, :rows, :cols]

    def outside_intact(self):
        c = self.buf.clone()
        c[LEAD: LEAD + self.slabs * self.slab].view(self.slabs, self.rows + SPARE_ROWS, self.ld)[:, :self.rows, :self.cols] = CANARY
        return bool((c == CANARY).all())


def bits(t):
    return t.contiguous().view(torch.int16)


def touch_buffer(n, seed):
    """Exactly n bytes of device memory with a known pattern."""
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    if n:
        t.copy_(torch.randint(0, 256, (n,), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)))
    return t


def launch(cfg, desc):
    lib = L.load()
    assert lib.mode_set_option(b"gemm_cfg", cfg) == 0
    try:
        rc = lib.mode_gemm(C.byref(desc), stream())
        torch.cuda.synchronize()
    finally:
        lib.mode_set_option(b"gemm_cfg", 0)
    assert rc == 0, (cfg, rc)


@pytest.fixture(scope="module")
def swiglu_case():
    """Operands and the two references (ping-pong without a range, 128 x 128 ring), computed once."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    M, K, N = 448, 128, 128 * ((ncu + 1) // 2 + 32)
    assert 2 * (N // 128) > ncu                                        # more 224 x 128 output tiles than workgroups: two tiles per workgroup
    A = rnd(M, K, seed=1, scale=0.5).to(BF).cuda()
    W = rnd(2 * N, K, seed=2, scale=K ** -0.5).to(BF).cuda()
    b = rnd(2 * N, seed=3).cuda()
    rows = torch.arange(M, dtype=torch.int32, device="cuda")
    off = torch.tensor([0, M], dtype=torch.int32, device="cuda")
    keep = (A, W, b, rows, off)

    def run(cfg, t0=None, t1=None):
        out = Padded(M, N)
        d = L.ModeGemmDesc(dtype=L.MODE_BF16, epilogue=L.EPI_SWIGLU, out_dtype=L.MODE_BF16, M=M, N=N, K=K, A=p(A), lda=K, W=p(W), ldw=K, w_expert_stride=2 * N * K,
                           bias=p(b), bias_expert_stride=2 * N, C=p(out.t), ldc=out.ld, a_rows=p(rows), expert_offsets=p(off), num_experts=1,
                           flags=L.GEMM_UNIFORM_GROUPS | L.GEMM_IDENTITY_ROWS,
                           touch0=p(t0) if t0 is not None and t0.numel() else None, touch0_bytes=t0.numel() if t0 is not None else 0,
                           touch1=p(t1) if t1 is not None and t1.numel() else None, touch1_bytes=t1.numel() if t1 is not None else 0)
        launch(cfg, d)
        return out

    plain, ring = run(17), run(1)
    assert plain.outside_intact() and ring.outside_intact()
    assert not bool((plain.valid == CANARY).all(-1).any())
    assert torch.equal(bits(plain.valid), bits(ring.valid))
    return run, bits(plain.valid).clone(), keep


def none_sliced_run(cfg, t0=None, t1=None):
    M, K, N, S = 225, 512, 256, 4
    if not hasattr(none_sliced_run, "ops"):
        none_sliced_run.ops = (rnd(M, K, seed=11, scale=0.5).to(BF).cuda(), rnd(N, K, seed=12, scale=K ** -0.5).to(BF).cuda())
    A, W = none_sliced_run.ops
    out = Padded(M, N, slabs=S)
    d = L.ModeGemmDesc(dtype=L.MODE_BF16, epilogue=L.EPI_NONE, out_dtype=L.MODE_BF16, M=M, N=N, K=K, A=p(A), lda=K, W=p(W), ldw=K, C=p(out.t), ldc=out.ld,
                       split_k=S, split_stride=out.slab,
                       touch0=p(t0) if t0 is not None and t0.numel() else None, touch0_bytes=t0.numel() if t0 is not None else 0,
                       touch1=p(t1) if t1 is not None and t1.numel() else None, touch1_bytes=t1.numel() if t1 is not None else 0)
    launch(cfg, d)
    return out


@pytest.mark.parametrize("nbytes", TOUCH_SIZES)
def test_pingpong_swiglu_two_tiles_per_workgroup_is_bit_equal_with_a_touch_range(swiglu_case, nbytes):
    run, want, _ = swiglu_case
    t = touch_buffer(nbytes, seed=nbytes + 1)
    before = t.clone()
    for got in (run(17, t0=t), run(17, t1=t)):                         # as the first and as the second range of the launch
        assert got.outside_intact(), (nbytes, "bytes outside the valid region were written")
        assert torch.equal(bits(got.valid), want), (nbytes, "differs from the launch without a range / the ring geometry")
    assert torch.equal(t, before), "a touched buffer changed"


def test_pingpong_swiglu_two_ranges_in_one_launch(swiglu_case):
    run, want, _ = swiglu_case
    t0, t1 = touch_buffer(2097152, seed=5), touch_buffer(129, seed=6)
    b0, b1 = t0.clone(), t1.clone()
    got = run(17, t0=t0, t1=t1)
    assert got.outside_intact() and torch.equal(bits(got.valid), want)
    assert torch.equal(t0, b0) and torch.equal(t1, b1)
    ring = run(1, t0=t0, t1=t1)                                         # a geometry that ignores the hint takes the descriptor all the same
    assert ring.outside_intact() and torch.equal(bits(ring.valid), want)


@pytest.mark.parametrize("nbytes", TOUCH_SIZES)
def test_pingpong_k_sliced_one_tile_per_workgroup_is_bit_equal_with_a_touch_range(nbytes):
    plain, ring = none_sliced_run(17), none_sliced_run(1)
    assert plain.outside_intact() and ring.outside_intact()
    assert torch.equal(bits(plain.valid), bits(ring.valid))
    t = touch_buffer(nbytes, seed=nbytes + 2)
    before = t.clone()
    got = none_sliced_run(17, t0=t, t1=t)
    assert got.outside_intact(), (nbytes, "bytes outside the valid region were written")
    assert torch.equal(bits(got.valid), bits(plain.valid)), nbytes
    assert torch.equal(t, before)


# ================================================================================================================== the chain
@pytest.fixture(scope="module")
def small_model():
    import mode_diffusion_policy_amd as M
    torch.manual_seed(0)
    m = M.MoDeDiT(obs_dim=64, goal_dim=32, device="cuda", goal_conditioned=True, action_dim=7, embed_dim=256, embed_pdrob=0, attn_pdrop=0.0, n_layers=2,
                  n_heads=2, goal_seq_len=1, obs_seq_len=1, action_seq_len=10, num_experts=4, top_k=2, compute_dtype="bf16")
    return m.to("cuda").eval()


@pytest.mark.parametrize("B", [200, 264])
def test_chain_is_bit_equal_with_run_ahead_on_off_and_unfused(small_model, B):
    m, lib = small_model, L.load()
    assert B * m.seq_len * 2 == {200: 5600, 264: 7392}[B]
    g = torch.Generator().manual_seed(B)
    st = {"state_images": torch.randn(B, 2, 64, generator=g).cuda()}
    goal, x = torch.randn(B, 1, 32, generator=g).cuda(), (torch.randn(B, 10, 7, generator=g) * 3).cuda()
    sigma = torch.tensor(0.7)                                           # one noise level: one routing row for the whole batch

    def run(runahead, fuse, pp_min_tiles=200):
        assert lib.mode_set_option(b"weight_runahead", runahead) == 0 and lib.mode_set_option(b"fuse_qkv_attn", fuse) == 0
        assert lib.mode_set_option(b"gemm_pp_min_tiles", pp_min_tiles) == 0
        try:
            out = m.denoise(st, x, goal, sigma, 0.5)
            torch.cuda.synchronize()
        finally:
            lib.mode_set_option(b"weight_runahead", 1); lib.mode_set_option(b"fuse_qkv_attn", 1); lib.mode_set_option(b"gemm_pp_min_tiles", 200)
        return out.clone()

    on, off, unfused_on, unfused_off = run(1, 1), run(0, 1), run(1, 0), run(0, 0)
    assert torch.isfinite(on).all() and float(on.abs().max()) > 0
    assert torch.equal(on.view(torch.int32), off.view(torch.int32)), "weight_runahead changed the chain's output"
    assert torch.equal(on.view(torch.int32), unfused_on.view(torch.int32)) and torch.equal(on.view(torch.int32), unfused_off.view(torch.int32))
    # the issuing launch is the K-sliced down-projection, which at D = 256 has 100 / 132 tiles: below the ping-pong kernel's default threshold (200).
    # With the threshold at 64 it IS the ping-pong kernel and the chain's own ranges are issued (every forward geometry gives the same bits).
    assert torch.equal(on.view(torch.int32), run(1, 1, 64).view(torch.int32)) and torch.equal(on.view(torch.int32), run(0, 1, 64).view(torch.int32))
