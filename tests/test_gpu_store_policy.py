"""The forward chain's output stores (csrc/mode_common.h: StorePolicy, store_out16 / store_out8) through the ctypes entry points tests/hip_helpers.py
uses.  A store's cache policy cannot change a value; what such a change CAN break is a store's predicate or its address.  So every output here
lives in a buffer with spare rows and spare columns (ldc > N) pre-filled with a sentinel, and

  * every byte OUTSIDE the valid region must still be the sentinel after the launch,
  * every byte INSIDE must be bit-equal to another geometry of the same operation - the project's own guarantee (a result does not depend on the
    tile geometry it was computed with) - or, for the row kernels, within the bounds of tests/test_gpu_row_kernels.py of the fp64 restatements
    in tests/row_refs.py (fp32 rows rel-L2 < 1e-6, one bf16 rounding < 4e-3, head outputs 1e-5 / 3e-5 of the reference's norm).

Shapes are the smallest that reach every store site: the persistent ping-pong GEMM forced with "gemm_cfg" 17 (224-row tile) and 18 (256-row tile) at
M = 225 - the 224-row tile's second m-tile holds ONE valid row - with K = 128 S for S in {1, 4} (S K-slices for the NONE epilogue, which is the only one
that is cut into slices; one 128 S deep product otherwise: one and four K-step pairs), N = 256 (SwiGLU: 256 weight rows), bf16 and fp32 output,
grouped with expert segments of {0, 1, 224, 225} rows; c_proj's RESIDUAL_NORM epilogue at M = 65, N = 64, K = 128 on three ring geometries; the fused
QKV + attention at B = 5 (one full group of four samples and a partial one) against GEMM + attention; the three row kernels at 3 rows, D = 1024."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from mode_diffusion_policy_amd import _lib as L  # noqa: E402

import hip_helpers as H  # noqa: E402
import row_refs as R  # noqa: E402
from hip_helpers import CANARY, p, stream  # noqa: E402
from row_refs import nrm, rel  # noqa: E402

F32, LP, HEAD = 1e-6, 4e-3, 1e-5          # tests/test_gpu_row_kernels.py
BF, FP = torch.bfloat16, torch.float32
SPARE_ROWS, SPARE_COLS, LEAD = 3, 8, 64


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


class Padded:
    """[slabs, rows + SPARE_ROWS, cols + SPARE_COLS] of `dtype` behind LEAD sentinel elements and in front of as many, all pre-filled with the
    sentinel.  `.t` is the whole slab stack (its data pointer is the output's base, `.ld` its row stride, `.slab` its slab stride), `.valid` the
    [slabs, rows, cols] region a launch may write, `.outside_intact()` whether it wrote nothing else."""

    def __init__(self, rows, cols, dtype, slabs=1, spare_cols=SPARE_COLS):
        self.rows, self.cols, self.ld, self.slabs = rows, cols, cols + spare_cols, slabs
        self.slab = (rows + SPARE_ROWS) * self.ld
        self.buf = torch.full((2 * LEAD + slabs * self.slab,), CANARY, dtype=dtype, device="cuda")
        self.t = self.buf[LEAD: LEAD + slabs * self.slab].view(slabs, rows + SPARE_ROWS, self.ld)
        assert self.t.data_ptr() % 16 == 0
        self.valid = self.t[:, :rows, :cols]

    def outside_intact(self):
        c = self.buf.clone()
        c[LEAD: LEAD + self.slabs * self.slab].view(self.slabs, self.rows + SPARE_ROWS, self.ld)[:, :self.rows, :self.cols] = CANARY
        return bool((c == CANARY).all())


def with_cfg(cfg, fn):
    lib = L.load()
    assert lib.mode_set_option(b"gemm_cfg", cfg) == 0
    try:
        rc = fn()
        torch.cuda.synchronize()
    finally:
        lib.mode_set_option(b"gemm_cfg", 0)
    assert rc == 0, (cfg, rc)


# ================================================================================================================== the ping-pong GEMM's epilogue
def pp_operands(M, K, n_w_rows, E):
    """bf16 A [M, K], W [E or 1, n_w_rows, K], fp32 bias [E or 1, n_w_rows] - computed once per (M, K, rows, E) and shared by every case."""
    key = (M, K, n_w_rows, E)
    if key not in pp_operands.cache:
        A = rnd(M, K, seed=M + K, scale=0.5).to(BF).cuda()
        W = rnd(max(E, 1), n_w_rows, K, seed=K + n_w_rows + E, scale=K ** -0.5).to(BF).cuda()
        b = rnd(max(E, 1), n_w_rows, seed=3 + E).cuda()
        pp_operands.cache[key] = (A, W, b)
    return pp_operands.cache[key]


pp_operands.cache = {}


def run_pp_case(cfg, M, epi, S, odt, counts=None):
    """One GEMM on geometry `cfg` into a Padded output.  S > 1 with the NONE epilogue: S K-slice slabs; otherwise one product over K = 128 S."""
    lib = L.load()
    E = len(counts) if counts else 0
    K = 128 * S
    slices = S if epi == L.EPI_NONE else 1
    n_w_rows = 256
    N = 128 if epi == L.EPI_SWIGLU else 256
    A, W, b = pp_operands(M, K, n_w_rows, E)
    out = Padded(M, N, odt, slabs=slices)
    off = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32, device="cuda") if counts else None
    d = L.ModeGemmDesc(dtype=L.MODE_BF16, epilogue=epi, out_dtype=L.MODE_BF16 if odt == BF else L.MODE_F32, M=M, N=N, K=K, A=p(A), lda=K, W=p(W), ldw=K,
                       w_expert_stride=n_w_rows * K if E else 0, bias=None if epi == L.EPI_NONE else p(b), bias_expert_stride=n_w_rows if E else 0,
                       C=p(out.t), ldc=out.ld, expert_offsets=p(off), num_experts=E, split_k=slices, split_stride=out.slab)
    with_cfg(cfg, lambda: lib.mode_gemm(C.byref(d), stream()))
    return out, (A, W, b)


def check_pp_case(cfg, M, epi, S, odt, counts=None):
    what = (cfg, M, epi, S, odt, counts)
    got, (A, W, b) = run_pp_case(cfg, M, epi, S, odt, counts)
    ref, _ = run_pp_case(1, M, epi, S, odt, counts)                     # the 128 x 128 two-slot ring
    assert got.outside_intact(), (what, "bytes outside the valid region were written")
    assert ref.outside_intact(), (what, "ring: bytes outside the valid region were written")
    assert not bool((got.valid == CANARY).all(-1).any()), (what, "a valid row was not written")
    assert torch.equal(bits(got.valid), bits(ref.valid)), (what, "differs from the ring kernel's bits")
    if epi != L.EPI_SWIGLU:                                             # and the ring's own result is the product (bf16 bound of tests/test_gpu_kernels.py)
        want = torch.empty(M, 256)
        lo = 0
        for e, c in enumerate(counts or [M]):
            want[lo:lo + c] = A[lo:lo + c].float().cpu() @ W[e].float().cpu().t() + (b[e].cpu() if epi == L.EPI_BIAS else 0)
            lo += c
        e_ = rel(got.valid.float().sum(0), want)
        print(f"pp {what}: rel-L2 against fp32 torch {e_:.2e} (< 6e-3)")
        assert e_ < 6e-3, what


@pytest.mark.parametrize("odt", [BF, FP], ids=["bf16", "fp32"])
@pytest.mark.parametrize("cfg,M", [(17, 225), (18, 225), (18, 257)])
def test_pingpong_epilogue_writes_its_valid_region_only(cfg, M, odt):
    """NONE (one slab and four K-slice slabs) and BIAS (K = 128 and 512) on both tiles; SwiGLU on the 224-row tile, the only one that has it.  M = 257 adds
    the 256-row tile's own one-row second m-tile."""
    for epi in (L.EPI_NONE, L.EPI_BIAS) + ((L.EPI_SWIGLU,) if cfg == 17 else ()):
        for S in (1, 4):
            check_pp_case(cfg, M, epi, S, odt)


@pytest.mark.parametrize("odt", [BF, FP], ids=["bf16", "fp32"])
@pytest.mark.parametrize("cfg", [17, 18])
def test_pingpong_epilogue_grouped_segments_of_0_1_224_225_rows(cfg, odt):
    """Four experts owning 0, 1, 224 and 225 sorted rows: an empty segment, a one-row tile, a full 224-row tile, and a tile pair whose second holds one row."""
    counts = (0, 1, 224, 225)
    for epi in (L.EPI_NONE, L.EPI_BIAS) + ((L.EPI_SWIGLU,) if cfg == 17 else ()):
        for S in (1, 4):
            check_pp_case(cfg, sum(counts), epi, S, odt, counts)


# ================================================================================================================== c_proj: the ring kernel's RESIDUAL_NORM epilogue
def test_residual_norm_epilogue_writes_its_valid_region_only():
    """x (fp32), the gain-scaled bf16 copy and the per-64-column sums of squares at M = 65, N = 64, K = 128 on the 64 x 64, 128 x 64 and 128 x 128 rings:
    same bits, nothing outside [65, 64] of either output or past the 65 row sums; x against fp32 torch at the bound of tests/test_gpu_kernels.py."""
    lib = L.load()
    M, N, K = 65, 64, 128
    ya = rnd(M, K, seed=1, scale=0.5).to(BF).cuda(); wo = rnd(N, K, seed=2, scale=K ** -0.5).to(BF).cuda()
    x0 = rnd(M, N, seed=3).cuda(); g2 = (1 + 0.1 * rnd(N, seed=4)).cuda()
    outs = {}
    for cfg in (14, 4, 1):
        x, h, ss = Padded(M, N, FP), Padded(M, N, BF), Padded(M, 1, FP, spare_cols=0)
        d = L.ModeGemmDesc(dtype=L.MODE_BF16, epilogue=L.EPI_RESIDUAL_NORM, out_dtype=L.MODE_F32, M=M, N=N, K=K, A=p(ya), lda=K, W=p(wo), ldw=K, resid=p(x0), ldr=N,
                           C=p(x.t), ldc=x.ld, C2=p(h.t), ldc2=h.ld, gain=p(g2), row_ss_out=p(ss.t))
        with_cfg(cfg, lambda: lib.mode_gemm(C.byref(d), stream()))
        for name, o in (("x", x), ("h", h), ("ss", ss)):
            assert o.outside_intact(), (cfg, name, "bytes outside the valid region were written")
        outs[cfg] = (x.valid.clone(), h.valid.clone(), ss.valid.clone())
    for cfg in (4, 1):
        for a, b in zip(outs[cfg], outs[14]):
            assert torch.equal(bits(a), bits(b)), cfg
    xg = outs[14][0][0]
    ref = x0 + ya.float() @ wo.float().t()
    e = float((xg - ref).norm() / ref.norm())
    print(f"residual_norm: x rel-L2 {e:.2e} (< 1e-3)")
    assert e < 1e-3
    assert torch.equal(bits(outs[14][1][0]), bits((xg * g2).to(BF)))          # the bf16 copy is one rounding of x * gain
    assert float((outs[14][2][0, :, 0] - (xg ** 2).sum(1)).abs().max() / (xg ** 2).sum(1).max()) < 1e-5


# ================================================================================================================== attention output (attn_core.h)
def test_fused_qkv_attention_writes_its_valid_region_only():
    """B = 5 samples of 14 tokens, 8 heads of 128: the fused launch into y with ldy = D + 8 and spare rows, against the QKV GEMM + the stand-alone
    attention kernel (which shares the output store), itself between canary rows."""
    lib = L.load()
    B, T, Hh, hd = 5, 14, 8, 128
    D = Hh * hd
    h = rnd(B * T, D, seed=61).to(BF).cuda(); w = rnd(3 * D, D, seed=62, scale=D ** -0.5).to(BF).cuda()
    b = (0.1 * rnd(3 * D, seed=63)).cuda(); qg = (1 + 0.1 * rnd(hd, seed=64)).cuda(); kg = (1 + 0.1 * rnd(hd, seed=65)).cuda()
    y = Padded(B * T, D, BF)
    d = L.ModeQkvAttnDesc(dtype=L.MODE_BF16, B=B, T=T, H=Hh, D=D, h=p(h), ldh=D, wqkv=p(w), ldw=D, bqkv=p(b), q_gain=p(qg), k_gain=p(kg), eps=1e-6,
                          y=p(y.t), ldy=y.ld)
    assert lib.mode_set_option(b"fuse_qkv_attn_min_b", 0) == 0
    try:
        rc = lib.mode_qkv_attn_fwd(C.byref(d), stream())
        torch.cuda.synchronize()
    finally:
        lib.mode_set_option(b"fuse_qkv_attn_min_b", 56)
    assert rc == 0, rc
    assert y.outside_intact(), "bytes outside the valid region were written"
    qkv = H.gemm(h, w, epilogue=L.EPI_BIAS, bias=b)
    y2 = H.Guarded(B * T, D, BF)
    L.check(lib.mode_attn_block_fwd(p(qkv), p(qg), p(kg), p(y2.t), L.MODE_BF16, B, T, Hh, hd, 1e-6, 0, 0.0, stream()), "attn")
    torch.cuda.synchronize()
    assert y2.intact(), "attention: canary rows overwritten"
    assert not torch.isnan(y2.t.float()).any()
    assert torch.equal(bits(y.valid[0]), bits(y2.t))


# ================================================================================================================== row kernels: 3 rows, D = 1024
D_ROW = 1024


def test_combine_row_kernel_three_rows():
    """combine + ln_1 (one workgroup per row; k = 2, four bf16 slabs, fused ln_2) on 3 rows: x_next fp32, h bf16, between canary rows."""
    n, k, S, nss = 3, 2, 4, 16
    u = rnd(n, D_ROW, seed=1); Y = rnd(S, n * k, D_ROW, seed=2, scale=0.5).to(BF)
    pos = torch.randperm(n * k, generator=torch.Generator().manual_seed(3)).to(torch.int32).view(n, k)
    posw = 0.2 + rnd(n, k, seed=4).abs(); g = 1.0 + 0.1 * rnd(D_ROW, seed=5); cond = rnd(1, D_ROW, seed=6)
    u_ss, u_gain = R.partial_ss(u, nss), 1.0 + 0.2 * rnd(D_ROW, seed=7)
    xn, h = H.Guarded(n, D_ROW), H.Guarded(n, D_ROW, BF)
    rc = H.combine_fused(u.cuda(), Y.cuda(), pos.cuda(), posw.cuda(), g.cuda(), cond.cuda(), n, xn, h, u_ss.cuda(), u_gain.cuda())
    torch.cuda.synchronize()
    assert rc == 0 and xn.intact() and h.intact(), rc
    xr, hr = R.combine(u, Y.float(), pos, posw, g, cond, n, u_ss=u_ss, u_gain=u_gain)
    ex, eh = rel(xn.t, xr), rel(h.t.float(), hr)
    print(f"combine 3 rows: x_next {ex:.2e} (< {F32:.0e}), h {eh:.2e} (< {LP:.0e})")
    assert ex < F32 and eh < LP


def test_embed_row_kernel_three_rows():
    """Token embedding + ln_1 on one sample of 3 tokens (goal, one image token, one action row): x fp32, h bf16, between canary rows."""
    lib, B, A_len, A_dim, n_img = L.load(), 1, 1, 7, 1
    T = 1 + n_img + A_len
    act, w_act = rnd(B, A_len, A_dim, seed=4, scale=2.0), rnd(D_ROW, A_dim, seed=6, scale=0.3)
    pos, g, goal_e, img_e = rnd(1 + A_len, D_ROW, seed=7, scale=0.2), 1.0 + 0.1 * rnd(D_ROW, seed=8), rnd(B, D_ROW, seed=2), rnd(B, n_img, D_ROW, seed=3)
    dv = [t.cuda().contiguous() for t in (goal_e, img_e, act, w_act, pos, g)]
    x, h = H.Guarded(B * T, D_ROW), H.Guarded(B * T, D_ROW, BF)
    H.launch_guard(D_ROW, *dv, x.t, h.t)
    desc = L.ModeEmbedDesc(B=B, T=T, D=D_ROW, A_len=A_len, A_dim=A_dim, n_img=n_img, use_noise_token=0, emb_t=None, emb_row_stride=0, goal_e=p(dv[0]),
                           img_e=p(dv[1]), actions=p(dv[2]), c_in=None, c_in_stride=0, w_act=p(dv[3]), pos=p(dv[4]), g=p(dv[5]), cond=None, cond_row_stride=0,
                           eps=1e-6, x=p(x.t), h=p(h.t), h_dtype=L.MODE_BF16)
    rc = lib.mode_embed_tokens_fwd(C.byref(desc), stream())
    torch.cuda.synchronize()
    assert rc == 0 and x.intact() and h.intact(), rc
    xr, hr = R.embed(goal_e, img_e, act, w_act, pos, g)
    ex, eh = rel(x.t, xr.reshape(-1, D_ROW)), rel(h.t.float(), hr.reshape(-1, D_ROW))
    print(f"embed 3 rows: x {ex:.2e} (< {F32:.0e}), h {eh:.2e} (< {LP:.0e})")
    assert ex < F32 and eh < LP


def test_head_row_kernel_three_rows():
    """Last combine + final norm + output projection + DDIM update on one sample of 3 tokens, 2 of them action rows: F, denoised and x_next between
    canary rows."""
    lib, B, T, A_len, A_dim, k, S, nss = L.load(), 1, 3, 2, 7, 2, 4, 16
    n = B * T
    u = rnd(n, D_ROW, seed=11); Y = rnd(S, n * k, D_ROW, seed=12, scale=0.5).to(BF)
    pos = torch.randperm(n * k, generator=torch.Generator().manual_seed(13)).to(torch.int32).view(n, k)
    posw = 0.2 + rnd(n, k, seed=14).abs(); g = 1.0 + 0.1 * rnd(D_ROW, seed=15)
    u_ss, u_gain = R.partial_ss(u, nss), 1.0 + 0.2 * rnd(D_ROW, seed=17)
    w_out, b_out = rnd(A_dim, D_ROW, seed=23, scale=D_ROW ** -0.5), rnd(A_dim, seed=24, scale=0.1)
    x_a, scal = rnd(B, A_len, A_dim, seed=25, scale=3.0), torch.tensor([[0.4, 0.8, 0.6, 0.0]])
    out = {name: H.Guarded(B * A_len, A_dim) for name in ("F", "denoised", "x_next")}
    desc = H.head_desc(u.cuda(), Y.cuda(), pos.cuda(), posw.cuda(), g.cuda(), w_out.cuda(), b_out.cuda(), B, T, A_len, u_ss=u_ss.cuda(), u_gain=u_gain.cuda(),
                       x_a=x_a.cuda(), scal=scal.cuda(), scal_stride=0, **{k_: v.t for k_, v in out.items()})
    rc = lib.mode_head_ddim_fwd(C.byref(desc), stream())
    torch.cuda.synchronize()
    assert rc == 0 and all(v.intact() for v in out.values()), rc
    ref = R.head(u, Y.float(), pos, posw, g, w_out, b_out, B, T, A_len, u_ss=u_ss, u_gain=u_gain, x_a=x_a, scal=scal)
    for (name, mult), r in zip((("F", 1), ("denoised", 1), ("x_next", 3)), ref):
        r = r.reshape(-1, A_dim)
        e, tol = nrm(out[name].t.double().cpu() - r), mult * HEAD * nrm(r)
        print(f"head 3 rows: {name} {e:.2e} (<= {tol:.2e})")
        assert e <= tol, name
