"""Thin test-side wrappers that call the C-ABI (ctypes) with torch device tensors."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from mode_diffusion_policy_amd import _lib as L


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


def dt_of(t):
    return L.MODE_BF16 if t.dtype == torch.bfloat16 else L.MODE_F32


def gemm(A, W, epilogue=L.EPI_NONE, bias=None, resid=None, out_dtype=None, n_out=None, a_rows=None, offsets=None, num_experts=0,
         M=None, w_estride=0, b_estride=0, flags=0):
    lib = L.load()
    out_dtype = out_dtype or A.dtype
    K = A.shape[-1]
    Wm = W if W.dim() == 2 else W[0]
    N = n_out if n_out is not None else (Wm.shape[0] // 2 if epilogue == L.EPI_SWIGLU else Wm.shape[0])
    M = M if M is not None else A.shape[0]
    Cc = torch.full((M, N), float("nan"), dtype=out_dtype, device=A.device)
    d = L.ModeGemmDesc(dtype=dt_of(A), epilogue=epilogue, out_dtype=L.MODE_BF16 if out_dtype == torch.bfloat16 else L.MODE_F32,
                       M=M, N=N, K=K, A=p(A), lda=A.stride(0), W=p(W), ldw=Wm.stride(0), w_expert_stride=w_estride,
                       bias=p(bias), bias_expert_stride=b_estride, resid=p(resid), ldr=(resid.stride(0) if resid is not None else 0),
                       C=p(Cc), ldc=Cc.stride(0), a_rows=p(a_rows), expert_offsets=p(offsets), num_experts=num_experts, flags=flags)
    L.check(lib.mode_gemm(C.byref(d), stream()), "gemm")
    return Cc


def route_topk(logits, k, normalize=True):
    lib = L.load()
    R, E = logits.shape
    sh = torch.empty_like(logits); pr = torch.empty_like(logits)
    idx = torch.full((R, k), -1, dtype=torch.int32, device=logits.device)
    w = torch.empty(R, k, dtype=torch.float32, device=logits.device)
    L.check(lib.mode_moe_route_topk_f32(p(logits), R, E, k, int(normalize), p(sh), p(pr), p(idx), p(w), stream()), "route")
    return sh, pr, idx, w


def dispatch_meta(idx, w, tokens_per_row, N, E):
    lib = L.load()
    R, k = idx.shape
    dev = idx.device
    i32 = lambda *s: torch.full(s, -1, dtype=torch.int32, device=dev)
    counts, offsets, perm, pos = i32(E), i32(E + 1), i32(N * k), i32(N * k)
    posw = torch.empty(N * k, dtype=torch.float32, device=dev)
    poffsets, prow = i32(E + 1), i32(N * k)
    L.check(lib.mode_moe_dispatch_meta(p(idx), p(w), R, tokens_per_row, N, E, k, p(counts), p(offsets), p(perm), p(pos), p(posw),
                                       p(poffsets), p(prow), stream()), "dispatch_meta")
    return dict(counts=counts, offsets=offsets, perm=perm, pos=pos, posw=posw, poffsets=poffsets, prow=prow)


def rmsnorm(x, g, cond=None, rows_per_cond=1, eps=1e-6, lp_dtype=torch.bfloat16, want_f32=True):
    lib = L.load()
    rows, D = x.shape
    y32 = torch.empty_like(x) if want_f32 else None
    ylp = torch.empty(rows, D, dtype=lp_dtype, device=x.device)
    L.check(lib.mode_rmsnorm_cond_fwd(p(x), p(g), p(cond), rows, D, rows_per_cond, eps, p(y32), p(ylp),
                                      L.MODE_BF16 if lp_dtype == torch.bfloat16 else L.MODE_F32, stream()), "rmsnorm")
    return y32, ylp


def attn(qkv, qg, kg, B, T, H, hd, eps=1e-6, seed=0, p_drop=0.0, out=None):
    """mode_attn_block_fwd.  out: a Guarded [B*T, H*hd] to write into; then the status is returned (the caller decides what it means), else y."""
    lib = L.load()
    y = out.t if out is not None else torch.full((B * T, H * hd), float("nan"), dtype=qkv.dtype, device=qkv.device)
    rc = lib.mode_attn_block_fwd(p(qkv), p(qg), p(kg), p(y), dt_of(qkv), B, T, H, hd, eps, seed, p_drop, stream())
    if out is not None:
        return rc
    L.check(rc, "attn")
    return y


def attn_bwd(qkv, qg, kg, dy, B, T, H, hd, eps=1e-6, seed=0, p_drop=0.0):
    """mode_attn_block_bwd into Guarded outputs: returns (status, dqkv [B*T, 3D], dgq_partial [B*H, hd], dgk_partial [B*H, hd])."""
    lib = L.load()
    dqkv, pq, pk = Guarded(B * T, 3 * H * hd, qkv.dtype), Guarded(B * H, hd), Guarded(B * H, hd)
    rc = lib.mode_attn_block_bwd(p(qkv), p(qg), p(kg), p(dy), p(dqkv.t), p(pq.t), p(pk.t), dt_of(qkv), B, T, H, hd, eps, seed, p_drop, stream())
    return rc, dqkv, pq, pk


def qkv_attn(h, wqkv, bqkv, qg, kg, B, T, H, eps=1e-6, D=None, out=None, ldy=None):
    """mode_qkv_attn_fwd: returns (status, y) - the caller decides what an UNSUPPORTED (-2) shape means.  h / wqkv may be column slices of wider
    buffers (D = the logical width); out: a Guarded [B*T, ldy] whose first D columns are y."""
    lib = L.load()
    D = D or h.shape[1]
    y = out.t if out is not None else torch.full((B * T, D), float("nan"), dtype=h.dtype, device=h.device)
    d = L.ModeQkvAttnDesc(dtype=dt_of(h), B=B, T=T, H=H, D=D, h=p(h), ldh=h.stride(0), wqkv=p(wqkv), ldw=wqkv.stride(0), bqkv=p(bqkv), q_gain=p(qg),
                          k_gain=p(kg), eps=eps, y=p(y), ldy=ldy or y.stride(0))
    return lib.mode_qkv_attn_fwd(C.byref(d), stream()), y


CANARY = -1536.0          # exact in bf16 and fp32


class Guarded:
    """A NaN-prefilled [rows, cols] output `t` with at least 2 canary rows before and after it (the pad is a multiple of 8 elements, so that `t` keeps the
    allocation's 16-byte alignment); `intact()` after the launch: nothing was written outside `t`."""

    def __init__(self, rows, cols, dtype=torch.float32, fill=float("nan")):
        self.pad = -(-2 * cols // 8) * 8
        self.buf = torch.full((2 * self.pad + rows * cols,), CANARY, dtype=dtype, device="cuda")
        self.t = self.buf[self.pad: self.pad + rows * cols].view(rows, cols)
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.buf[: self.pad] == CANARY).all()) and bool((self.buf[self.pad + self.t.numel():] == CANARY).all())


class GuardedCols(Guarded):
    """A Guarded [rows, ld] buffer whose logical output `out` is the columns [col0, col0 + cols) of every row: NaN-prefilled, every other column of
    those rows holding the canary value like the rows around them.  `intact()`: neither the canary rows nor the pad columns were written."""

    def __init__(self, rows, cols, ld, dtype=torch.float32, col0=0):
        assert col0 + cols <= ld
        super().__init__(rows, ld, dtype, fill=CANARY)
        self.out = self.t[:, col0: col0 + cols]
        self.out.fill_(float("nan"))
        self.ld, self.cols, self.col0 = ld, cols, col0
        assert self.out.data_ptr() % 16 == 0

    def intact(self):
        return super().intact() and bool((self.t[:, : self.col0] == CANARY).all()) and bool((self.t[:, self.col0 + self.cols:] == CANARY).all())


def gemm_into(A, W, out, M, N, K, epilogue=L.EPI_NONE, bias=None, resid=None, a_rows=None, offsets=None, num_experts=0, w_estride=0, b_estride=0,
              split_k=0, split_stride=0, flags=0, C2=None, gain=None, row_ss_out=None, row_ss=None, row_eps=0.0, lda=None, ldw=None,
              k_group_offsets=None, num_k_groups=0, c_group_stride=0, w_rows=None, w_tap_cols=0, w_rows_tap_stride=0, a_tap_cols=0, a_rows_tap_stride=0):
    """mode_gemm through a full descriptor into GuardedCols outputs; returns the status (the caller decides what it means).  A / W / resid may be column
    slices of wider buffers (their row strides are the leading dimensions; W is the first expert's [Nw, K] view, or its [K, N] view under MODE_GEMM_W_KN);
    out / C2: GuardedCols (ldc / ldc2 are their widths); row_ss_out: a Guarded [M, N / group]; row_ss: [tokens, row_ss_n].  The backward layouts'
    fields: k_group_offsets int32 [num_k_groups + 1] with group z written c_group_stride elements after group z - 1 (`out` holds them all); w_rows int32
    index tables, w_rows_tap_stride apart when w_tap_cols > 0; a_rows in taps (the implicit-GEMM convolution): a_tap_cols columns per tap, the tables
    a_rows_tap_stride apart."""
    lib = L.load()
    d = L.ModeGemmDesc(dtype=dt_of(A), epilogue=epilogue, out_dtype=dt_of(out.out), M=M, N=N, K=K, A=p(A), lda=lda if lda is not None else A.stride(0),
                       W=p(W), ldw=ldw if ldw is not None else W.stride(0), w_expert_stride=w_estride, bias=p(bias), bias_expert_stride=b_estride,
                       resid=p(resid), ldr=0 if resid is None else resid.stride(0), C=p(out.out), ldc=out.ld, a_rows=p(a_rows), expert_offsets=p(offsets),
                       num_experts=num_experts, split_k=split_k, split_stride=split_stride, flags=flags, C2=p(C2 and C2.out), ldc2=C2.ld if C2 else 0,
                       gain=p(gain), row_ss_out=p(row_ss_out and row_ss_out.t), row_ss=p(row_ss), row_ss_n=0 if row_ss is None else row_ss.shape[1],
                       row_eps=row_eps, k_group_offsets=p(k_group_offsets), num_k_groups=num_k_groups, c_group_stride=c_group_stride, w_rows=p(w_rows),
                       w_tap_cols=w_tap_cols, w_rows_tap_stride=w_rows_tap_stride, a_tap_cols=a_tap_cols, a_rows_tap_stride=a_rows_tap_stride)
    return lib.mode_gemm(C.byref(d), stream())


def launch_guard(D, *tensors, pos=None, n_sorted=None):
    """Host-side contract of the row kernels, asserted before every launch: D % 4 == 0, 16-byte aligned base pointers, pos inside [0, n_sorted)."""
    assert D % 4 == 0, D
    for t in tensors:
        assert t is None or (t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0), "unaligned or non-contiguous operand"
    if pos is not None:
        assert pos.dtype == torch.int32 and int(pos.min()) >= 0 and int(pos.max()) < n_sorted, "pos outside the sorted rows"


def combine_fused(u, Y, pos, posw, g, cond, rpc, x_next, h, u_ss=None, u_gain=None, eps=1e-6):
    """mode_moe_combine_norm_fused_fwd on Y [S, N*k, D]; x_next / h are Guarded outputs or None.  Returns the status."""
    lib = L.load()
    (N, D), (S, NK, _), k = u.shape, Y.shape, pos.shape[1]
    assert NK == N * k and posw.shape == pos.shape and (u_ss is None or D % u_ss.shape[1] == 0)
    launch_guard(D, u, Y, pos, posw, g, cond, u_ss, u_gain, x_next and x_next.t, h and h.t, pos=pos, n_sorted=NK)
    return lib.mode_moe_combine_norm_fused_fwd(p(u), p(u_ss), 0 if u_ss is None else u_ss.shape[1], p(u_gain), p(Y), dt_of(Y), S, NK * D, p(pos), p(posw),
                                               N, D, k, p(g), p(cond), rpc, eps, p(x_next and x_next.t), p(h and h.t),
                                               dt_of(h.t) if h else L.MODE_F32, stream())


def head_desc(u, Y, pos, posw, g, w_out, b_out, B, T, A_len, eps=1e-6, u_ss=None, u_gain=None, x_a=None, scal=None, scal_stride=0, **out):
    """ModeHeadDesc on Y [S, N*k, D]; out: F / denoised / x_next / den_prev / lin / aux1 / aux2 as tensors."""
    (N, D), (S, NK, _), k, A_dim = u.shape, Y.shape, pos.shape[1], w_out.shape[0]
    assert N == B * T and NK == N * k and (u_ss is None or D % u_ss.shape[1] == 0) and (scal is None or scal.shape[0] >= (B if scal_stride else 1))
    launch_guard(D, u, Y, pos, posw, g, w_out, b_out, u_ss, u_gain, x_a, scal, *out.values(), pos=pos, n_sorted=NK)
    return L.ModeHeadDesc(B=B, T=T, D=D, A_len=A_len, A_dim=A_dim, k=k, u=p(u), Y=p(Y), y_dtype=dt_of(Y), y_splits=S, y_split_stride=NK * D, pos=p(pos),
                          posw=p(posw), g=p(g), eps=eps, w_out=p(w_out), b_out=p(b_out), x_a=p(x_a), scal=p(scal), scal_stride=scal_stride,
                          u_ss=p(u_ss), u_ss_n=0 if u_ss is None else u_ss.shape[1], u_gain=p(u_gain), **{k_: p(v) for k_, v in out.items()})


def combine_norm(u, Y, pos, posw, k, g, cond, rows_per_cond, eps=1e-6, h_dtype=torch.bfloat16):
    lib = L.load()
    N, D = u.shape
    xn = torch.empty_like(u)
    h = torch.empty(N, D, dtype=h_dtype, device=u.device)
    L.check(lib.mode_moe_combine_norm_fwd(p(u), p(Y), dt_of(Y), 1, 0, p(pos), p(posw), N, D, k, p(g), p(cond), rows_per_cond, eps, p(xn), p(h),
                                          L.MODE_BF16 if h_dtype == torch.bfloat16 else L.MODE_F32, stream()), "combine_norm")
    return xn, h


def dev_store(eps, norm):
    """The episode store's device tables, as data.EpisodeStore.finalize() lays them out, built by hand for the ctypes path."""
    lengths = [e[0].shape[0] for e in eps]
    t = dict(actions=torch.from_numpy(np.concatenate([e[0] for e in eps])).cuda(), goals=torch.from_numpy(np.stack([e[1] for e in eps])).cuda(),
             ep_begin=torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)).cuda(), lengths=lengths)
    t["lo"], t["scale"] = (None, None) if norm is None else (torch.from_numpy(norm[0]).cuda(), torch.from_numpy(norm[1]).cuda())
    return t
