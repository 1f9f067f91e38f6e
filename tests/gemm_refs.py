"""The fp64 reference of mode_gemm's forward layout (include/mode_hip.h: ModeGemmDesc, ModeEpilogue), the per-element bound, the input families, the
launchers' acceptance predicates and the case table, shared by tests/test_gpu_gemm_edges.py (which launches the kernels) and
tests/test_gemm_references.py (which validates all of this without a GPU).  The reference is written from the header's description of the operation:
plain torch on the CPU, operands widened to fp64 here.

The bound (LABNOTES.md, "Forward GEMM family against fp64").  Products of bf16 operands are exact in fp32; any order of K fp32 additions errs by at most
K u S with S = sum_k |a| |w| (+ |bias| + |resid|) and u = 2^-23 (a truncating adder tree inside the MFMA is covered).  Per output element:
  fp32 out, linear epilogue   (K + 2) u S                        (K + 3 for fp32 operands: the products round too)
  bf16 out                    + half a bf16 unit in the last place at the reference value, 2^(floor(log2 |ref|) - 8), and nothing more
  C2 of RESIDUAL_NORM         the fp32 term times |gain[n]|, + the bf16 half unit at C * gain
  row_ss_out                  sum over the group of 2 |C| bound_C, + (group + 1) u sum C^2
  GELU / SwiGLU               the pre-activation bound through the fp64 derivative AT the reference point (SwiGLU: |silu(g)| bound_v + |v| |silu'(g)| bound_g),
                              + 4 x the reference-alone gap of the case: the same expression in fp32 torch on the CPU from the fp64 pre-activation, against
                              fp64, as max |f32 - f64| / magnitude (magnitude: 0.5 |x| (1 + |erf|) for GELU, |v silu(g)| for SwiGLU) times the magnitude
  row factor (SwiGLU, row_ss) the accumulator bounds times the factor, + (row_ss_n + 6) u |acc| factor: the fp32 evaluation of the factor itself
                              (row_ss_n - 1 additions, sqrt, K^-1/2, its product, reciprocal: gemm_bf16.hip:187-209, gemm_bf16_skinny.hip:46-78,
                              gemm_bf16_pp.hip:274-280) - a named term, derived like the others
  split-K slab z              the product over K range z alone with K / split_k in place of K; the slab sum (fp64, slice order) against the whole
                              product under the sum of the slab bounds."""
import collections
import functools
import math

import torch
import torch.nn.functional as F

BF16, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -23
NONE, BIAS, BIAS_GELU, RESIDUAL, SWIGLU, RESIDUAL_NORM = range(6)                  # ModeEpilogue (checked against _lib by test_gemm_references.py)
EPI_NAME = ("NONE", "BIAS", "BIAS_GELU", "RESIDUAL", "SWIGLU", "RESIDUAL_NORM")
SKINNY_OK, UNIFORM_GROUPS, SMALL_ROWS, IDENTITY_ROWS = 1, 8, 16, 32                 # MODE_GEMM_* flags of the forward layout
FAMILIES = ("soft", "tails", "clamp")
CLAMP_EPS, SOFT_EPS = 2.0 ** -10, 1e-6
SKINNY_ROWS, MID_ROWS, MID_ROWS_RN = 32, 128, 512                                   # the library's defaults ("gemm_skinny_rows", "gemm_mid_rows", "gemm_mid_rows_rn")


def f64(t):
    return None if t is None else torch.as_tensor(t).detach().double().cpu()


# ------------------------------------------------------------------------------------------------------------------ cases
_Case = collections.namedtuple("Case", "kernel cfg epi out M N K family dtype counts gather split_k flags ss_n pad wextra bextra")


class Case(_Case):
    """One launch.  kernel: the kernel the case is meant for ("ring", "pp", "stream", "mid", "f32"); cfg: "gemm_cfg"; counts: expert segment lengths
    (grouped; M is their sum) or None; gather: a_rows (a permutation with repeats, or the per-segment identity under IDENTITY_ROWS); pad = (pa, pw, pc,
    off): lda = K + pa, ldw = K + pw, ldc = N + pc (ldr = N + pc + 4 and ldc2 = N + pc + 8 when pc > 0), and A / W / resid / C start `off` columns
    (C: off / 2 for fp32 output: 16 bytes) into their buffers; wextra: rows between two experts' matrices; bextra: bias_expert_stride - bias width."""
    __slots__ = ()

    @property
    def E(self):
        return len(self.counts) if self.counts else 1

    @property
    def Nw(self):
        return 2 * self.N if self.epi == SWIGLU else self.N

    @property
    def tokens(self):
        if not self.gather:
            return self.M
        return max(self.counts) if self.flags & IDENTITY_ROWS else -(-self.M // 2)

    @property
    def group(self):
        return 16 if self.flags & SMALL_ROWS else 64

    lda = property(lambda s: s.K + s.pad[0])
    ldw = property(lambda s: s.K + s.pad[1])
    ldc = property(lambda s: s.N + s.pad[2])
    ldr = property(lambda s: s.N + s.pad[2] + (4 if s.pad[2] else 0))
    ldc2 = property(lambda s: s.N + s.pad[2] + (8 if s.pad[2] else 0))
    c_off = property(lambda s: s.pad[3] if s.out == BF16 else s.pad[3] // 2)
    b_estride = property(lambda s: s.Nw + s.bextra)
    w_estride = property(lambda s: (s.Nw + s.wextra) * s.ldw)
    split_stride = property(lambda s: (s.M + 1) * s.ldc)               # one untouched row between two slabs

    @property
    def tag(self):
        t = f"{self.kernel} cfg={self.cfg} {EPI_NAME[self.epi]} {'bf16' if self.out == BF16 else 'f32'} M={self.M} N={self.N} K={self.K} {self.family}"
        if self.dtype == F32:
            t += " fp32-operands"
        if self.counts:
            t += f" segments={self.counts}"
        if self.gather:
            t += " gathered"
        if self.split_k > 1:
            t += f" split_k={self.split_k}"
        if self.flags:
            t += f" flags={self.flags}"
        if self.ss_n:
            t += f" row_ss_n={self.ss_n}"
        return t + f" pad={self.pad}"

    @property
    def data_key(self):
        """What the inputs and the reference depend on: everything but the geometry, the output dtype and the hint flags."""
        return self._replace(kernel="", cfg=0, out=F32, flags=self.flags & (SMALL_ROWS | IDENTITY_ROWS))


def case(kernel, cfg, epi, out, M, N, K, family="soft", dtype=BF16, counts=None, gather=False, split_k=1, flags=0, ss_n=0, pad=None, wextra=0, bextra=0):
    if counts:
        M = sum(counts)
    if pad is None:
        pad = (4, 4, 3, 0) if dtype == F32 else (8, 8, 8, 0)
    return Case(kernel, cfg, epi, out, M, N, K, family, dtype, tuple(counts) if counts else None, gather, split_k, flags, ss_n, tuple(pad), wextra, bextra)


# ------------------------------------------------------------------------------------------------------------------ inputs
class Inputs:
    """CPU tensors of one case: A_buf / W_buf / resid_buf (the wide buffers, pads filled with data of their own) and their logical views A [tokens, K],
    W [E, Nw, K], resid [M, N]; bias [E, Nw + bextra]; gain [N]; row_ss [tokens, ss_n]; a_rows / offsets int32; row_eps; clamped (token ids)."""


_CYC = (3.4, -3.4, 0.2, -1.0, 1.7, -2.5, 0.05, -0.6)


def _seed(c):
    return (7919 * c.M + 104729 * c.N + 31 * c.K + 1009 * c.epi + 17 * FAMILIES.index(c.family) + 13 * c.ss_n + 5 * c.split_k + 3 * sum(c.pad)
            + (977 if c.gather else 0) + 7 * sum((i + 1) * n for i, n in enumerate(c.counts or ())) + (1 if c.dtype == F32 else 0)) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def _inputs(c):
    g = torch.Generator().manual_seed(_seed(c))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    pa, pw, pc, off = c.pad
    E, Nw, K, T = c.E, c.Nw, c.K, c.tokens
    inp = Inputs()
    wrows = Nw + c.wextra
    A_buf = rn(T, K + pa)
    W_buf = rn(E * wrows, K + pw) * K ** -0.5
    if c.family == "tails":
        # pre-activation ~ s[m] t[n]: a rank-one component along u (|u_k| = 1) plus noise; both cycles visit +-3.4, so every 8 x 8 block of the output
        # holds pre-activations near +-11.6, +-6 and 0
        u = torch.where(rn(K) >= 0, 1.0, -1.0).double()
        s = torch.tensor([_CYC[(3 * m + 1) % 8] for m in range(T)], dtype=torch.float64) * (1 + 0.05 * rn(T))
        A_buf[:, off:off + K] = s[:, None] * u + 0.2 * rn(T, K)
        for e in range(E):
            t = torch.tensor([_CYC[(5 * j + 3 * (j >= c.N) + e) % 8] for j in range(Nw)], dtype=torch.float64) * (1 + 0.05 * rn(Nw))
            W_buf[e * wrows: e * wrows + Nw, off:off + K] = t[:, None] * u / K + 0.2 * K ** -0.5 * rn(Nw, K)
    inp.clamped = ()
    inp.row_ss, inp.row_eps = None, 0.0
    if c.ss_n:
        inp.row_eps = CLAMP_EPS if c.family == "clamp" else SOFT_EPS
        row_ss = (0.5 + ru(T, c.ss_n)) * K / c.ss_n                                # a row norm of ~1
        if c.family == "clamp":
            inp.clamped = tuple(sorted({0, T // 2, T - 1}))
            for i, t in enumerate(inp.clamped):                                    # a tiny row of x: A = x * gain is tiny too, and its norm is under eps
                A_buf[t] *= 2.0 ** -12
                row_ss[t] *= 0.0 if i == 1 else 2.0 ** -26                          # (the middle one: an all-zero row, sqrt(0) = 0)
        inp.row_ss = row_ss.float()
    inp.A_buf, inp.W_buf = A_buf.to(c.dtype), W_buf.to(c.dtype)
    inp.A = inp.A_buf[:, off:off + K]
    inp.W = torch.stack([inp.W_buf[e * wrows: e * wrows + Nw, off:off + K] for e in range(E)])
    inp.bias = (0.1 + 0.9 * ru(E, c.b_estride)).float()
    inp.resid_buf = rn(c.M, c.ldr).float()
    inp.resid = inp.resid_buf[:, off:off + c.N]
    inp.gain = (1 + 0.1 * rn(c.N)).float()
    assert not bool((inp.gain == 1).all())
    inp.offsets = torch.tensor([0] + list(torch.tensor(c.counts).cumsum(0)), dtype=torch.int32) if c.counts else None
    inp.a_rows = None
    if c.gather:
        if c.flags & IDENTITY_ROWS:
            inp.a_rows = torch.cat([torch.arange(n) for n in c.counts]).int()
        else:
            inp.a_rows = (torch.arange(c.M) % T)[torch.randperm(c.M, generator=g)].int()   # every token twice (once when M is odd): one token, two experts
    if c.family == "clamp":
        assert c.ss_n and all(float(inp.row_ss[t].double().sum().sqrt()) * K ** -0.5 < inp.row_eps for t in inp.clamped)
    return inp


def inputs(c):
    return _inputs(c.data_key)


# ------------------------------------------------------------------------------------------------------------------ the reference
def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def dgelu64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def silu64(g):
    return g * torch.sigmoid(g)


def dsilu64(g):
    s = torch.sigmoid(g)
    return s * (1 + g * (1 - s))


def row_factor(row_ss, K, eps):
    """1 / max(sqrt(sum_j row_ss[token][j]) * K^-1/2, row_eps), per token."""
    return 1.0 / torch.clamp_min(f64(row_ss).sum(1).sqrt() * K ** -0.5, eps)


def gemm_ref(A, W, M, N, K, epi, bias=None, resid=None, a_rows=None, offsets=None, gain=None, row_ss=None, row_eps=0.0, split_k=1, group=64):
    """mode_gemm in fp64.  A [tokens, K]; W [E, Nw, K] and bias [E, >= Nw] per expert (E = 1 when ungrouped; Nw = 2 N for SWIGLU, the gate half from row
    N); resid [M, N]; a_rows int [M]; offsets int [E + 1]; gain [N]; row_ss [tokens, n].  Returns a dict: "C" (and "C2", "row_ss_out" for RESIDUAL_NORM,
    "slab" [split_k, M, N] for split_k > 1) with, for every output element, the magnitude sum under "S_" + name; "pre" / "S_pre" [M, Nw]: the value the
    activation is applied to (the accumulator times the row factor, plus bias) and its magnitude sum; "acc" [M, Nw]: the bare product; "rfac" [M]."""
    A, W = f64(A), f64(W)
    Nw = W.shape[1]
    rows = torch.arange(M) if a_rows is None else torch.as_tensor(a_rows).long()
    Ag = A[rows]
    eid = torch.zeros(M, dtype=torch.long) if offsets is None else torch.bucketize(torch.arange(M), torch.as_tensor(offsets).long()[1:], right=True)

    def product(k0, k1):
        acc, S = torch.zeros(M, Nw, dtype=torch.float64), torch.zeros(M, Nw, dtype=torch.float64)
        for e in range(W.shape[0]):
            sel = eid == e
            if bool(sel.any()):
                acc[sel] = Ag[sel, k0:k1] @ W[e, :, k0:k1].t()
                S[sel] = Ag[sel, k0:k1].abs() @ W[e, :, k0:k1].abs().t()
        return acc, S

    acc, S = product(0, K)
    out = dict(acc=acc, S_acc=S)
    if split_k > 1:
        assert epi == NONE and K % split_k == 0
        parts = [product(z * (K // split_k), (z + 1) * (K // split_k)) for z in range(split_k)]
        out["slab"], out["S_slab"] = torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])
    rfac = torch.ones(M, dtype=torch.float64) if row_ss is None else row_factor(row_ss, K, row_eps)[rows]
    out["rfac"] = rfac
    pre, Sp = acc * rfac[:, None], S * rfac[:, None]
    if epi in (BIAS, BIAS_GELU, SWIGLU):
        b = f64(bias)[eid, :Nw]
        pre, Sp = pre + b, Sp + b.abs()
    if epi in (RESIDUAL, RESIDUAL_NORM):
        r = f64(resid)
        pre, Sp = pre + r, Sp + r.abs()
    out["pre"], out["S_pre"] = pre, Sp
    if epi == BIAS_GELU:
        out["C"] = gelu64(pre)
    elif epi == SWIGLU:
        out["C"] = pre[:, :N] * silu64(pre[:, N:])
    else:
        out["C"] = pre
    out["S_C"] = Sp if epi != SWIGLU else None
    if epi == RESIDUAL_NORM:
        out["C2"] = pre * f64(gain)
        out["row_ss_out"] = pre.pow(2).reshape(M, N // group, group).sum(2)
    return out


def half_ulp_bf16(ref):
    """2^(floor(log2 |ref|) - 8): half the spacing of bf16 at the reference value."""
    _, e = torch.frexp(ref.abs())                                      # |ref| = m 2^e, m in [0.5, 1): floor(log2 |ref|) = e - 1
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 9))


def act_gap(epi, pre, N):
    """The reference-alone gap of an activation epilogue: fp32 torch on the CPU from the fp64 pre-activation against fp64, relative to the expression's
    magnitude.  Returns (gap, magnitude [M, N])."""
    p32 = pre.float()
    if epi == BIAS_GELU:
        y32, y64, mag = F.gelu(p32), gelu64(pre), 0.5 * pre.abs() * (1 + torch.erf(pre / math.sqrt(2)).abs())
    else:
        y32, y64 = p32[:, :N] * F.silu(p32[:, N:]), pre[:, :N] * silu64(pre[:, N:])
        mag = y64.abs()
    d = (y32.double() - y64).abs()
    gap = torch.where(d == 0, torch.zeros_like(d), d / mag)
    return (float(gap.max()) if gap.numel() else 0.0), mag


def bounds(ref, epi, N, K, out_bf16, operands=BF16, ss_n=0, gain=None, split_k=1, group=64):
    """Per-element bounds of every output of gemm_ref's dict (module docstring).  Returns (dict name -> bound, gap)."""
    kk = (K + 2 if operands == BF16 else K + 3) * U
    b, gap = {}, 0.0
    bpre = kk * ref["S_pre"]
    if ss_n:
        bpre = bpre + (ss_n + 6) * U * (ref["acc"] * ref["rfac"][:, None]).abs()                  # the row factor's own fp32 evaluation
    if epi == BIAS_GELU:
        gap, mag = act_gap(epi, ref["pre"], N)
        b["C"] = dgelu64(ref["pre"]).abs() * bpre + 4 * gap * mag
    elif epi == SWIGLU:
        gap, mag = act_gap(epi, ref["pre"], N)
        v, g = ref["pre"][:, :N], ref["pre"][:, N:]
        b["C"] = silu64(g).abs() * bpre[:, :N] + v.abs() * dsilu64(g).abs() * bpre[:, N:] + 4 * gap * mag
    else:
        b["C"] = bpre
    if epi == RESIDUAL_NORM:
        M = ref["C"].shape[0]
        b["C2"] = b["C"] * f64(gain).abs() + half_ulp_bf16(ref["C2"])
        b["row_ss_out"] = (2 * ref["C"].abs() * b["C"]).reshape(M, N // group, group).sum(2) + (group + 1) * U * ref["row_ss_out"]
    if out_bf16:
        b["C"] = b["C"] + half_ulp_bf16(ref["C"])
    if split_k > 1:
        b["slab"] = (K // split_k + 2) * U * ref["S_slab"]
        if out_bf16:
            b["slab"] = b["slab"] + half_ulp_bf16(ref["slab"])
        b["slab_sum"] = b["slab"].sum(0)
    return b, gap


@functools.lru_cache(maxsize=None)
def _reference(c):
    inp = _inputs(c)
    return gemm_ref(inp.A, inp.W, c.M, c.N, c.K, c.epi, inp.bias, inp.resid, inp.a_rows, inp.offsets, inp.gain, inp.row_ss if c.ss_n else None,
                    inp.row_eps, c.split_k, c.group)


def reference(c):
    """(reference dict, bound dict, gap) of a case; the reference is shared by every geometry and output dtype of the same data."""
    ref = _reference(c.data_key)
    b, gap = bounds(ref, c.epi, c.N, c.K, c.out == BF16, c.dtype, c.ss_n, inputs(c).gain, c.split_k, c.group)
    return ref, b, gap


def ratios(got, ref, bound, clamped_rows=()):
    """got: dict name -> CPU tensor ("C", "C2", "row_ss_out", "slab" [S, M, N]).  Returns [(name, worst err / bound, index)]; an element that is exactly
    right counts 0 whatever its bound.  The slab sum is formed here, in fp64 and slice order.  clamped_rows: reported row by row beside the rest."""
    out = []

    def one(name, g, r, b):
        err = (f64(g) - r).abs()
        q = torch.where(err == 0, torch.zeros_like(err), err / b)
        q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
        if q.numel():
            i = int(q.argmax())
            out.append((name, float(q.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), q.shape))))

    for name, g in got.items():
        if name == "slab":
            one("slab", g, ref["slab"], bound["slab"])
            one("slab_sum", f64(g).sum(0), ref["C"], bound["slab_sum"])
        else:
            one(name, g, ref[name], bound[name])
            if name == "C":
                for m in clamped_rows:
                    one(f"C[clamped row {m}]", g[m], ref[name][m], bound[name][m])
    return out


# ------------------------------------------------------------------------------------------------------------------ which kernel takes a case
def ring_accepts(c):
    """gemm_bf16_launch's own conditions (gemm_bf16.hip:475-476, 494-495) and the geometries' epilogues (launch_epi, gemm_bf16.hip:419-422)."""
    ok = c.K % 64 == 0 and c.N % 4 == 0 and c.lda % 8 == 0 and c.ldw % 8 == 0 and c.ldc % 4 == 0
    ok = ok and c.K % (64 * c.split_k) == 0 and (c.split_k == 1 or c.epi == NONE)
    if c.cfg == 14:
        ok = ok and c.epi != SWIGLU
    if c.cfg == 20:
        ok = ok and c.epi == NONE
    return ok and not (c.flags & SMALL_ROWS)


def takes_skinny(c):
    """The weight streamer: entered for M <= "gemm_skinny_rows" or under MODE_GEMM_SMALL_ROWS on the automatic geometry only (gemm_bf16.hip:507-508);
    gemm_bf16_skinny_launch's conditions (gemm_bf16_skinny.hip:545-548, 559-560)."""
    small = bool(c.flags & SMALL_ROWS)
    if c.cfg != 0 or not (c.M <= SKINNY_ROWS or small):
        return False
    if (c.ss_n or c.epi == RESIDUAL_NORM) and not small:
        return False
    if c.epi == RESIDUAL_NORM and c.N % 16:
        return False
    if c.epi in (RESIDUAL, RESIDUAL_NORM) and c.out == BF16:
        return False
    if small and c.counts and max(c.counts) > SKINNY_ROWS:                          # what the flag vouches for
        return False
    return c.K % (128 * c.split_k) == 0 and c.N % 4 == 0


def takes_mid(c):
    """The register-resident kernel: entered on the automatic geometry for M <= "gemm_mid_rows" (or "gemm_mid_rows_rn" for RESIDUAL_NORM) when the
    streamer did not take the shape (gemm_bf16.hip:512); gemm_bf16_mid_launch's conditions (gemm_bf16_skinny.hip:477-479)."""
    if c.cfg != 0 or c.flags & SMALL_ROWS or takes_skinny(c):
        return False
    if not (c.M <= MID_ROWS or (c.epi == RESIDUAL_NORM and c.M <= MID_ROWS_RN)):
        return False
    if c.counts or c.gather or c.split_k != 1 or c.K != 1024 or c.N % 64 or c.ss_n:
        return False
    return c.epi in (NONE, BIAS, RESIDUAL_NORM) and not (c.epi == RESIDUAL_NORM and c.out != F32)


def takes_pp(c, rows256):
    """The persistent ping-pong kernel under a forced "gemm_cfg" 17 / 18 (gemm_bf16.hip:516-518); gemm_bf16_pp_launch's conditions
    (gemm_bf16_pp.hip:527-538; the pointer alignments are the allocator's)."""
    if c.cfg != (18 if rows256 else 17):
        return False
    if rows256 and c.epi == SWIGLU:
        return False
    if c.epi not in (NONE, BIAS, SWIGLU):
        return False
    nout, S = (128 if c.epi == SWIGLU else 256), c.split_k
    if c.N % nout or c.K % (128 * S) or c.K // S < 128 or c.E > 8:
        return False
    if c.ldc % 8 or (S > 1 and c.split_stride % 8) or (c.c_off * (2 if c.out == BF16 else 4)) % 16:
        return False
    if c.ss_n and (c.ss_n > 16 or c.ss_n % 4):
        return False
    return c.b_estride % 4 == 0


def f32_kernel(c):
    """gemm_f32_launch's order (gemm_f32.hip:409-415): the dot kernel for N <= 16 and K >= 64, the GEMV under MODE_GEMM_SKINNY_OK for M <= 16, else MFMA."""
    vec_ok = c.K % 4 == 0 and c.lda % 4 == 0 and c.ldw % 4 == 0 and c.pad[3] % 4 == 0
    if c.N <= 16 and c.K >= 64 and vec_ok and not c.counts and c.epi != SWIGLU:
        return "f32-dot"
    if c.flags & SKINNY_OK and c.M <= 16 and not c.gather and not c.counts and vec_ok and c.epi in (NONE, BIAS, BIAS_GELU):
        return "f32-gemv"
    return "f32-mfma"


def kernel_of(c):
    """The kernel mode_gemm runs for a case, following gemm_bf16_launch's order: streamer, mid, ping-pong (forced), ring."""
    if c.dtype == F32:
        return "f32"
    assert ring_accepts(c._replace(cfg=0, flags=c.flags & ~SMALL_ROWS)), "refused by gemm_bf16_launch itself"
    if takes_skinny(c):
        return "stream"
    if c.flags & SMALL_ROWS:
        return "refused"
    if takes_mid(c):
        return "mid"
    if c.cfg in (17, 18):
        return "pp" if takes_pp(c, c.cfg == 18) else "ring"
    if c.cfg == 0:                                                      # pick_cfg (gemm_bf16.hip:439-457): the ping-pong kernel from 190 tiles on
        assert -(-c.M // 224) * max(c.N // 128, 1) * c.split_k < 190
        return "ring"
    return "ring" if ring_accepts(c) else "heuristic"


# ------------------------------------------------------------------------------------------------------------------ the case table
RING_CFGS = (1, 4, 6, 8, 13, 14)
RING_M, RING_N, RING_K = (1, 63, 64, 65, 127, 128, 129, 257), (4, 12, 60, 64, 68, 132, 260), (64, 128, 192)
RING_SWIGLU_N = (4, 60, 64, 68, 132)
LINEAR_EPIS = ((NONE, F32), (NONE, BF16), (BIAS, F32), (BIAS, BF16), (RESIDUAL, F32))
ACT_FAMILIES = ("soft", "tails")


def _epi_sweep(kernel, cfg, M, N, K, swiglu=True, linear=LINEAR_EPIS, gelu=True, **kw):
    out = [case(kernel, cfg, e, o, M, N, K, **kw) for e, o in linear]
    if gelu:
        out += [case(kernel, cfg, BIAS_GELU, o, M, N, K, family=f, **kw) for o in (F32, BF16) for f in ACT_FAMILIES]
    if swiglu:
        out += [case(kernel, cfg, SWIGLU, o, M, N, K, family=f, **kw) for o in (F32, BF16) for f in ACT_FAMILIES]
    return out


def ring_shapes():
    """One sweep over M at a ragged N (N % 8 == 4: the 8-byte tail store), one over N at a ragged M, one over K (64: a single K-step)."""
    return [(M, 68, 128) for M in RING_M] + [(65, N, 128) for N in RING_N if N != 68] + [(65, 68, K) for K in RING_K if K != 128]


def ring_cases(cfg):
    if cfg == 20:
        return [case("ring", 20, NONE, o, M, N, K) for M, N, K in ring_shapes() for o in (F32, BF16)]
    out = []
    for M, N, K in ring_shapes():
        out += _epi_sweep("ring", cfg, M, N, K, swiglu=False)
    if cfg != 14:
        for N in RING_SWIGLU_N:
            out += [case("ring", cfg, SWIGLU, o, 65, N, 128, family=f) for o in (F32, BF16) for f in ACT_FAMILIES]
    return out


def bit_identity_cases():
    """One ragged shape per epilogue, dense leading dimensions: every geometry against geometry 1."""
    M, N, K, dense = 129, 68, 192, (0, 0, 0, 0)
    out = _epi_sweep("ring", 1, M, N, K, swiglu=True, pad=dense)
    out = [c for c in out if c.family != "soft" or c.epi not in (BIAS_GELU, SWIGLU)]
    return out + [case("ring", 1, RESIDUAL_NORM, F32, M, 128, K, pad=dense)]


def other_geometries(c):
    """The geometries a bit-identity case is repeated on: every ring geometry that has its epilogue."""
    return [g for g in RING_CFGS[1:] + (20,) if ring_accepts(c._replace(cfg=g))]


def residual_norm_cases(cfg):
    """cfg 0: the mid kernel (K = 1024; up to 32 rows the streamer declines RESIDUAL_NORM without MODE_GEMM_SMALL_ROWS); else that ring geometry."""
    if cfg == 0:
        return [case("mid", 0, RESIDUAL_NORM, F32, M, N, 1024) for M in (1, 31, 32, 33, 100) for N in (64, 192)]
    return [case("ring", cfg, RESIDUAL_NORM, F32, M, N, 128) for M in (1, 65, 129) for N in (64, 128, 192)]


STREAM_M, STREAM_K, STREAM_N = (1, 2, 16, 17, 32), (128, 384), (4, 20, 64, 132)


def stream_cases(K):
    out = []
    for M in STREAM_M:
        for N in STREAM_N:
            out += _epi_sweep("stream", 0, M, N, K)
    return out


def stream_small_rows_cases():
    out = [case("stream", 0, RESIDUAL_NORM, F32, M, N, 128, flags=SMALL_ROWS) for M in (1, 17, 32) for N in (16, 48, 80)]
    for ss_n, fam in ((3, "soft"), (3, "tails"), (6, "clamp"), (6, "soft"), (18, "tails"), (18, "clamp"), (70, "soft"), (70, "tails")):
        out += [case("stream", 0, SWIGLU, o, 17, 20, 128, family=fam, flags=SMALL_ROWS, ss_n=ss_n) for o in (F32, BF16)]
    seg = (0, 1, 32, 5)
    out += [case("stream", 0, e, o, 0, 20, 128, counts=seg, gather=True, flags=SMALL_ROWS, wextra=3, bextra=4) for e, o in ((NONE, BF16), (BIAS, F32))]
    out += [case("stream", 0, SWIGLU, BF16, 0, 20, 128, family=f, counts=seg, gather=True, flags=SMALL_ROWS, ss_n=6, wextra=3, bextra=4)
            for f in FAMILIES]
    out += [case("stream", 0, NONE, BF16, 0, 20, 256, counts=seg, flags=SMALL_ROWS, split_k=2, wextra=3)]
    return out


def mid_cases():
    return [case("mid", 0, e, o, M, N, 1024) for M in (33, 64, 65, 128) for N in (64, 192) for e in (NONE, BIAS) for o in (F32, BF16)]


def mid_boundary_case(out=F32):
    return case("ring", 0, BIAS, out, 129, 64, 1024)                     # one row past "gemm_mid_rows": the ring; its first 128 rows, launched alone, the mid kernel


PP_M = {17: (223, 224, 225), 18: (255, 256, 257)}


def pp_cases(cfg):
    Ms = PP_M[cfg]
    out = [case("pp", cfg, e, o, M, N, K) for M in Ms for N in (256, 512) for K in (128, 256) for e in (NONE, BIAS) for o in (F32, BF16)]
    out += [case("pp", cfg, NONE, o, Ms[2], 256, 256, split_k=2) for o in (F32, BF16)]                     # K / split_k at its minimum of 128
    seg = (0, 1, Ms[1], Ms[2])
    out += [case("pp", cfg, e, o, 0, 256, 128, counts=seg, bextra=8, wextra=3) for e, o in ((NONE, BF16), (BIAS, F32), (BIAS, BF16))]
    if cfg == 17:
        out += [case("pp", 17, SWIGLU, o, M, N, K, family=f) for M in Ms for N in (128, 256) for K in (128, 256) for o in (F32, BF16) for f in ACT_FAMILIES]
        for ss_n in (4, 16):
            out += [case("pp", 17, SWIGLU, BF16, 0, 128, 128, family=f, counts=seg, gather=True, ss_n=ss_n, bextra=8) for f in FAMILIES]
    return out


def pp_identity_case():
    return case("pp", 17, SWIGLU, BF16, 0, 128, 128, counts=(0, 1, 224, 225), gather=True, flags=IDENTITY_ROWS | UNIFORM_GROUPS, ss_n=4, bextra=8)


GROUPED_SEGMENTS = ((0, 1, 128, 129), (130, 0, 0, 0))


def grouped_ring_cases(cfg):
    """The expert MLP's two GEMMs on a ring geometry: the gathered SwiGLU up-projection with row_ss by token, and the NONE down-projection (rows already
    sorted) in bf16 K-slice slabs.  w_expert_stride is three rows more than one matrix."""
    out = []
    for seg in GROUPED_SEGMENTS:
        if cfg not in (14, 20):
            out += [case("ring", cfg, SWIGLU, BF16, 0, 68, 128, family=f, counts=seg, gather=True, ss_n=n, wextra=3, bextra=4)
                    for f, n in (("soft", 2), ("tails", 2), ("clamp", 16), ("tails", 16))]
        out += [case("ring", cfg, NONE, BF16, 0, 68, 256, counts=seg, split_k=S, wextra=3) for S in (2, 4)]
        if cfg != 20:
            out += [case("ring", cfg, BIAS, F32, 0, 68, 64, counts=seg, gather=True, wextra=3, bextra=4)]
    return out


STRIDED = (64, 8, 8, 8)                                                  # lda = K + 64, ldw = K + 8, ldc = N + 8, operands 8 columns into their buffers


def strided_cases():
    out = [case("ring", 1, RESIDUAL, F32, 65, 68, 128, pad=STRIDED), case("ring", 1, BIAS, BF16, 65, 68, 128, pad=STRIDED),
           case("ring", 4, RESIDUAL_NORM, F32, 65, 64, 128, pad=STRIDED), case("ring", 1, SWIGLU, BF16, 65, 68, 128, family="tails", pad=STRIDED),
           case("pp", 17, BIAS, BF16, 225, 256, 128, pad=STRIDED), case("pp", 18, NONE, F32, 257, 256, 128, pad=STRIDED),
           case("stream", 0, RESIDUAL, F32, 17, 20, 128, pad=STRIDED), case("stream", 0, BIAS, BF16, 17, 20, 128, pad=STRIDED),
           case("stream", 0, RESIDUAL_NORM, F32, 17, 48, 128, flags=SMALL_ROWS, pad=STRIDED),
           case("mid", 0, BIAS, BF16, 65, 64, 1024, pad=STRIDED), case("mid", 0, RESIDUAL_NORM, F32, 65, 64, 1024, pad=STRIDED)]
    return out


F32_M, F32_N, F32_K = (1, 15, 16, 17, 65), (1, 2, 6, 130), (1, 7, 30, 100, 1000)


def f32_cases(flags, K):
    out = []
    for M, N in ((M, N) for M in F32_M for N in F32_N):
        out += [case("f32", 0, e, F32, M, N, K, dtype=F32, flags=flags) for e in (NONE, BIAS)]
        out += [case("f32", 0, BIAS_GELU, F32, M, N, K, family=f, dtype=F32, flags=flags) for f in ACT_FAMILIES]
    return out


def all_cases():
    out = []
    for cfg in RING_CFGS + (20,):
        out += ring_cases(cfg) + grouped_ring_cases(cfg)
    for cfg in (0,) + RING_CFGS:
        out += residual_norm_cases(cfg)
    out += [c._replace(cfg=g) for c in bit_identity_cases() for g in [1] + other_geometries(c)] + stream_cases(128) + stream_cases(384) + stream_small_rows_cases() + mid_cases() + [mid_boundary_case(F32), mid_boundary_case(BF16)]
    out += pp_cases(17) + pp_cases(18) + [pp_identity_case()] + strided_cases() + [c for K in F32_K for f in (0, SKINNY_OK) for c in f32_cases(f, K)]
    return out


# ------------------------------------------------------------------------------------------------------------------ report
class Report:
    """Worst err / bound per (path, epilogue, output) of one test, printed at its end; a ratio above 1 fails the test."""

    def __init__(self, what):
        self.what, self.worst, self.failed, self.gaps = what, collections.OrderedDict(), [], collections.OrderedDict()

    def add(self, c, rs, gap=0.0):
        path = f32_kernel(c) if c.dtype == F32 else c.kernel
        if c.epi in (BIAS_GELU, SWIGLU):
            key = (path, EPI_NAME[c.epi], c.family)
            self.gaps[key] = max(self.gaps.get(key, 0.0), gap)
        for name, q, idx in rs:
            key = (path, EPI_NAME[c.epi], ("bf16 " if c.out == BF16 else "f32 ") + name.split("[")[0])
            if key not in self.worst or q > self.worst[key][0]:
                self.worst[key] = (q, f"{c.tag} {name}{list(idx)}")
            if not q <= 1.0:
                self.failed.append(f"{c.tag}: {name}{list(idx)} err / bound = {q:.3g}")

    def fail(self, msg):
        self.failed.append(msg)

    def close(self):
        for (path, epi, name), (q, where) in self.worst.items():
            print(f"{self.what} | {path} {epi} {name}: worst err / bound {q:.3g} ({where})")
        for (path, epi, fam), gap in self.gaps.items():
            print(f"{self.what} | {path} {epi} {fam}: reference-alone gap {gap:.3g}")
        assert not self.failed, "\n".join(self.failed[:40]) + f"\n({len(self.failed)} failures)"
