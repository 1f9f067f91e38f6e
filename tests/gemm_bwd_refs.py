"""The fp64 reference of mode_gemm's backward-pass layouts (include/mode_hip.h: MODE_GEMM_W_KN, MODE_GEMM_A_KM, k_group_offsets, w_rows in taps), the
per-element bound, the input families, the launchers' predicates and the case table, shared by tests/test_gpu_gemm_bwd_edges.py (which launches the
kernels of gemm_bf16_tr.hip, gemm_bf16_pptr.hip and gemm_f32.hip) and tests/test_gemm_bwd_references.py (which validates all of this without a GPU).
U, f64, half_ulp_bf16, bounds(..., NONE, ...), ratios and Report are the forward family's (tests/gemm_refs.py), unchanged.

The operation, from the header.  Output part z (a K-slice slab, a K group, or the one product) is C_z [M, N]:
  dgrad    C[m, :] = A[m, k0:k1] @ W_e[k0:k1, :]      A [M, K]; W_e [K, N] = W + e * w_expert_stride, e the expert whose segment holds row m;
                                                       slab z of split_k covers k0 = z K / split_k .. k1 = (z + 1) K / split_k
  wgrad    C_z = A[kb:ke, :M]^T @ W[rows[kb:ke], :N]  A [R, M], W [Rw, .]; [kb, ke) = [off[z], off[z + 1]) (or [0, K)); rows = the identity, or w_rows
                                                       (a negative index is a zero row); tap t reads table w_rows + t * w_rows_tap_stride and
                                                       writes output columns [t * tap_cols, (t + 1) * tap_cols) from W's columns [0, tap_cols)
  f32 lay 1  A^T @ W^T, W [N, K]      f32 lay 2  A @ W, W [K, N]      f32 lay 3  A^T @ W, W [K, N]      (lay 1 and 3 take K groups)
An empty range gives exactly +0.0.

The bound is the forward family's: fp32 output (k + 2) u S with S = sum |a| |w| over the element's own reduction range and k its length (ke - kb, or
K / split_k per slab; k + 3 for fp32 operands), bf16 output + half a bf16 unit at |ref|, the slab sum under the sum of the slab bounds.  No term was
added after a launch."""
import collections
import functools

import torch

from gemm_refs import BF16, F32, NONE, U, Report as _Report, bounds, f64, half_ulp_bf16, ratios  # noqa: F401  (re-exported)

W_KN, A_KM = 2, 4                                                       # MODE_GEMM_* (checked against _lib by test_gemm_bwd_references.py)
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
FAMILIES = ("soft", "spiky", "poison", "poison_max")
BF16_MAX = 3.3895313892515355e38                                         # the largest finite bf16
LAYOUTS = ("dgrad", "wgrad", "f32 lay 1", "f32 lay 2", "f32 lay 3")
OUTS = (F32, BF16)

# ------------------------------------------------------------------------------------------------------------------ cases
_Case = collections.namedtuple("Case", "layout kernel cfg out M N K family counts kranges split_k w_rows taps tap_cols pad wextra path")


class Case(_Case):
    """One launch.  layout: LAYOUTS; kernel: "ring" / "pptr" / "f32" - the kernel the case is meant for; cfg: "gemm_tr_cfg"; counts: expert segment
    lengths (dgrad; M is their sum); kranges = (off0, lengths, tail): the K groups start at row off0 and end `tail` rows before the end of the buffers
    (K, the row count, is their total); w_rows: "none" / "gathered" / "taps"; pad = (pa, pw, pc, off): lda = cols + pa, ldw = cols + pw (fp32 operands: rounded up to a multiple of 4), ldc = N + pc, A / W
    start `off` columns into their buffers (fp32 operands: off / 2) and C `off` columns (fp32 output: off / 2): 16 bytes each; wextra: rows between two
    experts' matrices; path: what the launcher must make of the case - the ring geometry 1..5, 6 for the ping-pong kernel, or the fp32 kernel's
    "vec" / "scalar" + " small" / " 64"."""
    __slots__ = ()

    dtype = property(lambda s: F32 if s.layout.startswith("f32") else BF16)
    a_km = property(lambda s: s.layout in ("wgrad", "f32 lay 1", "f32 lay 3"))
    w_kn = property(lambda s: s.layout != "f32 lay 1")
    flags = property(lambda s: (A_KM if s.a_km else 0) | (W_KN if s.w_kn else 0))
    E = property(lambda s: len(s.counts) if s.counts else 1)
    G = property(lambda s: len(s.kranges[1]) if s.kranges else 1)
    Z = property(lambda s: s.G if s.a_km else s.split_k)                # output parts
    a_cols = property(lambda s: s.M if s.a_km else s.K)
    a_rows_n = property(lambda s: s.K if s.a_km else s.M + 2)           # dgrad: two spare rows behind the last segment
    w_cols = property(lambda s: (s.tap_cols or s.N) if s.w_kn else s.K)
    Rw = property(lambda s: s.K if s.w_rows == "none" else s.K // 2 + 4)    # gathered: fewer rows than indices (repeats); the last one is never named
    w_rows_n = property(lambda s: (s.Rw if s.a_km else s.E * (s.K + s.wextra)) if s.w_kn else s.N)
    op_off = property(lambda s: s.pad[3] if s.dtype == BF16 else s.pad[3] // 2)
    c_off = property(lambda s: s.pad[3] if s.out == BF16 else s.pad[3] // 2)
    lda = property(lambda s: s._ld(s.a_cols + s.pad[0]))
    ldw = property(lambda s: s._ld(s.w_cols + s.pad[1]))
    ldc = property(lambda s: s.N + s.pad[2])
    w_estride = property(lambda s: (s.K + s.wextra) * s.ldw)
    part_stride = property(lambda s: (s.M + 1) * s.ldc)                 # c_group_stride / split_stride: one untouched row between two parts
    tap_stride = property(lambda s: s.K + 3)                            # w_rows_tap_stride: larger than the row count

    def _ld(self, n):
        """fp32 operands: the next multiple of 4 (gemm_f32.hip:419 wants 16-byte rows on the backward layouts whatever the logical width)."""
        return n if self.dtype == BF16 else -(-n // 4) * 4

    @property
    def offsets(self):
        """k_group_offsets as a list, or None."""
        if not self.kranges:
            return None
        o = [self.kranges[0]]
        for n in self.kranges[1]:
            o.append(o[-1] + n)
        return o

    @property
    def ranges(self):
        """[(kb, ke)] of the output parts of an A_KM layout."""
        o = self.offsets
        return [(0, self.K)] if o is None else list(zip(o[:-1], o[1:]))

    @property
    def tag(self):
        t = f"{self.kernel} cfg={self.cfg} {self.layout} {'bf16' if self.out == BF16 else 'f32'} M={self.M} N={self.N} K={self.K} {self.family}"
        if self.counts:
            t += f" segments={self.counts}"
        if self.kranges:
            t += f" kgroups={self.kranges}"
        if self.split_k > 1:
            t += f" split_k={self.split_k}"
        if self.w_rows != "none":
            t += f" w_rows={self.w_rows}" + (f" {self.taps}x{self.tap_cols}" if self.tap_cols else "")
        return t + f" pad={self.pad}"

    @property
    def data_key(self):
        """What the inputs and the reference depend on: everything but the kernel, the geometry and the output dtype."""
        return self._replace(kernel="", cfg=0, out=F32, path=None)


DEFAULT_PAD, STRIDED = (8, 8, 8, 0), (64, 8, 8, 8)


def case(layout, kernel, cfg, out, M, N, K=0, family="soft", counts=None, kranges=None, split_k=1, w_rows="none", taps=1, tap_cols=0, pad=DEFAULT_PAD,
         wextra=0, path=None):
    assert layout in LAYOUTS and family in FAMILIES
    if counts:
        M = sum(counts)
    if kranges:
        kranges = (kranges[0], tuple(kranges[1]), kranges[2])
        K = kranges[0] + sum(kranges[1]) + kranges[2]
    if tap_cols:
        N = taps * tap_cols
    if path is None:
        path = 6 if kernel == "pptr" else cfg
    return Case(layout, kernel, cfg, out, M, N, K, family, tuple(counts) if counts else None, kranges, split_k, w_rows, taps, tap_cols, tuple(pad), wextra, path)


# ------------------------------------------------------------------------------------------------------------------ inputs
class Inputs:
    """CPU tensors of one case: A_buf [a_rows_n, lda] and W_buf [w_rows_n, ldw] (the wide buffers) with their logical views A and W (dgrad: W
    [E, K, N]); seg = expert_offsets, koffs = k_group_offsets, idx = the index tables [taps, tap_stride] (int32) or None."""


def _seed(c):
    return (7919 * c.M + 104729 * c.N + 31 * c.K + 1009 * LAYOUTS.index(c.layout) + 17 * FAMILIES.index(c.family) + 5 * c.split_k + 3 * sum(c.pad)
            + 977 * ("none", "gathered", "taps").index(c.w_rows) + 7 * sum((i + 1) * n for i, n in enumerate(c.counts or ()))
            + 11 * sum((i + 2) * n for i, n in enumerate(c.kranges[1] if c.kranges else ())) + 13 * c.taps) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def _inputs(c):
    g = torch.Generator().manual_seed(_seed(c))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    inp = Inputs()
    off = c.op_off
    kred = max(c.kranges[1]) if c.kranges else c.K // c.split_k           # N(0, 1) against N(0, 1 / k)
    A_buf, W_buf = rn(c.a_rows_n, c.lda), rn(c.w_rows_n, c.ldw) * max(kred, 1) ** -0.5
    if c.family == "spiky":                                               # ~1 % of the elements x 2^6, ~10 % x 2^-8
        for t in (A_buf, W_buf):
            r = ru(*t.shape)
            t *= torch.where(r < 0.01, 64.0, 1.0) * torch.where((r >= 0.01) & (r < 0.11), 2.0 ** -8, 1.0)
    inp.idx = None
    if c.w_rows != "none":
        idx = torch.randint(0, c.Rw - 1, (c.taps, c.tap_stride), generator=g, dtype=torch.int32)      # row Rw - 1 is never named
        idx[ru(c.taps, c.tap_stride) < 0.15] = -1
        inp.idx = idx
    if c.family in ("poison", "poison_max"):
        nan = float("nan")
        wbad = nan if c.family == "poison" else BF16_MAX
        lo, hi = (c.offsets[0], c.offsets[-1]) if c.kranges else (0, c.K)
        if c.a_km:
            A_buf[:lo] = nan; A_buf[hi:] = nan                             # rows of A outside [off[0], off[G])
            if c.layout == "f32 lay 1":
                W_buf[:, :off + lo] = wbad; W_buf[:, off + hi:] = wbad     # W [N, K]: its K index is the column
            elif inp.idx is None:
                W_buf[:lo] = wbad; W_buf[hi:] = wbad
            else:                                                         # every row no index of a range names; indices outside the ranges name row Rw - 1
                inp.idx[:, :lo] = c.Rw - 1; inp.idx[:, hi:] = c.Rw - 1
                named = torch.zeros(c.Rw, dtype=torch.bool)
                live = inp.idx[:, lo:hi].reshape(-1)
                named[live[live >= 0].long()] = True
                W_buf[~named] = wbad
        else:
            A_buf[c.M:] = nan                                             # rows behind the last segment
            for e in range(c.E):                                          # rows between two experts' matrices
                W_buf[e * (c.K + c.wextra) + c.K: (e + 1) * (c.K + c.wextra)] = wbad
        A_buf[:, :off] = nan; A_buf[:, off + c.a_cols:] = nan              # every pad column of every operand
        W_buf[:, :off] = nan; W_buf[:, off + c.w_cols:] = nan
    inp.A_buf, inp.W_buf = A_buf.to(c.dtype), W_buf.to(c.dtype)
    inp.A = inp.A_buf[:, off:off + c.a_cols]
    Wv = inp.W_buf[:, off:off + c.w_cols]
    inp.W = torch.stack([Wv[e * (c.K + c.wextra): e * (c.K + c.wextra) + c.K] for e in range(c.E)]) if c.layout == "dgrad" else Wv
    inp.seg = torch.tensor([0] + list(torch.tensor(c.counts).cumsum(0)), dtype=torch.int32) if c.counts else None
    inp.koffs = torch.tensor(c.offsets, dtype=torch.int32) if c.kranges else None
    return inp


def inputs(c):
    return _inputs(c.data_key)


# ------------------------------------------------------------------------------------------------------------------ the reference
DEFECTS = ("k_late", "k_drop_last", "k_past", "prev_group", "neg_as_row0", "tap0_table", "tap_swap", "slab_range", "next_expert", "transposed",
           "lay1_as_3", "truncate")


def applies(defect, c):
    """Can `defect` be stated for the case at all (and, for truncate, is the accumulation term well under the bf16 half unit)."""
    nonempty = any(ke > kb for kb, ke in c.ranges) if c.a_km else True
    return {
        "k_late": nonempty,
        "k_drop_last": nonempty,
        # a row past the range exists: a K group that ends before the buffers do, or a K-slice that is not the last
        "k_past": (c.a_km and any(ke < c.K for kb, ke in c.ranges)) or (not c.a_km and c.split_k > 1),
        "prev_group": c.a_km and c.G > 1 and len(set(c.ranges)) > 1,
        "neg_as_row0": c.w_rows != "none" and nonempty,
        "tap0_table": c.taps > 1 and nonempty,
        "tap_swap": c.taps > 1 and nonempty,
        "slab_range": c.split_k > 1,
        "next_expert": bool(c.counts) and any(n > 0 for n in c.counts[:-1]),
        "transposed": c.M == c.N and nonempty,
        "lay1_as_3": c.layout == "f32 lay 1" and c.N == c.K and not c.kranges,
        "truncate": c.out == BF16 and c.M * c.N >= 1024 and (max(c.kranges[1]) if c.kranges else c.K) <= 256 and nonempty,
    }[defect]


def _w_rows_of(c, inp, kb, ke, defect):
    """W's rows [ke - kb, N] of the range [kb, ke) of an A_KM layout in fp64: the identity, or through the index tables, tap by tap."""
    W = f64(inp.W)
    if c.layout == "f32 lay 1":
        return (W[:, kb:ke].t() if defect != "lay1_as_3" else f64(inp.W_buf)[kb:ke, c.op_off:c.op_off + c.N])
    if inp.idx is None:
        return W[kb:ke, :c.N]
    blocks = []
    for t in range(c.taps):
        rows = inp.idx[0 if defect == "tap0_table" else t, kb:ke].long()
        Wt = W[rows.clamp_min(0)]
        if defect != "neg_as_row0":
            Wt = torch.where((rows >= 0)[:, None], Wt, torch.zeros_like(Wt))
        blocks.append(Wt[:, :c.tap_cols or c.N])
    if defect == "tap_swap":
        blocks[0], blocks[1] = blocks[1], blocks[0]
    return torch.cat(blocks, 1)


def gemm_bwd_ref(c, inp, defect=None):
    """The descriptor in fp64.  Returns (C [Z, M, N], S [Z, M, N], k [Z]): the parts, their magnitude sums sum |a| |w| and the lengths of their
    reduction ranges.  defect: one of DEFECTS - the same descriptor read wrongly (tests of the bound's power); "truncate" is applied by the caller."""
    A = f64(inp.A)
    Cs, Ss, ks = [], [], []
    if c.a_km:
        rng = c.ranges
        for z, (kb, ke) in enumerate(rng):
            n = ke - kb
            if defect == "prev_group" and z > 0:
                kb, ke = rng[z - 1]
            if defect == "k_late" and ke > kb:
                kb += 1
            if defect == "k_drop_last" and ke > kb:
                ke -= 1
            if defect == "k_past" and ke < c.K:
                ke += 1
            a, w = A[kb:ke, :c.M].t(), _w_rows_of(c, inp, kb, ke, defect)
            Cs.append(a @ w); Ss.append(a.abs() @ w.abs()); ks.append(n)
    else:
        W = f64(inp.W) if c.layout == "dgrad" else f64(inp.W)[None]
        seg = inp.seg.tolist() if c.counts else [0, c.M]
        ksz = c.K // c.split_k
        for z in range(c.split_k):
            k0, k1 = z * ksz, (z + 1) * ksz
            if defect == "slab_range" and z == 1:
                k0, k1 = 0, ksz
            if defect == "k_late":
                k0 += 1
            if defect == "k_drop_last":
                k1 -= 1
            if defect == "k_past" and k1 < c.K:
                k1 += 1
            Cz, Sz = torch.zeros(c.M, c.N, dtype=torch.float64), torch.zeros(c.M, c.N, dtype=torch.float64)
            for e in range(c.E):
                r0, r1 = seg[e], seg[e + 1]
                we = W[e + 1 if defect == "next_expert" and e + 1 < c.E else e]
                Cz[r0:r1] = A[r0:r1, k0:k1] @ we[k0:k1, :c.N]
                Sz[r0:r1] = A[r0:r1, k0:k1].abs() @ we[k0:k1, :c.N].abs()
            Cs.append(Cz); Ss.append(Sz); ks.append(ksz)
    Cs, Ss = torch.stack(Cs), torch.stack(Ss)
    if defect == "transposed":
        Cs = Cs.transpose(1, 2).contiguous()
    return Cs, Ss, ks


Ref = collections.namedtuple("Ref", "C S k total")


@functools.lru_cache(maxsize=None)
def _reference(c):
    inp = _inputs(c)
    Cs, Ss, ks = gemm_bwd_ref(c, inp)
    total = None
    if c.split_k > 1:                                                    # the whole product, for the slab sum
        one = gemm_bwd_ref(c._replace(split_k=1), inp)
        total = one[0][0]
    return Ref(Cs, Ss, ks, total)


def reference(c):
    """(Ref, bound [Z, M, N]) of a case; the reference is shared by every kernel, geometry and output dtype of the same data."""
    ref = _reference(c.data_key)
    b = torch.stack([bounds(dict(S_pre=ref.S[z], C=ref.C[z]), NONE, c.N, ref.k[z], c.out == BF16, c.dtype)[0]["C"] for z in range(c.Z)])
    return ref, b


def to_out(t, out, truncate=False):
    """Stored as the output dtype: round to nearest even, or (the defect) by truncation."""
    if out == F32:
        return t.float()
    if truncate:
        return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)
    return t.float().to(BF16)


def wrong_reference(c, defect):
    """[Z, M, N] fp64: the descriptor read with `defect`; truncate: the right reference stored to bf16 by truncation."""
    if defect == "truncate":
        return to_out(reference(c)[0].C, BF16, truncate=True).double()
    return gemm_bwd_ref(c, inputs(c), defect)[0]


def part_ratios(got, ref_C, bound, total=None):
    """got [Z, M, N] (CPU) against ref_C [Z, M, N] under bound: [(name, worst err / bound, index)] per part through gemm_refs.ratios, plus the slab sum
    (fp64, slice order) against `total` under the sum of the slab bounds."""
    out = []
    for z in range(ref_C.shape[0]):
        out += [(f"part {z} {n}", q, i) for n, q, i in ratios({"C": got[z]}, {"C": ref_C[z]}, {"C": bound[z]})]
    if total is not None:
        out += [("slab_sum", q, i) for _, q, i in ratios({"C": f64(got).sum(0)}, {"C": total}, {"C": bound.sum(0)})]
    return out


def worst(rs):
    return max((q for _, q, _ in rs), default=0.0)


# ------------------------------------------------------------------------------------------------------------------ launcher predicates
def tr_status(c, a_rows=False, expert_offsets=None, k_groups=None, flags=None):
    """gemm_bf16_tr_launch's refusals (gemm_bf16_tr.hip:528-540, 551-553) for a bf16 case; the keyword arguments state descriptor fields a Case cannot
    (an a_rows gather; expert_offsets / k_group_offsets on the layout that does not take them; other flags)."""
    flags = c.flags if flags is None else flags
    a_km = bool(flags & A_KM)
    eo = bool(c.counts) if expert_offsets is None else expert_offsets
    kg = bool(c.kranges) if k_groups is None else k_groups
    if not flags & W_KN:
        return BAD_ARG
    if a_rows:
        return UNSUPPORTED
    if c.split_k > 1 and (a_km or c.K % (64 * c.split_k)):
        return UNSUPPORTED
    if c.N % 8 or c.N < 8 or c.lda % 8 or c.ldw % 8 or c.ldc % (8 if c.out == BF16 else 4):
        return UNSUPPORTED
    if a_km:
        if c.M % 8 or c.M < 8 or eo:
            return UNSUPPORTED
    elif c.K % 64 or c.K <= 0 or kg or c.w_rows != "none":
        return UNSUPPORTED
    if c.tap_cols and (not a_km or c.w_rows == "none" or c.tap_cols % 64 or c.N % c.tap_cols):
        return UNSUPPORTED
    return OK


def pptr_takes(c):
    """pptr_plan under a forced "gemm_tr_cfg" 6 (gemm_bf16_pptr.hip:420-447); the operands' and C's 16-byte alignment follows from their column offsets."""
    if c.dtype != BF16 or c.w_rows != "none" or c.N % 256 or c.ldc % 4 or c.lda % 8 or c.ldw % 8:
        return False
    if (c.op_off * 2) % 16 or (c.c_off * (2 if c.out == BF16 else 4)) % 16:
        return False
    if c.a_km:
        return not (c.M % 256 or c.M <= 0 or c.split_k > 1 or c.counts or c.K <= 0) and c.K * c.lda * 2 < 2 ** 31 and c.K * c.ldw * 2 < 2 ** 31
    S = c.split_k
    if c.K % (128 * S) or c.K // S < 128 or c.kranges or c.M <= 0 or c.E > 8:
        return False
    return not (S > 1 and c.part_stride % 4)


def ring_geometry(c):
    """The ring geometry gemm_bf16_tr_launch runs (gemm_bf16_tr.hip:562-568): the automatic choice for "gemm_tr_cfg" 0, 6 and 7, then the re-routing of
    gathered rows (two-slot rings only) and of taps that are no multiple of 128 columns."""
    groups = c.G if c.a_km else 1
    t128 = -(-c.M // 128) * -(-c.N // 128) * groups
    cfg = 0 if c.cfg >= 6 else c.cfg
    gathered = c.w_rows != "none"
    if cfg == 0:
        cfg = 5 if c.a_km and t128 >= 768 else (1 if t128 * c.split_k >= 448 or gathered else 2)
    if gathered and cfg in (2, 3):
        cfg = 1
    if c.tap_cols and c.tap_cols % 128 and cfg in (1, 3, 5):
        cfg = 4
    return cfg


def f32_path(c):
    """gemm_f32_launch's two switches on the backward layouts (gemm_f32.hip:434-441): float4 global loads and the 32 x 32 tile."""
    tiles64 = -(-c.M // 64) * -(-c.N // 64) * c.G
    vec = (not c.a_km or c.M % 4 == 0) and (not c.w_kn or c.N % 4 == 0)
    return ("vec" if vec else "scalar") + (" small" if tiles64 <= 160 else " 64")


def f32_status(c):
    """gemm_f32_launch's refusals on the backward layouts (gemm_f32.hip:417-421)."""
    if c.lda % 4 or c.ldw % 4 or (c.op_off * 4) % 16 or (not c.a_km and c.K % 4) or c.K <= 0 or c.split_k > 1 or c.counts:
        return UNSUPPORTED
    return OK


def path_of(c):
    """(kernel, path) mode_gemm makes of a case."""
    if c.dtype == F32:
        return ("f32", f32_path(c)) if f32_status(c) == OK else ("refused", None)
    if tr_status(c) != OK:
        return "refused", None
    if c.cfg == 6 and pptr_takes(c):
        return "pptr", 6
    assert c.cfg != 0, "the table forces every geometry"
    return "ring", ring_geometry(c)


# ------------------------------------------------------------------------------------------------------------------ the case table
RING_CFGS = (1, 2, 3, 4, 5)                                              # 128/NS2, 64/NS3, 128/NS3, 64/NS2, 128/NS1
GROUPED_SEGMENTS = ((0, 1, 128, 129), (130, 0, 0, 0))
RING_KG = (67, (0, 1, 63, 64, 65, 0, 130), 5)                            # off[0] = 67, the last group ends 5 rows before the buffers do
TAP_KG = (67, (0, 65, 130), 5)
TAPS = ((64, 9), (128, 4), (192, 1), (64, 1))                            # (tap_cols, taps)
# what the launcher makes of a forced geometry when W's rows are gathered, worked out by hand from gemm_bf16_tr.hip:567-568
GATHERED_PATH = {1: 1, 2: 1, 3: 1, 4: 4, 5: 5}
TAP_PATH = {64: {1: 4, 2: 4, 3: 4, 4: 4, 5: 4}, 128: GATHERED_PATH, 192: {1: 4, 2: 4, 3: 4, 4: 4, 5: 4}}


def ring_dgrad_cases(cfg):
    """Sweeps over M at N = 72, over N at M = 129 and over K (64 and 128: one and two K-steps, below the NS3 prefetch depth; 192), a poisoned one, and
    four experts in ragged segments, also in 2 and 4 K-slices."""
    out = []
    for o in OUTS:
        out += [case("dgrad", "ring", cfg, o, M, 72, 128) for M in (1, 127, 128, 129)] + [case("dgrad", "ring", cfg, o, 128, 128, 128)]     # (the one M == N)
        out += [case("dgrad", "ring", cfg, o, 129, N, 128) for N in (8, 64, 128, 136)]
        out += [case("dgrad", "ring", cfg, o, 129, 72, K, family="spiky") for K in (64, 192)]
        out += [case("dgrad", "ring", cfg, o, 127, 136, 64, family="poison")]
        for seg in GROUPED_SEGMENTS:
            out += [case("dgrad", "ring", cfg, o, 0, 72, 128, family="spiky", counts=seg, wextra=3)]
            out += [case("dgrad", "ring", cfg, o, 0, 72, 256, counts=seg, wextra=3, split_k=S) for S in (2, 4)]
        out += [case("dgrad", "ring", cfg, o, 0, 72, 128, family="poison", counts=GROUPED_SEGMENTS[0], wextra=3)]
    return out


def ring_wgrad_cases(cfg):
    """Ungrouped sweeps over M, N and K (1 .. 129 rows), seven K groups from row 67 in every family, the same through a gathered index table, and taps
    of 64, 128 and 192 columns."""
    out = []
    for o in OUTS:
        out += [case("wgrad", "ring", cfg, o, M, 72, 65) for M in (8, 128, 136)]
        out += [case("wgrad", "ring", cfg, o, 136, N, 65) for N in (8, 64, 136)]
        out += [case("wgrad", "ring", cfg, o, 136, 72, K, family="spiky") for K in (1, 63, 64, 129)]
        out += [case("wgrad", "ring", cfg, o, 136, 72, kranges=RING_KG, family=f) for f in FAMILIES]
        out += [case("wgrad", "ring", cfg, o, 136, 72, kranges=RING_KG, family=f, w_rows="gathered", path=GATHERED_PATH[cfg]) for f in ("spiky", "poison")]
        out += [case("wgrad", "ring", cfg, o, 136, 0, kranges=TAP_KG, w_rows="taps", taps=t, tap_cols=tc, path=TAP_PATH[tc][cfg],
                     family="poison" if (tc, t) == (64, 9) else "spiky") for tc, t in TAPS]
    return out


PPTR_KG = (0, 1, 64, 65, 128, 129)                                       # the first group is empty


def pptr_cases():
    out = []
    for o in OUTS:
        out += [case("dgrad", "pptr", 6, o, M, N, K, family="spiky" if K == 256 else "soft") for M in (1, 255, 256, 257) for N in (256, 512) for K in (128, 256)]
        out += [case("dgrad", "pptr", 6, o, 0, 256, 128, counts=seg, wextra=3) for seg in ((0, 1, 256, 257), (258, 0, 0, 0))]
        out += [case("dgrad", "pptr", 6, o, 0, 256, 128, counts=(0, 1, 256, 257), wextra=3, family="poison")]
        out += [case("dgrad", "pptr", 6, o, 257, 256, 256, split_k=2)]
        out += [nine_expert_case(o)]
        out += [case("wgrad", "pptr", 6, o, 256, 256, K) for K in (1, 129)]
        out += [case("wgrad", "pptr", 6, o, 256, 512, kranges=(off0, PPTR_KG, 5)) for off0 in (0, 67)]
        out += [case("wgrad", "pptr", 6, o, 256, 256, kranges=(0, PPTR_KG, 5), family="spiky")]
        out += [case("wgrad", "pptr", 6, o, 256, 256, kranges=(67, PPTR_KG, 5), family=f) for f in ("spiky", "poison", "poison_max")]
    return out


def nine_expert_case(o):
    """More than 8 experts under a forced "gemm_tr_cfg" 6: the ping-pong kernel declines, the ring (automatic geometry: 64/NS3) runs it."""
    return case("dgrad", "ring", 6, o, 0, 256, 128, counts=(3, 0, 40, 1, 17, 2, 5, 130, 60), wextra=3, path=2)


F32_MN = ((70, 52), (36, 7), (5, 130), (36, 52))
F32_KG = (7, (100, 0, 71, 129), 5)


def f32_cases():
    """Layouts 1, 2, 3 over K = 1 .. 100 at shapes that take the float4 and the scalar loads, K groups from row 7 (layouts 1 and 3), layout 1 at N = K (the
    shape at which it can be mistaken for layout 3), and the 64 x 64 tile reached by size and by the group count."""
    out = []
    for lay in (1, 2, 3):
        L = f"f32 lay {lay}"
        for M, N in F32_MN:
            vec = "vec" if (lay == 2 or M % 4 == 0) and (lay == 1 or N % 4 == 0) else "scalar"
            out += [case(L, "f32", 0, F32, M, N, K, family="spiky" if K == 100 else "soft", path=vec + " small")
                    for K in (1, 4, 36, 100) if lay != 2 or K % 4 == 0]
            if lay != 2 and N == 52:
                out += [case(L, "f32", 0, F32, M, N, kranges=F32_KG, family=f, path=vec + " small") for f in ("soft", "poison", "poison_max")]
        out += [case(L, "f32", 0, F32, 36, 52, 36, family="poison", path="vec small")]
    out += [case("f32 lay 1", "f32", 0, F32, 70, 36, 36, path="scalar small")]
    out += [case("f32 lay 3", "f32", 0, F32, 832, 832, 5, path="vec 64"), case("f32 lay 3", "f32", 0, F32, 830, 830, 5, path="scalar 64"),
            f32_group_count_case()]
    return out


def f32_group_count_case():
    return case("f32 lay 3", "f32", 0, F32, 256, 256, kranges=(0, (3, 0, 5, 1, 4, 2, 6, 7, 1, 3, 4), 0), path="vec 64")


def strided_cases():
    """lda = cols + 64, every operand 16 bytes into its buffer, c_group_stride = (M + 1) ldc (as everywhere)."""
    f32pad = (64, 8, 8, 8)
    return [case("dgrad", "ring", 1, F32, 129, 72, 128, pad=STRIDED), case("dgrad", "ring", 2, BF16, 129, 72, 128, pad=STRIDED),
            case("wgrad", "ring", 1, F32, 136, 72, kranges=RING_KG, family="poison", pad=STRIDED),
            case("wgrad", "ring", 5, BF16, 136, 72, kranges=RING_KG, family="poison", pad=STRIDED),
            case("wgrad", "ring", 4, F32, 136, 0, kranges=TAP_KG, w_rows="taps", taps=4, tap_cols=64, family="poison", pad=STRIDED),
            case("dgrad", "pptr", 6, BF16, 257, 256, 128, pad=STRIDED), case("wgrad", "pptr", 6, F32, 256, 256, kranges=(67, PPTR_KG, 5), family="poison", pad=STRIDED),
            case("f32 lay 1", "f32", 0, F32, 36, 52, kranges=F32_KG, family="poison", pad=f32pad, path="vec small"),
            case("f32 lay 2", "f32", 0, F32, 36, 7, 36, family="poison", pad=f32pad, path="scalar small"),
            case("f32 lay 3", "f32", 0, F32, 70, 52, kranges=F32_KG, family="poison", pad=f32pad, path="scalar small")]


def bit_identity_cases(out):
    """(ring data gradient, ring weight gradient, ping-pong data gradient, ping-pong weight gradient) of one output dtype, dense leading dimensions."""
    dense = (0, 0, 0, 0)
    return (case("dgrad", "ring", 1, out, 129, 72, 192, family="spiky", pad=dense), case("wgrad", "ring", 1, out, 136, 72, kranges=RING_KG, family="spiky", pad=dense),
            case("dgrad", "pptr", 6, out, 257, 256, 256, family="spiky", pad=dense), case("wgrad", "pptr", 6, out, 256, 256, kranges=(67, PPTR_KG, 5), family="spiky", pad=dense))


def all_cases():
    out = []
    for cfg in RING_CFGS:
        out += ring_dgrad_cases(cfg) + ring_wgrad_cases(cfg)
    out += pptr_cases() + f32_cases() + strided_cases()
    for o in OUTS:
        ring_d, ring_w, pp_d, pp_w = bit_identity_cases(o)
        out += [c._replace(cfg=g, path=g) for c in (ring_d, ring_w) for g in RING_CFGS] + [pp_d, pp_w]
    return out


# ------------------------------------------------------------------------------------------------------------------ report
class Report(_Report):
    """gemm_refs.Report keyed by (kernel, layout, output): worst err / bound of one test, printed at its end; a ratio above 1 fails the test."""

    def add(self, c, rs, gap=0.0):
        for name, q, idx in rs:
            what = "slab sum" if name == "slab_sum" else ("slab" if c.split_k > 1 else "C")
            key = (c.kernel, c.layout + (" gathered" if c.w_rows == "gathered" else " taps" if c.w_rows == "taps" else ""),
                   ("bf16 " if c.out == BF16 else "f32 ") + what)
            if key not in self.worst or q > self.worst[key][0]:
                self.worst[key] = (q, f"{c.tag} {name}{list(idx)}")
            if not q <= 1.0:
                self.failed.append(f"{c.tag}: {name}{list(idx)} err / bound = {q:.3g}")
