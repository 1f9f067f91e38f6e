"""fp64 restatement of the factored LoRA gradient (csrc/lora_train.hip, include/mode_hip.h ModeLoraFactDesc) with DERIVED per-element bounds, in
the style of tests/lora_refs.py (U = 2^-23 = two unit roundoffs u of fp32).

With Y = X W_eff^T, W_eff = W + s B A, and the rows lo_g .. hi_g of X [M, cols] (row m read at x_rows[m]) and dY [M, rows] belonging to matrix g:
    T = dY_g B_g [M_g, r]      U = X_g A_g^T [M_g, r]      dA_g = s T^T X_g [r, cols]      dB_g = s dY_g^T U [rows, r]

Bound.  Two chained fp32 reductions.  The first has K1 terms (K1 = rows for T, cols for U): however its fma chains are split and joined, an entry
carries at most K1 roundings of relative size u on partial sums bounded by the sum of magnitudes, |T^ - T| <= K1 u |dY_g||B_g| (U likewise).  The
second sums M_g products of such an entry with an exactly represented bf16 value: the inherited error passes through linearly, and the M_g fma
roundings, the at most ceil(M_g / 128) - 1 <= M_g adds of row-block shares and the multiplication by s add at most 2 M_g + 1 roundings on partial
sums bounded by the same sum of magnitudes.  To first order in u
    |got - ref| <= (K1 + 2 M_g + 1) u S  <=  (K1 + M_g + 2) U S        (u = U / 2; K1 >= 8)
    S_A = |s| (|dY_g||B_g|)^T |X_g|          S_B = |s| |dY_g|^T (|X_g||A_g|^T)
A group without rows has ref = 0 and bound = 0: only an exact zero passes.

The deliberately WRONG references (scale dropped, neighbouring groups' adapters swapped, x_rows ignored, last row of each group dropped, T and U
exchanged) are what the tests must tell from the right one; where a case cannot (one group: nothing to swap; identity rows: nothing to ignore)
`wrong_refs` returns None for it and says why in EXCUSED.

Exactness inputs: X, dY in {-1, 0, 1} and A, B = n + k 2^-10 with n, k in {-1, 0, 1} (not bf16 values), s = 0.5.  Every product and every partial
sum, in any order, is an integer multiple of 2^-10 below 2^24 such units - asserted here - so every fp32 operation is exact and the kernel must
return the fp64 reference bit for bit."""
from __future__ import annotations

import functools

import torch

from gemm_refs import U

SCALE = 1.7                                                                        # not a power of two: a dropped scale changes every bit
SHAPES = [(8, 64), (72, 64), (64, 192), (384, 128), (128, 512)]                    # (rows, cols)
RANKS = [1, 3, 16, 64]
GROUPS = [1, 3]
SIZES = [1, 63, 64, 65, 200]                                                       # non-empty group sizes (with 0: the set the kernel's row blocks of 128 see)
CASES = [(G, rows, cols, r, perm) for (rows, cols) in SHAPES for r in RANKS for G in GROUPS for perm in (False, True)]
EXACT_CASES = [(1, 96, 64, 3), (3, 96, 96, 16), (3, 8, 96, 1), (1, 72, 64, 64)]    # (G, rows, cols, r)
XTRA = 3
EXCUSED = {"groups swapped": "G == 1: there is no neighbouring group", "x_rows ignored": "x_rows is None: rows are read in place"}


def f64(t):
    return t.detach().double().cpu()


def group_sizes(G, rows, cols, r):
    """G = 1: one size out of SIZES; G = 3: two of them and ONE EMPTY group, whose position rotates with the case."""
    i = SHAPES.index((rows, cols)) * len(RANKS) + RANKS.index(r)
    if G == 1:
        return [SIZES[i % 5]]
    three = [0, SIZES[i % 5], SIZES[(i + 2 + i // 5) % 5]]
    return three[-(i % 3):] + three[:-(i % 3)] if i % 3 else three


@functools.lru_cache(maxsize=None)
def inputs(G, rows, cols, r, perm):
    """Operands of one case (CPU), the same for every test: X [M, cols] and dY [M, rows] bf16-valued Gaussians (as bf16 tensors), A [G, r, cols] and
    B [G, rows, r] fp32, offsets (a list of G + 1 ints), x_rows (int32, a random permutation, or None)."""
    g = torch.Generator().manual_seed(1000003 * G + 7919 * rows + 31 * cols + r + 500009 * int(perm))
    sizes = group_sizes(G, rows, cols, r)
    M = sum(sizes)
    offsets = [0]
    for n in sizes:
        offsets.append(offsets[-1] + n)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    # with x_rows, X holds XTRA rows more than dY and row m is read at XTRA + a random permutation: no row stays in place, even where M = 1
    return dict(X=rn(M + XTRA * int(perm), cols).bfloat16(), dY=rn(M, rows).bfloat16(), A=rn(G, r, cols) * r ** -0.5, B=rn(G, rows, r) * 0.1,
                offsets=offsets, x_rows=(XTRA + torch.randperm(M, generator=g)).to(torch.int32) if perm else None, M=M)


@functools.lru_cache(maxsize=None)
def exact_inputs(G, rows, cols, r):
    """The exactness family.  Group sizes {128, 65, 0} (G = 3) or {128}; a random permutation as x_rows."""
    g = torch.Generator().manual_seed(77 + 13 * rows + 7 * cols + r + G)
    sizes = [128, 0, 65][:G] if G == 3 else [128]
    M = sum(sizes)
    offsets = [0]
    for n in sizes:
        offsets.append(offsets[-1] + n)
    tri = lambda *s: torch.randint(-1, 2, s, generator=g).float()
    d = dict(X=tri(M, cols).bfloat16(), dY=tri(M, rows).bfloat16(), A=tri(G, r, cols) + tri(G, r, cols) * 2.0 ** -10,
             B=tri(G, rows, r) + tri(G, rows, r) * 2.0 ** -10, offsets=offsets, x_rows=torch.randperm(M, generator=g).to(torch.int32), M=M, s=0.5)
    # every partial sum of either stage, in units of 2^-10: at most max(M_g) * max(rows, cols) * 1025 - and in fact, on these operands:
    assert rows <= 96 and cols <= 96 and max(sizes) <= 128 and max(sizes) * max(rows, cols) * 1025 < 2 ** 24
    assert float(d["A"].abs().max()) <= 1 + 2.0 ** -10 and float(d["B"].abs().max()) <= 1 + 2.0 ** -10
    (_, _), (sA, sB) = fact_ref(d["X"], d["dY"], offsets, d["x_rows"], d["A"], d["B"], 1.0, sums=True)
    assert float(max(sA.max(), sB.max())) * 2 ** 10 < 2 ** 24
    assert not bool((d["A"].bfloat16().float() == d["A"]).all())                   # the adapter values do need fp32
    return d


def _groups(X, dY, offsets, x_rows, G):
    X, dY = f64(X), f64(dY)
    if x_rows is not None:
        X = X[x_rows.long().cpu()]
    offsets = [0, dY.shape[0]] if offsets is None else list(offsets)
    assert len(offsets) == G + 1
    return [(X[offsets[g]: offsets[g + 1]], dY[offsets[g]: offsets[g + 1]]) for g in range(G)]


def fact_ref(X, dY, offsets, x_rows, A, B, s, sums=False, drop_last=False, exchange=False):
    """((dA, dB), (bound_dA, bound_dB)) in fp64; with `sums` the second pair is (S_A, S_B) instead.  drop_last / exchange: the wrong references."""
    A, B = f64(A), f64(B)
    G, r, cols = A.shape
    rows = B.shape[1]
    dA, dB = torch.zeros(G, r, cols, dtype=torch.float64), torch.zeros(G, rows, r, dtype=torch.float64)
    bA, bB = torch.zeros_like(dA), torch.zeros_like(dB)
    for g, (Xg, dYg) in enumerate(_groups(X, dY, offsets, x_rows, G)):
        if drop_last:
            Xg, dYg = Xg[:-1], dYg[:-1]
        Mg = Xg.shape[0]
        T, Uu = dYg @ B[g], Xg @ A[g].T
        if exchange:
            T, Uu = Uu, T
        dA[g], dB[g] = s * (T.T @ Xg), s * (dYg.T @ Uu)
        SA = abs(s) * ((dYg.abs() @ B[g].abs()).T @ Xg.abs())
        SB = abs(s) * (dYg.abs().T @ (Xg.abs() @ A[g].abs().T))
        bA[g], bB[g] = (SA, SB) if sums else ((rows + Mg + 2) * U * SA, (cols + Mg + 2) * U * SB)
    return (dA, dB), (bA, bB)


def dense_ref(X, dY, offsets, x_rows, A, B, s):
    """The same gradients through the dense weight gradient dW_g = dY_g^T X_g: dA = s B^T dW, dB = s dW A^T (what grad="dense" computes)."""
    A, B = f64(A), f64(B)
    G = A.shape[0]
    dW = torch.stack([dYg.T @ Xg for Xg, dYg in _groups(X, dY, offsets, x_rows, G)])
    return s * (B.transpose(1, 2) @ dW), s * (dW @ A.transpose(1, 2))


def wrong_refs(X, dY, offsets, x_rows, A, B, s):
    """name -> (dA, dB), or None where this case cannot tell the wrong reference from the right one (EXCUSED says why)."""
    G = A.shape[0]
    ref = lambda *a, **k: fact_ref(*a, **k)[0]
    return {
        "scale dropped": ref(X, dY, offsets, x_rows, A, B, 1.0),
        "groups swapped": ref(X, dY, offsets, x_rows, torch.roll(A, -1, 0), torch.roll(B, -1, 0), s) if G > 1 else None,
        "x_rows ignored": ref(X, dY, offsets, None, A, B, s) if x_rows is not None else None,
        "last row of each group dropped": ref(X, dY, offsets, x_rows, A, B, s, drop_last=True),
        "T and U exchanged": ref(X, dY, offsets, x_rows, A, B, s, exchange=True),
    }


def worst(got, ref, bound):
    """max over elements of |got - ref| / bound (an exactly right element counts 0 whatever its bound)."""
    err = (f64(got) - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(ratio.max())
