"""fp64 reference of the camera transform (the semantics in include/mode_hip.h at mode_frames_preprocess) in plain torch: separable weight
matrices, einsum, quantise, shift, normalise.  Both the unrounded resize R and the levels are exposed, so that a kernel's output can be checked
against every level its fp32 arithmetic may legitimately round to."""
import torch

DELTA = 2e-3          # fp32 evaluation error of R allowed around a rounding tie, in levels (<= 17 + 17 taps on values <= 255: ~ 40 * 2^-24 * 255 = 6e-4)


def axis_weights(n_in: int, n_out: int) -> torch.Tensor:
    """[n_out, n_in] fp64: row o holds the normalised triangle-filter weights of output index o (torch's antialiased bilinear, align_corners=False)."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    Wm = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        center = scale * (o + 0.5)
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        w = [max(0.0, 1.0 - abs((i + xmin - center + 0.5) / support)) for i in range(xmax - xmin)]
        tot = sum(w)
        for i, v in enumerate(w):
            Wm[o, xmin + i] = v / tot
    return Wm


def resize(u8: torch.Tensor, size) -> torch.Tensor:
    """uint8 (..., H, W, 3) -> the unrounded resize R (..., 3, OH, OW) fp64."""
    H, W = u8.shape[-3], u8.shape[-2]
    wy, wx = axis_weights(H, size[0]), axis_weights(W, size[1])
    return torch.einsum("oy,...yxc,px->...cop", wy, u8.to(torch.float64), wx)


def levels(R: torch.Tensor) -> torch.Tensor:
    """The uint8 levels of a uint8-in / uint8-out resize: round to nearest even, clamped."""
    return torch.round(R).clamp(0, 255)


def shift(img: torch.Tensor, shifts, pad: int) -> torch.Tensor:
    """(F, 3, OH, OW) -> out[f][c][y][x] = img[f][c][clamp(y + sy - pad)][clamp(x + sx - pad)], shifts (F, 2) = (sx, sy) clamped into [0, 2 pad]."""
    if shifts is None:
        return img
    F_, _, OH, OW = img.shape
    out = torch.empty_like(img)
    for f in range(F_):
        sx, sy = (min(max(int(v), 0), 2 * pad) for v in shifts[f])
        ys = (torch.arange(OH) + sy - pad).clamp(0, OH - 1)
        xs = (torch.arange(OW) + sx - pad).clamp(0, OW - 1)
        out[f] = img[f][:, ys][:, :, xs]
    return out


def normalise(L: torch.Tensor, mean, std) -> torch.Tensor:
    m = torch.tensor(mean, dtype=torch.float64).view(3, 1, 1)
    s = torch.tensor(std, dtype=torch.float64).view(3, 1, 1)
    return (L / 255.0 - m) / s


def transform(u8: torch.Tensor, size, mean, std, shifts=None, pad: int = 0):
    """uint8 (F, H, W, 3) frames -> (R, out): R (F, 3, OH, OW) the unrounded, SHIFTED resize; out the reference output from its levels."""
    R = shift(resize(u8.cpu(), size), None if shifts is None else torch.as_tensor(shifts).cpu().tolist(), pad)
    return R, normalise(levels(R), mean, std)


def check_output(got: torch.Tensor, R: torch.Tensor, mean, std):
    """Every element of ``got`` (F, 3, OH, OW; fp32 or bf16) equals (L / 255 - mean) / std for an integer level L with |L - R| <= 0.5 + DELTA, within
    2e-6 (fp32: three fp32 operations on |values| < 2.5) or 2^-8 |ref| + 2e-6 (bf16: one more rounding to 8 significant bits).  Returns the worst
    excess over the tolerance (<= 0 passes) and the number of elements that sit within DELTA of a tie."""
    g = got.detach().cpu().to(torch.float64)
    assert g.shape == R.shape, (g.shape, R.shape)
    lo = torch.ceil(R - 0.5 - DELTA).clamp(0, 255)
    hi = torch.floor(R + 0.5 + DELTA).clamp(0, 255)
    assert bool((hi - lo <= 1).all()) and bool((hi >= lo).all())
    worst = None
    for L in (lo, hi):
        ref = normalise(L, mean, std)
        tol = 2e-6 + (ref.abs() * 2.0 ** -8 if got.dtype == torch.bfloat16 else 0.0)
        ex = (g - ref).abs() - tol
        worst = ex if worst is None else torch.minimum(worst, ex)
    return float(worst.max()), int((hi != lo).sum())


def random_shifts_aug(x: torch.Tensor, pad: int, shift_xy: torch.Tensor) -> torch.Tensor:
    """DrQ-v2's RandomShiftsAug.forward, line for line, with the random draw replaced by ``shift_xy`` ((n, 1, 1, 2), the integers it would draw)."""
    import torch.nn.functional as F
    n, c, h, w = x.size()
    assert h == w
    padding = tuple([pad] * 4)
    x = F.pad(x, padding, "replicate")
    eps = 1.0 / (h + 2 * pad)
    arange = torch.linspace(-1.0 + eps, 1.0 - eps, h + 2 * pad, device=x.device, dtype=x.dtype)[:h]
    arange = arange.unsqueeze(0).repeat(h, 1).unsqueeze(2)
    base_grid = torch.cat([arange, arange.transpose(1, 0)], dim=2)
    base_grid = base_grid.unsqueeze(0).repeat(n, 1, 1, 1)
    shift_ = shift_xy.to(x.dtype).clone()
    shift_ *= 2.0 / (h + 2 * pad)
    grid = base_grid + shift_
    return F.grid_sample(x, grid, padding_mode="zeros", align_corners=False)

