"""Plain fp64 restatements (CPU torch) of the row kernels and the small training kernels, shared by tests/test_gpu_row_kernels.py and
tests/test_gpu_train_ops.py; tests/test_row_kernel_references.py validates them without a GPU.  Inputs are the tensors the kernel reads (fp32, or
bf16 already rounded): every function widens them to fp64 itself.  Backward references are torch autograd of the forward expression."""
import torch
import torch.nn.functional as F


def f64(t):
    return None if t is None else torch.as_tensor(t).detach().double().cpu()


def rel(a, b):
    a, b = f64(a), f64(b)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def nrm(t):
    return float(f64(t).norm())


def rms(v, eps):
    return (v.pow(2).sum(-1, keepdim=True).sqrt() * v.shape[-1] ** -0.5).clamp_min(eps)


def partial_ss(u, n):
    """[N, n] sums of squares of u over n equal column groups, formed in fp64 and rounded to fp32 (what a MODE_EPI_RESIDUAL_NORM GEMM publishes)."""
    N, D = u.shape
    assert D % n == 0
    return f64(u).pow(2).view(N, n, D // n).sum(-1).float().contiguous()


def combine(u, Y, pos, posw, g=None, cond=None, rpc=1, eps=1e-6, u_ss=None, u_gain=None):
    """x_next = ln_2(u) + sum_j posw[:, j] * (sum of slabs Y)[pos[:, j]], h = x_next / rms * g (+ cond[row // rpc]).  u [N, D], Y [S, N*k, D],
    pos / posw [N, k].  Returns (x_next, h); h is None without g."""
    u, Y, posw = f64(u), f64(Y), f64(posw)
    N, D = u.shape
    if u_ss is not None:                                   # fused ln_2: u arrives un-normalised with its partial sums of squares
        u = u / (f64(u_ss).sum(1, keepdim=True).sqrt() * D ** -0.5).clamp_min(eps) * f64(u_gain)
    ys = Y.sum(0)
    x = u.clone()
    for j in range(pos.shape[1]):
        x = x + posw[:, j:j + 1] * ys[pos[:, j].long().cpu()]
    if g is None:
        return x, None
    h = x / rms(x, eps) * f64(g)
    if cond is not None:
        h = h + f64(cond)[torch.arange(N) // rpc]
    return x, h


def head(u, Y, pos, posw, g, w_out, b_out, B, T, A_len, eps=1e-6, u_ss=None, u_gain=None, x_a=None, scal=None, den_prev=None, lin=None,
         aux1=None, aux2=None):
    """Last combine, final norm and Linear(D, A_dim) on the last A_len tokens of each sample, then the EDM / solver update.  scal [B or 1, 4].
    Returns (F, denoised, x_next), each [B, A_len, A_dim]; the last two None without scal."""
    _, nv = combine(u, Y, pos, posw, g=g, eps=eps, u_ss=u_ss, u_gain=u_gain)
    rows = torch.tensor([[b * T + (T - A_len) + ai for ai in range(A_len)] for b in range(B)])
    Fh = nv[rows] @ f64(w_out).t() + f64(b_out)
    if scal is None:
        return Fh, None, None
    s, xa = f64(scal).expand(B, 4)[:, None, None, :], f64(x_a)
    den = Fh * s[..., 1] + xa * s[..., 0]
    if lin is not None:
        l = f64(lin)
        xn = l[0] * xa + l[1] * den
        if aux1 is not None:
            xn = xn + l[2] * f64(aux1)
        if aux2 is not None:
            xn = xn + l[3] * f64(aux2)
        return Fh, den, xn
    dd = den
    if den_prev is not None:
        dd = torch.where(s[..., 3] != 0, (1 + s[..., 3]) * den - s[..., 3] * f64(den_prev), den)
    return Fh, den, s[..., 2] * xa + (1 - s[..., 2]) * dd


def embed(goal_e, img_e, act, w_act, pos, g, emb_t=None, c_in=None, cond=None, eps=1e-6):
    """[ emb_t | goal_e + pos[0] | img_e + pos[1] | (act * c_in) @ w_act^T + pos[1:] ] and its conditioned norm.  emb_t [B or 1, D] or None (no sigma
    token), c_in [B or 1] or None, cond [B or 1, D] or None.  Returns (x [B, T, D], h)."""
    goal_e, img_e, act, pos = f64(goal_e), f64(img_e), f64(act), f64(pos)
    B, D = goal_e.shape
    if c_in is not None:
        act = act * f64(c_in).expand(B)[:, None, None]
    parts = [] if emb_t is None else [f64(emb_t).expand(B, D)[:, None]]
    parts += [(goal_e + pos[0])[:, None], img_e + pos[1], act @ f64(w_act).t() + pos[1:]]
    x = torch.cat(parts, 1)
    h = x / rms(x, eps) * f64(g)
    if cond is not None:
        h = h + f64(cond).expand(B, D)[:, None]
    return x, h


def rmsnorm_cond(x, g, cond=None, rpc=1, eps=1e-6):
    x = f64(x)
    y = x / rms(x, eps) * f64(g)
    return y if cond is None else y + f64(cond)[torch.arange(x.shape[0]) // rpc]


def ddim_edm_step(Fh, x_a, scal):
    """scal [B or 1, 4] = {c_skip, c_out, r, -}; Fh / x_a [B, per_sample].  Returns (denoised, x_next)."""
    Fh, xa = f64(Fh), f64(x_a)
    s = f64(scal).expand(Fh.shape[0], 4)[:, None, :]
    den = Fh * s[..., 1] + xa * s[..., 0]
    return den, s[..., 2] * xa + (1 - s[..., 2]) * den


def sigma_embed(sigma, w, b):
    return f64(sigma).log()[:, None] / 4 * f64(w).reshape(-1) + f64(b)


# ------------------------------------------------------------------------------------------------------------------ training kernels
def edm_noise_scale(action, noise, sigma, sd):
    s = f64(sigma)[:, None]
    return (f64(action) + f64(noise) * s) / (s * s + sd * sd).sqrt()


def edm_loss(Fh, action, noise, sigma, sd, dtype=torch.float64):
    """GCDenoiser.loss on the model output Fh [B, n]: (loss, dF by autograd, the B*n terms of the mean).  dtype = float32: the same expressions in
    fp32 on the CPU - the reference's own sensitivity to fp32 rounding (the target divides a cancelling difference by c_out ~ sigma)."""
    c = lambda t: torch.as_tensor(t).detach().cpu().to(dtype)
    Fh = c(Fh).requires_grad_(True)
    a, s = c(action), c(sigma)[:, None]
    s2 = s * s + sd * sd
    c_skip, c_out = sd * sd / s2, s * sd / s2.sqrt()
    noised = a + c(noise) * s
    terms = (Fh - (a - c_skip * noised) / c_out).pow(2)
    loss = terms.flatten(1).mean()
    loss.backward()
    return loss.detach(), Fh.grad, terms.detach() / terms.numel()


def pos_row_map(T, t0, n_img, A_len, shift=0):
    """Positional row added to each token of the assembled sequence (-1: none).  shift != 0 is the deliberately wrong map of the sensitivity check."""
    rows = [-1] * T
    rows[t0] = 0
    for i in range(n_img):
        rows[t0 + 1 + i] = 1
    for a in range(A_len):
        rows[t0 + 1 + n_img + a] = min(1 + a + shift, A_len)
    return rows


def pos_emb_bwd(dx0, t0, n_img, A_len, shift=0):
    """Gradient of <x0, dx0> with respect to pos for x0[:, t] = token[t] + pos[row(t)], by autograd.  dx0 [B, T, D].  Returns (dpos, sum of |terms|)."""
    dx0 = f64(dx0)
    B, T, D = dx0.shape
    pos = torch.zeros(1 + A_len, D, dtype=torch.float64, requires_grad=True)
    rows = pos_row_map(T, t0, n_img, A_len, shift)
    x0 = torch.stack([pos[r] if r >= 0 else torch.zeros(D, dtype=torch.float64) for r in rows]).expand(B, T, D)
    (x0 * dx0).sum().backward()
    mag = torch.zeros(1 + A_len, D, dtype=torch.float64)
    for t, r in enumerate(rows):
        if r >= 0:
            mag[r] += dx0[:, t].abs().sum(0)
    return pos.grad, mag


def sigma_embed_bwd(de1, sigma):
    """Autograd of e1 = log(sigma)/4 * w + b.  Returns (dw, db, sum |terms| of dw, sum |terms| of db)."""
    de1, s = f64(de1), f64(sigma).log()[:, None] / 4
    D = de1.shape[1]
    w = torch.zeros(D, dtype=torch.float64, requires_grad=True); b = torch.zeros(D, dtype=torch.float64, requires_grad=True)
    ((s * w + b) * de1).sum().backward()
    return w.grad, b.grad, (de1 * s).abs().sum(0), de1.abs().sum(0)


def gelu(x, dout):
    x = f64(x).requires_grad_(True)
    y = F.gelu(x)
    y.backward(f64(dout))
    return y.detach(), x.grad


def router_weights(logits, idx_sorted, normalize, T):
    """softmax -> clamp -> gather -> optional renormalisation: combine weights [B, T, k] of logits [B, E], slots in ascending expert id."""
    B, E = logits.shape
    probs = torch.softmax(logits - logits.max(-1, keepdim=True).values, -1).clamp(1e-9, 1 - 1e-9)
    w = probs[:, None, :].expand(B, T, E).gather(2, idx_sorted)
    return w / w.sum(-1, keepdim=True) if normalize else w


def router_loss(logits, dw, idx, normalize, T, lb_coef=None, z_coef=None, rows_per_layer=None):
    """The scalar whose gradient with respect to logits the router backward returns: <w, dw> (+ the load-balancing term, linear in the combine weights
    with coefficient lb_coef[layer, expert]) (+ z_coef / 2 * sum_rows log(sum exp(l) + 1e-6)^2 on l = logits - logits.max()).  idx [B, T, k], any order."""
    B, E = logits.shape
    srt = idx.long().sort(-1).values
    w = router_weights(logits, srt, normalize, T)
    loss = (w * dw.to(logits.dtype).view(B, T, -1)).sum()
    if lb_coef is not None:
        layer = torch.arange(B) // rows_per_layer
        loss = loss + (w * lb_coef.to(logits.dtype)[layer][:, None, :].expand(B, T, E).gather(2, srt)).sum()
    if z_coef is not None:
        l = logits - logits.max(-1, keepdim=True).values          # torch.max: the FIRST maximal column receives the shift's gradient
        loss = loss + z_coef / 2 * torch.log(torch.exp(l).sum(-1) + 1e-6).pow(2).sum()
    return loss


def router_bwd(logits, dw, idx, normalize, T, dtype=torch.float64, **aux):
    lg = torch.as_tensor(logits).detach().cpu().to(dtype).requires_grad_(True)
    router_loss(lg, dw.cpu(), idx.cpu(), normalize, T, **{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in aux.items()}).backward()
    return lg.grad
