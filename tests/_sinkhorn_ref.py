"""References for the Sinkhorn divergence tests (not a test module).

``oracle``: an fp64 NumPy restatement of the contract of diffsound_amd/ddsp/sinkhorn.py (geomloss==0.2.6
SamplesLoss("sinkhorn", p=2, blur, scaling, debias) on its tensorized backend), logsumexp by max shift, with the
gradient formula of the last extrapolation.  ``torch_geomloss``: the same algorithm as geomloss's tensorized code
states it, in torch at the inputs' precision (expanded cost |x|^2 + |y|^2 - 2 x.y, torch.logsumexp, autograd for the
gradient) - the fp32 error level of the reference algorithm itself."""
import numpy as np


def eps_schedule(d, blur, scaling):
    return [d ** 2] + [float(np.exp(e)) for e in np.arange(2 * np.log(d), 2 * np.log(blur), 2 * np.log(scaling))] + \
        [blur ** 2]


def diameter(x, y):
    """Diagonal of the joint bounding box of every point of x and y (all batches)."""
    D = x.shape[-1]
    p = np.concatenate([np.asarray(x, np.float64).reshape(-1, D), np.asarray(y, np.float64).reshape(-1, D)])
    return float(np.sqrt(((p.max(0) - p.min(0)) ** 2).sum()))


def _cost(p, q):
    return ((p[:, None, :] - q[None, :, :]) ** 2).sum(-1) / 2


def _lse(v):
    m = v.max(1, keepdims=True)
    return (m + np.log(np.exp(v - m).sum(1, keepdims=True)))[:, 0]


def _softmin(eps, C, h):
    return -eps * _lse(h[None, :] - C / eps)


def _one(x, y, a, b, eps_list, debias, converge):
    """One batch: (S, grad_x, grad_y, residual of the last averaged update)."""
    la, lb = np.log(a), np.log(b)
    Cxy, Cyx, Cxx, Cyy = _cost(x, y), _cost(y, x), _cost(x, x), _cost(y, y)
    e = eps_list[0]
    f_ba, g_ab = _softmin(e, Cxy, lb), _softmin(e, Cyx, la)
    f_aa, g_bb = (_softmin(e, Cxx, la), _softmin(e, Cyy, lb)) if debias else (None, None)

    def update(e, f_ba, g_ab, f_aa, g_bb):
        ft_ba, gt_ab = _softmin(e, Cxy, lb + g_ab / e), _softmin(e, Cyx, la + f_ba / e)
        out = [(f_ba + ft_ba) / 2, (g_ab + gt_ab) / 2]
        if debias:
            out += [(f_aa + _softmin(e, Cxx, la + f_aa / e)) / 2, (g_bb + _softmin(e, Cyy, lb + g_bb / e)) / 2]
        else:
            out += [None, None]
        return out

    def change(old, new):
        return max(np.abs(n - o).max() for o, n in zip(old, new) if o is not None)

    res = np.inf
    for e in eps_list:
        new = update(e, f_ba, g_ab, f_aa, g_bb)
        res = change((f_ba, g_ab, f_aa, g_bb), new)
        f_ba, g_ab, f_aa, g_bb = new
    if converge:
        e = eps_list[-1]
        for _ in range(100000):
            if res < 1e-12:
                break
            new = update(e, f_ba, g_ab, f_aa, g_bb)
            res = change((f_ba, g_ab, f_aa, g_bb), new)
            f_ba, g_ab, f_aa, g_bb = new
    e = eps_list[-1]
    # last extrapolation: simultaneous, no averaging; its row-softmax weights give the gradient
    hx, hy = lb + g_ab / e, la + f_ba / e
    Vxy, Vyx = hx[None, :] - Cxy / e, hy[None, :] - Cyx / e
    F_ba, G_ab = -e * _lse(Vxy), -e * _lse(Vyx)
    P = np.exp(Vxy - _lse(Vxy)[:, None])
    Pt = np.exp(Vyx - _lse(Vyx)[:, None])
    gx = a[:, None] * (P.sum(1)[:, None] * x - P @ y)
    gy = b[:, None] * (Pt.sum(1)[:, None] * y - Pt @ x)
    S = float(a @ F_ba + b @ G_ab)
    if debias:
        Vxx, Vyy = (la + f_aa / e)[None, :] - Cxx / e, (lb + g_bb / e)[None, :] - Cyy / e
        F_aa, G_bb = -e * _lse(Vxx), -e * _lse(Vyy)
        Q = np.exp(Vxx - _lse(Vxx)[:, None])
        R = np.exp(Vyy - _lse(Vyy)[:, None])
        gx -= a[:, None] * (Q.sum(1)[:, None] * x - Q @ x)
        gy -= b[:, None] * (R.sum(1)[:, None] * y - R @ y)
        S -= float(a @ F_aa + b @ G_bb)
    return S, gx, gy, res


def oracle(x, y, a=None, b=None, blur=0.05, scaling=0.5, diameter_=None, debias=True, converge=False):
    """fp64.  x (N, D) or (B, N, D), y likewise; a, b weights (uniform when None).  Returns (S (B,), grad_x, grad_y,
    eps_list, residuals) with batch axes as given; ``converge`` continues the averaged update at blur^2 until the
    largest change of a potential is below 1e-12 before the last extrapolation."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    batched = x.ndim == 3
    if not batched:
        x, y = x[None], y[None]
        a = None if a is None else np.asarray(a)[None]
        b = None if b is None else np.asarray(b)[None]
    B, N, _ = x.shape
    M = y.shape[1]
    a = np.full((B, N), 1.0 / N) if a is None else np.asarray(a, np.float64)
    b = np.full((B, M), 1.0 / M) if b is None else np.asarray(b, np.float64)
    d = diameter(x, y) if diameter_ is None else float(diameter_)
    eps_list = eps_schedule(d, blur, scaling)
    out = [_one(x[k], y[k], a[k], b[k], eps_list, debias, converge) for k in range(B)]
    S = np.array([o[0] for o in out])
    gx = np.stack([o[1] for o in out])
    gy = np.stack([o[2] for o in out])
    res = np.array([o[3] for o in out])
    if not batched:
        gx, gy = gx[0], gy[0]
    return S, gx, gy, eps_list, res


def torch_geomloss(x, y, a=None, b=None, blur=0.05, scaling=0.5, diameter_=None, debias=True, grad=True):
    """geomloss's tensorized arithmetic restated in torch at x's dtype and device.  x (B, N, D), y (B, M, D).
    Returns (S (B,), grad_x, grad_y) with autograd through the last extrapolation (the loop runs without grad), or
    S alone when ``grad`` is False."""
    import torch

    x = x.detach().clone().requires_grad_(grad)
    y = y.detach().clone().requires_grad_(grad)
    B, N, _ = x.shape
    M = y.shape[1]
    a = torch.full((B, N), 1.0 / N, dtype=x.dtype, device=x.device) if a is None else a
    b = torch.full((B, M), 1.0 / M, dtype=x.dtype, device=x.device) if b is None else b
    if diameter_ is None:
        D = x.shape[-1]
        p = torch.cat([x.detach().reshape(-1, D), y.detach().reshape(-1, D)])
        diameter_ = (p.max(0)[0] - p.min(0)[0]).norm().item()
    eps_list = eps_schedule(diameter_, blur, scaling)

    def cost(p, q):
        pp = (p * p).sum(-1).unsqueeze(2)
        qq = (q * q).sum(-1).unsqueeze(1)
        return (pp - 2 * torch.matmul(p, q.permute(0, 2, 1)) + qq) / 2

    def softmin(eps, C, h):
        return -eps * (h.view(B, 1, -1) - C / eps).logsumexp(2).view(B, -1)

    la, lb = a.log(), b.log()
    Cxy, Cyx = cost(x, y.detach()), cost(y, x.detach())
    Cxx, Cyy = cost(x, x.detach()), cost(y, y.detach())
    with torch.no_grad():
        e = eps_list[0]
        g_ab, f_ba = softmin(e, Cyx, la), softmin(e, Cxy, lb)
        if debias:
            f_aa, g_bb = softmin(e, Cxx, la), softmin(e, Cyy, lb)
        for e in eps_list:
            ft_ba, gt_ab = softmin(e, Cxy, lb + g_ab / e), softmin(e, Cyx, la + f_ba / e)
            if debias:
                ft_aa, gt_bb = softmin(e, Cxx, la + f_aa / e), softmin(e, Cyy, lb + g_bb / e)
            f_ba, g_ab = 0.5 * (f_ba + ft_ba), 0.5 * (g_ab + gt_ab)
            if debias:
                f_aa, g_bb = 0.5 * (f_aa + ft_aa), 0.5 * (g_bb + gt_bb)
    e = eps_list[-1]
    F_ba, G_ab = softmin(e, Cxy, (lb + g_ab / e).detach()), softmin(e, Cyx, (la + f_ba / e).detach())
    if debias:
        F_aa, G_bb = softmin(e, Cxx, (la + f_aa / e).detach()), softmin(e, Cyy, (lb + g_bb / e).detach())
        S = (a * (F_ba - F_aa)).sum(1) + (b * (G_ab - G_bb)).sum(1)
    else:
        S = (a * F_ba).sum(1) + (b * G_ab).sum(1)
    if not grad:
        return S.detach()
    gx, gy = torch.autograd.grad(S.sum(), [x, y])
    return S.detach(), gx, gy
