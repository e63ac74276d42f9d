"""The contact-force scheme of diffsound_amd/csrc/contact.hip (ds_contact_fwd / ds_contact_bwd) restated in numpy, its
adjoint, the bounds the kernel tests use and the cases they share.  Not a test module.

Per clip a, with h = 1 / (sr R), z_i = exp((-d_i + i w_i) h), kap_i = c[a,i]^2 / w_i, xh = 0, vh = v0, s_i = 0 at n = 0,
for n = 0 .. F R - 1:

    u     = sum_i kap_i Im s_i            (added in ascending i, one term after the other)
    delta = xh - u ;  f = kH delta^p where delta > 0, else 0
    force[a, n // R] += f / R
    vh   -= h f / M ;  xh += h vh
    s_i   = z_i (s_i + h f)

``forward`` and ``adjoint`` take the dtype (``np.float64`` or ``np.longdouble``) and do every operation in it; the force
is NOT rounded to fp32 here.  The adjoint is the reverse sweep of contact.hip's header; what vouches for it is
tests/test_contact_ref_cpu.py: central differences of the longdouble forward.

Bounds (``bound``).  The truth of an output is the longdouble restatement.  E64 = the float64 restatement's largest
deviation from it over the output, divided by the output's largest magnitude.  A kernel output passes when every element
deviates by at most 8 max(E64, 2^-52) scale; the force, stored in fp32, also gets 2^-24 |ref| per element.  The 8 is a margin
over the restatement's own error for what the device does differently from numpy - the order of the modal sum (lane-strided,
then a butterfly) and its exp, sincos and pow against libm (contact.hip fuses no multiply-adds, so the rest is the same
operations in the same order).
"""
import numpy as np

SR = 44100.0
TWO_PI = 2.0 * np.pi
U32 = 2.0 ** -24
EPS64 = 2.0 ** -52


def _ctype(dtype):
    return np.clongdouble if np.dtype(dtype) == np.dtype(np.longdouble) else np.complex128


def _seq_sum(x):
    """Sum over the last axis in ascending order, one term after the other (np.sum adds pairwise)."""
    return np.cumsum(x, axis=-1)[..., -1]


def _setup(d, w, c, M, v0, kH, sr, R, dtype):
    T = np.dtype(dtype).type
    d, w = np.asarray(d, dtype=dtype), np.asarray(w, dtype=dtype)
    c = np.asarray(c, dtype=dtype)
    M, v0, kH = (np.asarray(x, dtype=dtype) for x in (M, v0, kH))
    h = T(1) / (T(sr) * T(R))
    e = np.exp(-d * h)
    z = (e * np.cos(w * h) + 1j * (e * np.sin(w * h))).astype(_ctype(dtype))
    kap = c * c / w[None, :]
    return T, d, w, c, M, v0, kH, h, z, kap


def forward(d, w, c, M, v0, kH, F, p=1.5, R=8, sr=SR, dtype=np.float64, keep=False):
    """dict: force (A, F), f, delta (A, N) per substep, xh, vh (A,) at the end; ``keep`` adds s (N, A, m), the states that
    enter each substep.  d, w (m,), c (A, m), M, v0, kH (A,)."""
    T, d, w, c, M, v0, kH, h, z, kap = _setup(d, w, c, M, v0, kH, sr, R, dtype)
    A, m = c.shape
    N = F * R
    p = T(p)
    xh, vh = np.zeros(A, dtype=dtype), v0.copy()
    s = np.zeros((A, m), dtype=_ctype(dtype))
    force = np.zeros((A, F), dtype=dtype)
    fs, deltas = np.zeros((A, N), dtype=dtype), np.zeros((A, N), dtype=dtype)
    S = np.zeros((N, A, m), dtype=_ctype(dtype)) if keep else None
    hit = v0 > 0
    for n in range(N):
        delta = xh - _seq_sum(kap * s.imag)
        on = (delta > 0) & hit
        f = kH * np.where(on, np.power(np.where(on, delta, T(1)), p), T(0))
        force[:, n // R] += f / T(R)
        fs[:, n], deltas[:, n] = f, delta
        if keep:
            S[n] = s
        vh = vh - h * f / M
        xh = xh + h * vh
        s = z[None, :] * (s + (h * f)[:, None])
    out = dict(force=force, f=fs, delta=deltas, xh=xh, vh=vh, h=h)
    if keep:
        out["s"] = S
    return out


def adjoint(gforce, d, w, c, M, v0, kH, p=1.5, R=8, sr=SR, dtype=np.float64):
    """dict gd, gw (m,), gc (A, m), gM, gv0, gkH (A,) of sum(gforce * force): the reverse sweep."""
    gforce = np.asarray(gforce, dtype=dtype)
    A, F = gforce.shape
    fw = forward(d, w, c, M, v0, kH, F, p, R, sr, dtype, keep=True)
    T, d, w, c, M, v0, kH, h, z, kap = _setup(d, w, c, M, v0, kH, sr, R, dtype)
    m = c.shape[1]
    N = F * R
    p = T(p)
    hit = v0 > 0
    lx, lv = np.zeros(A, dtype=dtype), np.zeros(A, dtype=dtype)
    ls = np.zeros((A, m), dtype=_ctype(dtype))
    H = np.zeros((A, m), dtype=_ctype(dtype))
    gkap = np.zeros((A, m), dtype=dtype)
    gM, gkH = np.zeros(A, dtype=dtype), np.zeros(A, dtype=dtype)
    zc = np.conj(z)[None, :]
    for n in range(N - 1, -1, -1):
        delta, f, s = fw["delta"][:, n], fw["f"][:, n], fw["s"][n]
        on = (delta > 0) & hit
        dp = np.where(on, delta, T(1))
        lv = lv + h * lx
        a = zc * ls
        lf = gforce[:, n // R] / T(R) - (h / M) * lv + h * _seq_sum(a.real)
        ld = np.where(on, lf * kH * p * np.power(dp, p - T(1)), T(0))
        gkH = gkH + lf * np.where(on, np.power(dp, p), T(0))
        gM = gM + lv * h * f / (M * M)
        lx = lx + ld
        H = H + np.conj(s + (h * f)[:, None]) * a
        gkap = gkap - ld[:, None] * s.imag
        ls = a - 1j * (kap * ld[:, None])
    live = hit[:, None]
    H, gkap = np.where(live, H, 0), np.where(live, gkap, T(0))
    cw = c / w[None, :]
    return dict(gd=(-h * H.real).sum(0), gw=(h * H.imag - cw * cw * gkap).sum(0), gc=2 * cw * gkap,
                gM=np.where(hit, gM, T(0)), gv0=np.where(hit, lv, T(0)), gkH=np.where(hit, gkH, T(0)))


GRADS = ("gd", "gw", "gc", "gM", "gv0", "gkH")


# ---------------------------------------------------------------------------------------------------- bounds
def e64(ref64, truth):
    """(E64, scale) of one output: the float64 restatement's largest deviation from the longdouble truth over the output's
    largest magnitude, and that magnitude."""
    truth = np.asarray(truth, dtype=np.longdouble)
    scale = float(np.abs(truth).max())
    if scale == 0.0:
        return 0.0, 0.0
    return float(np.abs(np.asarray(ref64, dtype=np.longdouble) - truth).max()) / scale, scale


def bound(ref64, truth, stored32=False):
    """Per element: 8 max(E64, 2^-52) scale, plus 2^-24 |truth| for an output stored in fp32.  An output that is zero
    throughout admits only exact zeros."""
    E, scale = e64(ref64, truth)
    b = np.full(np.shape(truth), 8.0 * max(E, EPS64) * scale if scale > 0 else 0.0)
    if stored32:
        b = b + U32 * np.abs(np.asarray(truth, dtype=np.float64))
    return b


# ------------------------------------------------------------------------------------------- shapes and inputs
def modes(m, rng):
    """w [rad/s] of m modes between 200 Hz and 9 kHz, ascending, and the material damping d = 0.5 (5 + 1e-7 w^2)."""
    w = TWO_PI * np.sort(rng.uniform(200.0, 9000.0, m))
    return 0.5 * (5.0 + 1e-7 * w * w), w


# (A, m, F, R, p, kH, M, v0 of every clip, what the reference must show).  Properties: "ends" contact ends inside the window,
# "on" contact still on at the last substep, "none" a clip without contact (v0 <= 0), "double" a clip with two or more
# separate contact intervals, "zero_gain" a clip with a gain that is exactly zero, "mixed" clips with different hammers.
# m over {1, 5, 64, 70, 130}: lanes with 0, 1, 2 or 3 modes and a partly filled last round; A over {1, 3}; R over {1, 4, 8};
# F over {1, 2, 33, 64}; p over {1, 1.5, 2}.
CASES = [
    (1, 5, 64, 8, 1.5, (1e7,), (0.01,), (1.0,), ("ends",)),
    (1, 1, 64, 1, 1.5, (1e7,), (0.01,), (1.0,), ("ends",)),
    (1, 70, 32, 8, 1.5, (1e9,), (0.005,), (2.0,), ("double",)),
    (3, 5, 33, 4, 1.0, (1e7, 1e5, 1e7), (0.01, 0.02, 0.01), (1.0, 0.5, -1.0), ("ends", "on", "none", "mixed")),
    (3, 64, 2, 8, 2.0, (1e10, 1e10, 3e10), (0.01, 0.01, 0.02), (1.0, 0.0, 2.0), ("on", "none", "mixed")),
    (1, 130, 1, 8, 1.5, (1e7,), (0.01,), (1.0,), ("on",)),
    (1, 130, 1, 1, 1.5, (1e7,), (0.01,), (1.0,), ()),          # one substep: the hammer only just touches, all zeros
    (3, 130, 64, 4, 1.5, (1e7, 1e8, 1e9), (0.01, 0.004, 0.005), (1.0, 1.5, 2.0), ("ends", "zero_gain", "mixed")),
    (1, 64, 33, 1, 2.0, (1e10,), (0.01,), (1.0,), ("ends", "zero_gain")),
    (3, 70, 33, 8, 1.0, (1e6, 2e6, 4e6), (0.01, 0.01, 0.01), (1.0, 1.0, 1.0), ("ends", "mixed")),
]


def case_id(case):
    A, m, F, R, p = case[:5]
    return f"A{A}-m{m}-F{F}-R{R}-p{p}"


def inputs(case):
    """(d, w (m,), c (A, m), M, v0, kH (A,) fp64, gforce (A, F) fp32); fixed seed per case.  Gains uniform in 0.5 .. 1.5 with
    random signs (mass-orthonormal shapes of an object of about a kilogram), twice that in the "double" case (a lighter
    object recoils enough for the hammer to hit again); "zero_gain": every fifth gain of every clip is exactly zero."""
    A, m, F, R, p, kH, M, v0, props = case
    rng = np.random.default_rng([A, m, F, R, int(10 * p), 53])
    d, w = modes(m, rng)
    c = rng.uniform(0.5, 1.5, (A, m)) * rng.choice([-1.0, 1.0], (A, m))
    if "double" in props:
        c *= 2.0
    if "zero_gain" in props:
        c[:, ::5] = 0.0
    gforce = rng.standard_normal((A, F)).astype(np.float32)
    return d, w, c, np.array(M, dtype=np.float64), np.array(v0, dtype=np.float64), np.array(kH, dtype=np.float64), gforce


def contact_intervals(f_row):
    """Number of separate runs of f > 0 in one clip's substep forces."""
    on = np.asarray(f_row) > 0
    return int(on[0]) + int(np.count_nonzero(on[1:] & ~on[:-1]))


def properties(case, fw):
    """The properties the reference trajectory ``fw`` (a ``forward`` result) of ``case`` shows."""
    d, w, c, M, v0, kH, _ = inputs(case)
    f = np.asarray(fw["f"], dtype=np.float64)
    got = set()
    for a in range(f.shape[0]):
        k = contact_intervals(f[a])
        if k == 0 and v0[a] <= 0:
            got.add("none")
        if k >= 1 and f[a, -1] == 0:
            got.add("ends")
        if k >= 1 and f[a, -1] > 0:
            got.add("on")
        if k >= 2:
            got.add("double")
    if (c == 0).any():
        got.add("zero_gain")
    if len({(x, y, z) for x, y, z in zip(M, v0, kH)}) > 1:
        got.add("mixed")
    return got


# ---------------------------------------------------------------------------------------------------- recovery
RECOVERY = dict(m=5, F=64, R=8, p=1.5, kH=1e7, M=0.01, v0=1.0, steps=80, lr=0.05)


def recovery_problem():
    """(d, w, c, M, target kH, target v0): one clip of the first table case."""
    rng = np.random.default_rng(59)
    d, w = modes(RECOVERY["m"], rng)
    c = rng.uniform(0.5, 1.5, (1, RECOVERY["m"]))
    return d, w, c, np.array([RECOVERY["M"]]), np.array([RECOVERY["kH"]]), np.array([RECOVERY["v0"]])


def adam(loss_and_grad, theta, steps, lr, b1=0.9, b2=0.999, eps=1e-8):
    """Plain Adam on the float64 vector theta; ``loss_and_grad(theta) -> (loss, grad)``.  Returns (theta, losses) with the
    loss at every visited point, the last one included."""
    theta = np.array(theta, dtype=np.float64)
    mom, var = np.zeros_like(theta), np.zeros_like(theta)
    losses = []
    for t in range(1, steps + 1):
        loss, g = loss_and_grad(theta)
        losses.append(float(loss))
        mom = b1 * mom + (1 - b1) * g
        var = b2 * var + (1 - b2) * g * g
        theta = theta - lr * (mom / (1 - b1 ** t)) / (np.sqrt(var / (1 - b2 ** t)) + eps)
    losses.append(float(loss_and_grad(theta)[0]))
    return theta, losses


def recovery_numpy():
    """The recovery run on the restatement: theta = (log kH, v0) from (2 kH, 0.7 v0); returns the loss ratio end / start."""
    d, w, c, M, kH, v0 = recovery_problem()
    F, R, p = RECOVERY["F"], RECOVERY["R"], RECOVERY["p"]
    target = forward(d, w, c, M, v0, kH, F, p, R)["force"]

    def lg(theta):
        k, v = np.exp(theta[:1]), theta[1:]
        r = forward(d, w, c, M, v, k, F, p, R)["force"] - target
        g = adjoint(2 * r, d, w, c, M, v, k, p, R)
        return (r * r).sum(), np.array([g["gkH"][0] * k[0], g["gv0"][0]])

    _, losses = adam(lg, [np.log(2 * kH[0]), 0.7 * v0[0]], RECOVERY["steps"], RECOVERY["lr"])
    return losses[-1] / losses[0]
