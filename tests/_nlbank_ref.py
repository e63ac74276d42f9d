"""The tension-modulated bank of diffsound_amd/csrc/nlbank.hip (ds_nlbank_fwd / ds_nlbank_bwd) restated in numpy, its
adjoint, the bounds the kernel tests use and the cases they share.  Not a test module.

Per clip a, with h = 1 / (sr R), z_i = exp((-d_i + i w_i) h) and s_i = 0 at n = 0, for n = 0 .. S R - 1 and k = n // R:

    q_i   = Im s_i / w_i
    E_r   = sum_i C[r,i] q_i^2 ;  T_r = gamma[a,r] E_r      (r < K; added in ascending i, one term after the other)
    kap_i = sum_r C[r,i] T_r                                (ascending r)
    p_i   = c[a,i] f[a,k] - kap_i q_i                       (f[a,k] = 0 for k >= F)
    s_i   = z_i (s_i + h p_i)
    if n = k R + R - 1:  y[a,k] = sr sum_i amp[a,i] Im s_i

``forward`` and ``adjoint`` take the dtype (``np.float64`` or ``np.longdouble``) and do every operation in it; y is NOT
rounded to fp32 here.  The adjoint is the reverse sweep of nlbank.hip's header; what vouches for it is
tests/test_nlbank_ref_cpu.py: central differences of the longdouble forward.

Bounds: the error model of tests/_contact_ref.py, unchanged (``e64``, ``bound`` are its own functions).  The truth of an
output is the longdouble restatement, E64 the float64 restatement's largest deviation from it over the output's largest
magnitude; a kernel output passes when every element deviates by at most 8 max(E64, 2^-52) scale, y, stored in fp32, also
gets 2^-24 |ref| per element.  A strongly coupled multi-mode system can amplify rounding, so a case is admitted to the
device tests only if the reference alone shows E64 <= E64_MAX in every output: a condition on the inputs, held in
tests/test_nlbank_ref_cpu.py, not a tolerance."""
import functools

import numpy as np

from _contact_ref import EPS64, SR, TWO_PI, U32, _ctype, _seq_sum, adam, bound, e64, modes  # noqa: F401

E64_MAX = 1e-10


def _setup(d, w, c, amp, f, C, gamma, sr, R, dtype):
    T = np.dtype(dtype).type
    d, w, c, amp, f, C, gamma = (np.asarray(x, dtype=dtype) for x in (d, w, c, amp, f, C, gamma))
    h = T(1) / (T(sr) * T(R))
    e = np.exp(-d * h)
    z = (e * np.cos(w * h) + 1j * (e * np.sin(w * h))).astype(_ctype(dtype))
    return T, d, w, c, amp, f, C, gamma, h, z


def _tension(s, w, C, gamma):
    """q, q^2 (A, m), E, T (A, K) and kap (A, m) of the states s (A, m): the part of a substep that the forward and the
    reverse sweep share."""
    q = s.imag / w[None, :]
    q2 = q * q
    E = np.stack([_seq_sum(C[r][None, :] * q2) for r in range(C.shape[0])], axis=-1)
    Tn = gamma * E
    kap = np.zeros_like(q)
    for r in range(C.shape[0]):
        kap = kap + C[r][None, :] * Tn[:, r:r + 1]
    return q, q2, E, Tn, kap


def forward(d, w, c, amp, f, C, gamma, S, R=8, sr=SR, dtype=np.float64, keep=False):
    """dict: y (A, S); s_end (A, m); kap_max (A, m), the largest stiffening kap_i each mode saw; ``keep`` adds s (S R, A, m),
    the states that enter each substep.  d, w (m,), c, amp (A, m), f (A, F), C (K, m), gamma (A, K)."""
    T, d, w, c, amp, f, C, gamma, h, z = _setup(d, w, c, amp, f, C, gamma, sr, R, dtype)
    A, m = c.shape
    F = f.shape[1]
    s = np.zeros((A, m), dtype=_ctype(dtype))
    y = np.zeros((A, S), dtype=dtype)
    kap_max = np.zeros((A, m), dtype=dtype)
    states = np.zeros((S * R, A, m), dtype=_ctype(dtype)) if keep else None
    zero = np.zeros(A, dtype=dtype)
    for n in range(S * R):
        k = n // R
        fk = f[:, k] if k < F else zero
        q, _, _, _, kap = _tension(s, w, C, gamma)
        kap_max = np.maximum(kap_max, kap)
        p = c * fk[:, None] - kap * q
        if keep:
            states[n] = s
        s = z[None, :] * (s + h * p)
        if n % R == R - 1:
            y[:, k] = T(sr) * _seq_sum(amp * s.imag)
    out = dict(y=y, s_end=s, kap_max=kap_max, h=h)
    if keep:
        out["s"] = states
    return out


def adjoint(gy, d, w, c, amp, f, C, gamma, R=8, sr=SR, dtype=np.float64, per_clip=False):
    """dict gd, gw (m,), gc, gamp (A, m), gf (A, F), gC (K, m), ggamma (A, K) of sum(gy * y): the reverse sweep.  gd, gw and
    gC are the clips' partials added in ascending order; ``per_clip`` adds the partials themselves as gd_a, gw_a (A, m) and
    gC_a (A, K, m)."""
    gy = np.asarray(gy, dtype=dtype)
    A, S = gy.shape
    fw = forward(d, w, c, amp, f, C, gamma, S, R, sr, dtype, keep=True)
    T, d, w, c, amp, f, C, gamma, h, z = _setup(d, w, c, amp, f, C, gamma, sr, R, dtype)
    m, K, F = c.shape[1], C.shape[0], f.shape[1]
    ls = np.zeros((A, m), dtype=_ctype(dtype))
    H = np.zeros((A, m), dtype=_ctype(dtype))
    gc, gamp, gq = (np.zeros((A, m), dtype=dtype) for _ in range(3))
    gf = np.zeros((A, F), dtype=dtype)
    gC = np.zeros((A, K, m), dtype=dtype)
    ggamma = np.zeros((A, K), dtype=dtype)
    zc = np.conj(z)[None, :]
    zero = np.zeros(A, dtype=dtype)
    s_next = fw["s_end"]
    for n in range(S * R - 1, -1, -1):
        k = n // R
        fk = f[:, k] if k < F else zero
        s = fw["s"][n]
        q, q2, E, Tn, kap = _tension(s, w, C, gamma)
        p = c * fk[:, None] - kap * q
        if n % R == R - 1:
            gk = T(sr) * gy[:, k]
            ls = ls + 1j * (amp * gk[:, None])
            gamp = gamp + gk[:, None] * s_next.imag
        a = zc * ls
        lp = h * a.real
        if k < F:
            gf[:, k] += _seq_sum(c * lp)
        gc = gc + fk[:, None] * lp
        lkap = -(q * lp)
        lq = -(kap * lp)
        for r in range(K):
            lT = _seq_sum(C[r][None, :] * lkap)
            gC[:, r] = gC[:, r] + Tn[:, r:r + 1] * lkap
            ggamma[:, r] = ggamma[:, r] + lT * E[:, r]
            lE = gamma[:, r] * lT
            gC[:, r] = gC[:, r] + lE[:, None] * q2
            lq = lq + (T(2) * lE)[:, None] * (C[r][None, :] * q)
        H = H + np.conj(s + h * p) * a
        gq = gq + lq * q
        ls = a + 1j * (lq / w[None, :])
        s_next = s
    gd = T(0) - h * H.real
    gw = h * H.imag - gq / w[None, :]
    out = dict(gd=_asc_sum(gd), gw=_asc_sum(gw), gc=gc, gamp=gamp, gf=gf, gC=_asc_sum(gC), ggamma=ggamma)
    if per_clip:
        out.update(gd_a=gd, gw_a=gw, gC_a=gC)
    return out


def _asc_sum(x):
    """Sum over the clips in ascending order."""
    return np.cumsum(x, axis=0)[-1]


GRADS = ("gd", "gw", "gc", "gamp", "gf", "gC", "ggamma")


# ------------------------------------------------------------------------------------------- shapes and inputs
GLIDE = 0.2  # kap_0 / w_0^2 that a clip's couplings are scaled to on the LINEAR response's peak (the stiffened one stays below)

# (A, m, K, R, F, S, what each clip is).  "hard": a strike scaled to GLIDE; "linear": gamma = 0 throughout; "idle": a force of
# zeros (its gamma is the first clip's).  m over {1, 3, 5, 65, 70, 130, 260}: NM = 1, 2, 4 and 8, lanes with a slot past m and
# one slot a lane past m; K over 1..4; R over {1, 2, 4, 8, 64}; F < S, F = S, F = S + 3, and F = 70 and 130: two and three
# chunks of the force.
CASES = [
    (1, 1, 1, 1, 64, 64, ("hard",)),               # the Duffing oscillator, one lane live
    (1, 3, 2, 8, 20, 24, ("hard",)),               # F < S
    (1, 65, 1, 4, 35, 32, ("hard",)),              # F = S + 3: the tail is not read
    (1, 260, 4, 2, 40, 40, ("hard",)),             # NM = 8 with K = 4
    (1, 5, 2, 64, 5, 5, ("hard",)),
    (3, 5, 2, 4, 70, 70, ("hard", "linear", "idle")),
    (1, 130, 3, 1, 130, 133, ("hard",)),
    (3, 70, 4, 8, 33, 33, ("hard", "linear", "idle")),
]
KINDS = ("hard", "linear", "idle")


def case_id(case):
    A, m, K, R, F, S = case[:6]
    return f"A{A}-m{m}-K{K}-R{R}-F{F}-S{S}"


def strike(F, rng):
    """(F,) a raised-cosine pulse over the first 12 samples (or F, if that is less) of about 1 N, with 5 % of noise on every
    sample, so that no sample's force - and no sample's gradient - is a trivial one."""
    k = np.arange(F, dtype=np.float64)
    L = min(F, 12)
    pulse = np.where(k < L, 0.5 - 0.5 * np.cos(TWO_PI * (k + 0.5) / L), 0.0)
    return pulse + 0.05 * rng.standard_normal(F)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(d, w (m,), c, amp (A, m), f (A, F), C (K, m), gamma (A, K) fp64, gy (A, S) fp32); fixed seed per case.  Gains uniform
    in 0.5 .. 1.5 with random signs; C uniform in 0.5 .. 1.5 with an exact zero at every (i + 2 r) mod 7 = 5 (never at the
    lowest mode).  gamma of a "hard" clip: GLIDE w_0^2 / (K C[r,0] Epk_r) with Epk_r the largest E_r of the clip's LINEAR
    response (float64 restatement, gamma = 0), so that at that peak every term stiffens the lowest mode by GLIDE w_0^2 / K."""
    A, m, K, R, F, S, kinds = case
    rng = np.random.default_rng([A, m, K, R, F, S, 71])
    d, w = modes(m, rng)
    c = rng.uniform(0.5, 1.5, (A, m)) * rng.choice([-1.0, 1.0], (A, m))
    amp = rng.uniform(0.5, 1.5, (A, m)) * rng.choice([-1.0, 1.0], (A, m))
    C = rng.uniform(0.5, 1.5, (K, m))
    r_idx, i_idx = np.meshgrid(np.arange(K), np.arange(m), indexing="ij")
    C[(i_idx + 2 * r_idx) % 7 == 5] = 0.0
    f = np.stack([strike(F, rng) if kind != "idle" else np.zeros(F) for kind in kinds])
    gy = rng.standard_normal((A, S)).astype(np.float32)
    gamma = np.zeros((A, K))
    lin = forward(d, w, c, amp, f, C, gamma, S, R, keep=True)
    q = lin["s"].imag / w[None, None, :]
    Epk = np.stack([(C[r][None, None, :] * q * q).sum(-1).max(0) for r in range(K)], axis=-1)  # (A, K)
    for a, kind in enumerate(kinds):
        if kind == "hard":
            gamma[a] = GLIDE * w[0] ** 2 / (K * C[:, 0] * Epk[a])
    for a, kind in enumerate(kinds):
        if kind == "idle":
            gamma[a] = gamma[0]
    return d, w, c, amp, f, C, gamma, gy


def glide(case, fw):
    """(A,) the relative rise of the lowest mode's frequency at the largest stiffening the reference trajectory ``fw`` shows:
    sqrt(1 + kap_0 / (w_0^2 + d_0^2)) - 1."""
    d, w = inputs(case)[:2]
    return np.sqrt(1.0 + np.asarray(fw["kap_max"][:, 0], dtype=np.float64) / (w[0] ** 2 + d[0] ** 2)) - 1.0


def stability(case, fw):
    """h sqrt(max_i kap_i) of every clip at the largest stiffening reached: the explicit scheme wants this well below 2."""
    return np.sqrt(np.asarray(fw["kap_max"], dtype=np.float64).max(-1)) / (SR * case[3])


# ---------------------------------------------------------------------------------------------------- recovery
RECOVERY = dict(m=5, K=1, S=64, R=8, steps=80, lr=0.05, off=2.0)


@functools.lru_cache(maxsize=None)
def recovery_problem():
    """(d, w, c, amp, f (1, S), C (1, m), target gamma (1, 1)): one hard strike."""
    case = (1, RECOVERY["m"], RECOVERY["K"], RECOVERY["R"], RECOVERY["S"], RECOVERY["S"], ("hard",))
    d, w, c, amp, f, C, gamma, _ = inputs(case)
    return d, w, c, amp, f, C, gamma


def recovery_start():
    return np.log(RECOVERY["off"] * recovery_problem()[6])


@functools.lru_cache(maxsize=None)
def recovery_numpy():
    """The recovery run on the restatement: theta = log gamma from a start a factor 2 off, the loss the squared error of y;
    returns the losses at every visited point."""
    d, w, c, amp, f, C, gamma = recovery_problem()
    S, R = RECOVERY["S"], RECOVERY["R"]
    target = forward(d, w, c, amp, f, C, gamma, S, R)["y"]

    def lg(theta):
        g = np.exp(theta).reshape(1, -1)
        r = forward(d, w, c, amp, f, C, g, S, R)["y"] - target
        adj = adjoint(2 * r, d, w, c, amp, f, C, g, R)
        return (r * r).sum(), (adj["ggamma"] * g).reshape(-1)

    _, losses = adam(lg, recovery_start().reshape(-1), RECOVERY["steps"], RECOVERY["lr"])
    return np.array(losses)
