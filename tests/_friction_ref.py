"""The friction scheme of diffsound_amd/csrc/friction.hip (ds_friction_fwd / ds_friction_bwd) restated in numpy, its
adjoint, the bounds the kernel tests use and the cases they share.  Not a test module.

Per clip a, with h = 1 / (sr R), z_i = exp((-d_i + i w_i) h), g_i = c[a,i]^2, r_i = d_i / w_i, s_i = 0 at n = 0, for
n = 0 .. F R - 1 and k = n // R:

    v   = sum_i g_i (Re s_i - r_i Im s_i)        (added in ascending i, one term after the other)
    vr  = vb[a,k] - v ;  x = vr / vs[a]
    phi = x exp((1 - x^2) / 2) ;  f = N[a,k] phi
    force[a,k] += f / R
    s_i = z_i (s_i + h f)

``forward`` and ``adjoint`` take the dtype (``np.float64`` or ``np.longdouble``) and do every operation in it; the force
is NOT rounded to fp32 here.  The adjoint is the reverse sweep of friction.hip's header; what vouches for it is
tests/test_friction_ref_cpu.py: central differences of the longdouble forward.

Bounds: the error model of tests/_contact_ref.py, unchanged (``e64``, ``bound`` are its own functions).  The truth of an
output is the longdouble restatement, E64 the float64 restatement's largest deviation from it over the output's largest
magnitude; a kernel output passes when every element deviates by at most 8 max(E64, 2^-52) scale, the force, stored in
fp32, also gets 2^-24 |ref| per element.  Self-sustained friction amplifies rounding (the falling branch of phi is a
negative damper), so a case is admitted to the device tests only if the reference alone shows E64 <= E64_MAX in every
output: a condition on the inputs, held in tests/test_friction_ref_cpu.py, not a tolerance."""
import numpy as np

from _contact_ref import EPS64, SR, TWO_PI, U32, _ctype, _seq_sum, adam, bound, e64, modes  # noqa: F401

E64_MAX = 1e-10


def _setup(d, w, c, vb, N, vs, sr, R, dtype):
    T = np.dtype(dtype).type
    d, w, c, vb, N, vs = (np.asarray(x, dtype=dtype) for x in (d, w, c, vb, N, vs))
    h = T(1) / (T(sr) * T(R))
    e = np.exp(-d * h)
    z = (e * np.cos(w * h) + 1j * (e * np.sin(w * h))).astype(_ctype(dtype))
    return T, d, w, c, vb, N, vs, h, z, c * c, d / w


def _phi(vr, vs, T):
    x = vr / vs
    e = np.exp((T(1) - x * x) / T(2))
    return x, e, x * e


def forward(d, w, c, vb, N, vs, R=8, sr=SR, dtype=np.float64, keep=False):
    """dict: force (A, F); f, vr, v (A, F R) per substep; s_end (A, m); ``keep`` adds s (F R, A, m), the states that enter
    each substep.  d, w (m,), c (A, m), vb, N (A, F), vs (A,)."""
    T, d, w, c, vb, N, vs, h, z, g, r = _setup(d, w, c, vb, N, vs, sr, R, dtype)
    A, m = c.shape
    F = vb.shape[1]
    n_sub = F * R
    s = np.zeros((A, m), dtype=_ctype(dtype))
    force = np.zeros((A, F), dtype=dtype)
    fs, vrs, vels = (np.zeros((A, n_sub), dtype=dtype) for _ in range(3))
    S = np.zeros((n_sub, A, m), dtype=_ctype(dtype)) if keep else None
    for n in range(n_sub):
        k = n // R
        v = _seq_sum(g * (s.real - r[None, :] * s.imag))
        vr = vb[:, k] - v
        _, _, phi = _phi(vr, vs, T)
        f = N[:, k] * phi
        force[:, k] += f / T(R)
        fs[:, n], vrs[:, n], vels[:, n] = f, vr, v
        if keep:
            S[n] = s
        s = z[None, :] * (s + (h * f)[:, None])
    out = dict(force=force, f=fs, vr=vrs, v=vels, s_end=s, h=h)
    if keep:
        out["s"] = S
    return out


def adjoint(gforce, d, w, c, vb, N, vs, R=8, sr=SR, dtype=np.float64):
    """dict gd, gw (m,), gc (A, m), gvb, gN (A, F), gvs (A,) of sum(gforce * force): the reverse sweep."""
    gforce = np.asarray(gforce, dtype=dtype)
    fw = forward(d, w, c, vb, N, vs, R, sr, dtype, keep=True)
    T, d, w, c, vb, N, vs, h, z, g, r = _setup(d, w, c, vb, N, vs, sr, R, dtype)
    A, m = c.shape
    F = vb.shape[1]
    ls = np.zeros((A, m), dtype=_ctype(dtype))
    H = np.zeros((A, m), dtype=_ctype(dtype))
    gg, gr = np.zeros((A, m), dtype=dtype), np.zeros((A, m), dtype=dtype)
    gvb, gN, gvs = np.zeros((A, F), dtype=dtype), np.zeros((A, F), dtype=dtype), np.zeros(A, dtype=dtype)
    zc = np.conj(z)[None, :]
    for n in range(F * R - 1, -1, -1):
        k = n // R
        s = fw["s"][n]
        x, e, phi = _phi(fw["vr"][:, n], vs, T)
        f = N[:, k] * phi
        a = zc * ls
        lf = gforce[:, k] / T(R) + h * _seq_sum(a.real)
        dphi = ((T(1) - x * x) * e) / vs
        lvr = (lf * N[:, k]) * dphi
        gN[:, k] += lf * phi
        gvb[:, k] += lvr
        gvs = gvs - lvr * x
        H = H + np.conj(s + (h * f)[:, None]) * a
        lg = lvr[:, None] * g
        gg = gg - lvr[:, None] * (s.real - r[None, :] * s.imag)
        gr = gr + lg * s.imag
        ls = (a.real - lg) + 1j * (a.imag + lg * r[None, :])
    gd = (T(0) - h * H.real) + gr / w[None, :]
    gw = h * H.imag - gr * d[None, :] / (w * w)[None, :]
    return dict(gd=_asc_sum(gd), gw=_asc_sum(gw), gc=T(2) * c * gg, gvb=gvb, gN=gN, gvs=gvs)


def _asc_sum(x):
    """Sum over the clips in ascending order."""
    return np.cumsum(x, axis=0)[-1]


GRADS = ("gd", "gw", "gc", "gvb", "gN", "gvs")


# ------------------------------------------------------------------------------------------- shapes and inputs
VS = 0.1  # the friction curve's peak velocity of a table case's first clip [m/s]; clip a has (1 + 0.1 a) times that

# What a clip's gesture is, and what the reference's vr must show for it (``properties``):
#   "slip"     the bow runs at 3 vs: |vr| > vs at every substep
#   "stick"    a slow bow under a large normal force: |vr| < vs from a quarter of the window on
#   "self"     a bow at 1.01 vs whose load lets the modes swing across the peak: three or more crossings of |vr| = vs
#   "reversal" the bow's velocity changes sign inside the window
#   "release"  the normal force is positive at first and exactly 0 from the middle of the window on
#   "idle"     N = 0 throughout: exact zeros
# (A, m, F, R, the clips' gestures, further properties: "zero_gain" every fifth gain exactly zero, "mixed" clips that differ).
# m over {1, 5, 64, 70, 130}: lanes with 0, 1, 2 or 3 modes (NM = 1, 2 and 4) and a partly filled last round; A over {1, 3};
# R over {1, 4, 8, 64}; F over {1, 2, 32, 33, 64}.
CASES = [
    (1, 5, 64, 8, ("self",), ()),
    (1, 1, 64, 1, ("slip",), ()),
    (1, 70, 32, 8, ("stick",), ()),
    (3, 5, 33, 4, ("self", "reversal", "idle"), ("mixed",)),
    (3, 64, 2, 64, ("slip", "idle", "release"), ("mixed",)),
    (1, 130, 1, 8, ("slip",), ()),
    (1, 130, 1, 1, ("slip",), ()),
    (3, 130, 64, 4, ("release", "self", "reversal"), ("zero_gain", "mixed")),
    (1, 64, 33, 1, ("reversal",), ("zero_gain",)),
    (3, 70, 33, 8, ("stick", "slip", "self"), ("mixed",)),
    (1, 5, 32, 64, ("self",), ()),
]
KINDS = ("slip", "stick", "self", "reversal", "release", "idle")


def case_id(case):
    A, m, F, R = case[:4]
    return f"A{A}-m{m}-F{F}-R{R}"


def gesture(kind, F, VS, rng):
    """(vb, N) (F,) of one clip whose friction curve peaks at VS."""
    k = np.arange(F, dtype=np.float64)
    wobble = 1.0 + 0.05 * rng.standard_normal(F)
    if kind == "slip":
        return 3 * VS * wobble, 40.0 * wobble[::-1]
    if kind == "stick":
        return 0.1 * VS * wobble, 300.0 * np.ones(F)
    if kind == "self":
        return 1.01 * VS * np.ones(F), 120.0 * np.ones(F)
    if kind == "reversal":
        return 3 * VS * np.cos(np.pi * (k + 0.5) / F) * wobble if F > 1 else 3 * VS * wobble, 40.0 * np.ones(F)
    if kind == "release":
        N = 40.0 * wobble
        N[(F + 1) // 2:] = 0.0
        return 2 * VS * np.ones(F), N
    assert kind == "idle", kind
    return 5 * VS * wobble, np.zeros(F)


def inputs(case):
    """(d, w (m,), c (A, m), vb, N (A, F), vs (A,) fp64, gforce (A, F) fp32); fixed seed per case.  Gains uniform in
    0.5 .. 1.5 over sqrt(m) with random signs, so that sum_i g_i, the object's admittance at the contact (1 / kg), is about
    1 whatever m is; "zero_gain": every fifth gain of every clip is exactly zero."""
    A, m, F, R, kinds, props = case
    rng = np.random.default_rng([A, m, F, R, 61])
    d, w = modes(m, rng)
    c = rng.uniform(0.5, 1.5, (A, m)) * rng.choice([-1.0, 1.0], (A, m)) / np.sqrt(m)
    if "zero_gain" in props:
        c[:, ::5] = 0.0
    vs = VS * (1.0 + 0.1 * np.arange(A))
    pairs = [gesture(kind, F, vs[a], rng) for a, kind in enumerate(kinds)]
    vb, N = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    gforce = rng.standard_normal((A, F)).astype(np.float32)
    return d, w, c, vb, N, vs, gforce


def stability(case):
    """h max(N) (sqrt(e) / vs) sum_i g_i of every clip: the explicit scheme wants this well below 2."""
    d, w, c, vb, N, vs, _ = inputs(case)
    return N.max(-1) * np.sqrt(np.e) / vs * (c * c).sum(-1) / (SR * case[3])


def crossings(vr_row, vs):
    """Number of times |vr| passes vs from one substep to the next."""
    out = np.abs(np.asarray(vr_row, dtype=np.float64)) > vs
    return int(np.count_nonzero(out[1:] != out[:-1]))


def clip_shows(kind, vr, vb, N, vs):
    """The reference's vr (F R,) of a clip and its gesture show ``kind``."""
    vr = np.abs(np.asarray(vr, dtype=np.float64))
    if kind == "slip":
        return bool((vr > vs).all() and (N > 0).all())
    if kind == "stick":
        return bool((vr[len(vr) // 4:] < vs).all() and (N > 0).all())
    if kind == "self":
        return crossings(vr, vs) >= 3
    if kind == "reversal":
        return bool(vb.min() < 0 < vb.max())
    if kind == "release":
        return bool(N[0] > 0 and N[-1] == 0)
    return not N.any()


def properties(case, fw):
    """The properties the reference trajectory ``fw`` (a ``forward`` result) of ``case`` shows."""
    d, w, c, vb, N, vs, _ = inputs(case)
    got = {kind for a, kind in enumerate(case[4]) if clip_shows(kind, fw["vr"][a], vb[a], N[a], vs[a])}
    if (c == 0).any():
        got.add("zero_gain")
    if len(set(case[4])) > 1:
        got.add("mixed")
    return got


# ---------------------------------------------------------------------------------------------------- the bow
def envelope(F, sr, attack, release, dtype=np.float64):
    """The fixed raised-cosine envelope of ``Bow``: a rise over ``attack`` seconds from sample 0, a fall over ``release``
    seconds to the last sample, their product."""
    k = np.arange(F, dtype=dtype)
    rise = 0.5 - 0.5 * np.cos(np.pi * np.minimum(k / (attack * sr), 1.0)) if attack > 0 else np.ones(F, dtype=dtype)
    fall = 0.5 - 0.5 * np.cos(np.pi * np.minimum((F - 1 - k) / (release * sr), 1.0)) if release > 0 else np.ones(F, dtype=dtype)
    return rise * fall


# ---------------------------------------------------------------------------------------------------- recovery
RECOVERY = dict(m=5, F=64, R=8, pressure=60.0, velocity=0.15, vs=VS, attack=8 / SR, release=8 / SR, steps=80, lr=0.05)


def recovery_problem():
    """(d, w, c, envelope (F,), target pressure, target velocity): one clip that slips, close to the friction peak."""
    rng = np.random.default_rng(67)
    d, w = modes(RECOVERY["m"], rng)
    c = rng.uniform(0.5, 1.5, (1, RECOVERY["m"])) / np.sqrt(RECOVERY["m"])
    env = envelope(RECOVERY["F"], SR, RECOVERY["attack"], RECOVERY["release"])
    return d, w, c, env, RECOVERY["pressure"], RECOVERY["velocity"]


def recovery_start():
    return [np.log(1.5 * RECOVERY["pressure"]), 0.8 * RECOVERY["velocity"]]


def recovery_numpy():
    """The recovery run on the restatement: theta = (log pressure, velocity) from (1.5 pressure, 0.8 velocity); returns the
    loss ratio end / start."""
    d, w, c, env, P, V = recovery_problem()
    R, vs = RECOVERY["R"], np.array([RECOVERY["vs"]])
    target = forward(d, w, c, V * env[None, :], P * env[None, :], vs, R)["force"]

    def lg(theta):
        p, v = np.exp(theta[0]), theta[1]
        vb, N = v * env[None, :], p * env[None, :]
        r = forward(d, w, c, vb, N, vs, R)["force"] - target
        g = adjoint(2 * r, d, w, c, vb, N, vs, R)
        return (r * r).sum(), np.array([(g["gN"][0] * env).sum() * p, (g["gvb"][0] * env).sum()])

    _, losses = adam(lg, recovery_start(), RECOVERY["steps"], RECOVERY["lr"])
    return losses[-1] / losses[0]
