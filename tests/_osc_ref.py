"""References and per-sample error bounds for the oscillator kernels of diffsound_amd/csrc/oscillator.hip (not a test
module).

The references are NumPy fp64 restatements of what the kernels compute, accurate to a few fp64 roundings, so that a
test may ask the device for its own fp32 roundings and nothing more:

``tv_forward`` / ``tv_backward``   the time-varying bank (ds_osc_tv_fwd / ds_osc_tv_bwd),
``bank_forward`` / ``bank_backward`` the closed-form bank (ds_osc_bank_fwd / ds_osc_bank_bwd),
``fir`` / ``corr``                  the causal force FIR and its adjoint,
``bound_*``                         what the device result may differ from the reference by, derived from the code,
``round_like_kernel``               the kernels' fp32 roundings applied to fp64 mode signals (a CPU model of the forward),
``torch_tv_chain`` / ``torch_bank_chain``  the same maps as torch ops, for fp64 autograd.

Two places need more than a plain fp64 evaluation to stay well inside the bounds.  The running sums of the time-varying
bank are taken exactly (``_prefix``): a plain fp64 cumsum of a phase that reaches 10^3 turns is off by ~1e-12 turns,
which is the size of the fp64 term of the gradient bounds.  The phase w tau of the closed form (up to ~7e3 rad) is formed
in extended precision for the same reason.  Both kernels keep their phase small by construction (floor of the carry; a
phasor seeded once per lane), so the references must not be the less accurate side."""
import numpy as np

U32 = 2.0 ** -24       # unit roundoff of fp32
TWO_PI = 2.0 * np.pi
TV_MODES_PER_GROUP = 16  # modes summed in fp64 into one fp32 partial signal by osc_tv_modes_kernel
BANK_PARTIALS = 4        # waves of osc_fwd_kernel, each rounding its fp64 mode sum to fp32 once

_LD = np.longdouble


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _prefix(v):
    """Inclusive running sum of fp64 ``v`` over the last axis as an unevaluated pair (hi, lo), hi + lo = the sum.

    v is split into hi = the nearest multiple of 2^-40 and lo = v - hi (exact, |lo| <= 2^-41).  Sums of the hi parts are
    multiples of 2^-40 below 2^13 in magnitude, so fp64 adds them without rounding; the lo parts sum to at most
    S 2^-41, where an fp64 rounding is below 2^-80.  Valid while |sum| < 2^13 (phase below 8192 turns)."""
    q = 2.0 ** -40
    hi = np.round(v / q) * q
    lo = v - hi
    H = np.cumsum(hi, axis=-1)
    assert np.abs(H).max(initial=0.0) < 2.0 ** 13
    return H, np.cumsum(lo, axis=-1)


def _suffix(x):
    """sum_{t' >= t} x[..., t'] in extended precision, returned as fp64."""
    return np.cumsum(x[..., ::-1].astype(_LD), axis=-1)[..., ::-1].astype(np.float64)


def fir(s, force):
    """y[a, t] = sum_f force[a, f] s[a, t - f], t < S (causal FIR cropped to S).  fp64."""
    s, force = _f64(s), _f64(force)
    S = s.shape[-1]
    y = np.zeros_like(s)
    for f in range(min(force.shape[-1], S)):
        y[:, f:] += force[:, f:f + 1] * s[:, :S - f]
    return y


def corr(gy, force):
    """gs[a, t] = sum_f force[a, f] gy[a, t + f] (adjoint of ``fir``).  fp64."""
    gy, force = _f64(gy), _f64(force)
    S = gy.shape[-1]
    gs = np.zeros_like(gy)
    for f in range(min(force.shape[-1], S)):
        gs[:, :S - f] += force[:, f:f + 1] * gy[:, f:]
    return gs


def _amp(amp, A, m):
    return np.ones((A, m)) if amp is None else _f64(amp).reshape(A, m)


# ------------------------------------------------------------------------------------------ time-varying bank
def tv_modes(dmp, frq, sr):
    """(e^{-D}, sin(2 pi P), cos(2 pi P)) of every (clip, mode, sample): D = cumsum(dmp * (1/sr)), P = cumsum(frq * (1/sr)),
    both inclusive; the products are the fp64 products the kernel forms, the sums are exact (``_prefix``)."""
    inv = 1.0 / float(sr)
    Dh, Dl = _prefix(_f64(dmp) * inv)
    Ph, Pl = _prefix(_f64(frq) * inv)
    ph = (Ph - np.floor(Ph)) + Pl  # whole turns leave exactly; one rounding
    return np.exp(-(Dh + Dl)), np.sin(TWO_PI * ph), np.cos(TWO_PI * ph)


def tv_mode_signals(dmp, frq, amp, sr):
    """amp e^{-D} sin(2 pi P) per (clip, mode, sample): what osc_tv_modes_kernel sums over modes."""
    A, m, _ = np.shape(dmp)
    env, sn, _ = tv_modes(dmp, frq, sr)
    return _amp(amp, A, m)[:, :, None] * env * sn


def tv_forward(dmp, frq, amp, force, sr):
    """ds_osc_tv_fwd: dmp, frq (A, m, S) fp32 (promoted exactly), amp (A, m) or None, force (A, F).
    Returns (y (A, S), E (A, S)) with the envelope E[a, t] = sum_m |amp| e^{-D}."""
    A, m, _ = np.shape(dmp)
    env, sn, _ = tv_modes(dmp, frq, sr)
    am = _amp(amp, A, m)[:, :, None]
    return fir((am * env * sn).sum(1), force), (np.abs(am) * env).sum(1)


def tv_backward(gs, dmp, frq, amp, sr):
    """ds_osc_tv_bwd after the correlation: with u_t = gs_t amp e^{-D_t}, gD_t = -u_t sin(2 pi P_t),
    gP_t = 2 pi u_t cos(2 pi P_t):  g_dmp[t] = (1/sr) sum_{t' >= t} gD_t', g_frq[t] = (1/sr) sum_{t' >= t} gP_t',
    gamp = sum_t gs_t e^{-D_t} sin(2 pi P_t).
    Returns (g_dmp, g_frq (A, m, S), gamp (A, m), U (A, m) = sum_t |u_t|, V (A, m) = sum_t |gs_t e^{-D_t}|)."""
    A, m, _ = np.shape(dmp)
    inv = 1.0 / float(sr)
    env, sn, cs = tv_modes(dmp, frq, sr)
    ge = _f64(gs)[:, None, :] * env
    u = ge * _amp(amp, A, m)[:, :, None]
    g_dmp = _suffix(-u * sn) * inv
    g_frq = _suffix(TWO_PI * u * cs) * inv
    return g_dmp, g_frq, (ge * sn).sum(-1), np.abs(u).sum(-1), np.abs(ge).sum(-1)


# -------------------------------------------------------------------------------------------- closed-form bank
def bank_modes(d, w, S, sr):
    """(tau (S,), e^{-d tau}, sin(w tau), cos(w tau) (m, S)) at tau = (t + 1) * (1/sr), 1/sr the fp64 number the kernels
    are handed.  w tau is formed in extended precision: in fp64 its rounding alone (|w tau| 2^-53, ~1e-12 rad at
    15 kHz and 2500 samples) would be as large as the bound on gd / gw."""
    inv = 1.0 / float(sr)
    n = np.arange(1, S + 1)
    tau = n * inv
    ph = (_f64(w).astype(_LD)[:, None] * n.astype(_LD)[None, :]) * _LD(inv)
    return tau, np.exp(-_f64(d)[:, None] * tau[None, :]), np.sin(ph).astype(np.float64), np.cos(ph).astype(np.float64)


def bank_mode_signals(d, w, amp, A, S, sr):
    """amp e^{-d tau} sin(w tau) per (clip, mode, sample): what osc_fwd_kernel sums over modes."""
    _, env, sn, _ = bank_modes(d, w, S, sr)
    return _amp(amp, A, len(env))[:, :, None] * (env * sn)[None]


def bank_forward(d, w, amp, force, S, sr):
    """ds_osc_bank_fwd: d, w (m,) fp64, amp (A, m) or None, force (A, F).  Returns (y (A, S), E (A, S)),
    E[a, t] = sum_m |amp| e^{-d tau}."""
    A = np.shape(force)[0]
    _, env, sn, _ = bank_modes(d, w, S, sr)
    am = _amp(amp, A, len(env))
    return fir(am @ (env * sn), force), np.abs(am) @ env


def bank_backward(gs, d, w, amp, sr):
    """ds_osc_bank_bwd after the correlation: gd[m] = -sum_{a,t} amp gs tau e^{-d tau} sin(w tau),
    gw[m] = sum_{a,t} amp gs tau e^{-d tau} cos(w tau), gamp[a, m] = sum_t gs e^{-d tau} sin(w tau).
    Returns (gd, gw (m,), gamp (A, m), W (m,) = sum_{a,t} |amp gs tau e^{-d tau}|, V (A, m) = sum_t |gs e^{-d tau}|)."""
    gs = _f64(gs)
    A, S = gs.shape
    tau, env, sn, cs = bank_modes(d, w, S, sr)
    am = _amp(amp, A, len(env))
    gt = gs * tau[None, :]
    gd = -((am.T @ gt) * (env * sn)).sum(-1)
    gw = ((am.T @ gt) * (env * cs)).sum(-1)
    W = ((np.abs(am).T @ np.abs(gt)) * env).sum(-1)
    return gd, gw, gs @ (env * sn).T, W, np.abs(gs) @ env.T


# ------------------------------------------------------------------------------------------------------ bounds
def tv_partials(m):
    return -(-m // TV_MODES_PER_GROUP)


def bound_y(force, E, partials):
    """|y - ref|[a, t] <= 2 (F + P + 1) u sum_f |force[a, f]| E[a, t - f],  u = 2^-24, P = ``partials``.

    Both forward kernels evaluate every mode in fp64 (error ~2^-50 E, nothing at this scale) and then round in fp32:
      * each of the P partial signals (16 modes of a workgroup in the time-varying kernel, the modes of one wave in
        the closed-form kernel) is rounded to fp32 once: error <= u |partial|, and sum_p |partial_p| <= E;
      * the P partials are added in fp32, P - 1 roundings of a running sum that never exceeds E (1 + u)^P: <= (P - 1) u E;
        so the signal s the FIR reads has |s_hat - s| <= P u E to first order;
      * the FIR is F sequential fp32 fmas: |fl(sum) - sum| <= gamma_F sum_f |force_f| |s_hat[t - f]|, gamma_F ~ F u.
    Together (F + P) u sum_f |force_f| E[t - f] to first order; the + 1 and the factor 2 cover the (1 + u)^k cross
    terms and the fp64 interior (exp, sin and the running sums: a few 2^-53, times 2 pi for the phase)."""
    F = np.shape(force)[-1]
    return 2.0 * (F + partials + 1) * U32 * fir(E, np.abs(_f64(force)))


def bound_gs(gy, force):
    """|gs - ref|[a, t] <= 2 (F + 1) u sum_f |force[a, f]| |gy[a, t + f]|: at most F sequential fp32 fmas of exact fp32
    inputs (gamma_F ~ F u on the sum of absolute terms); + 1 and the factor 2 as in ``bound_y``."""
    F = np.shape(force)[-1]
    return 2.0 * (F + 1) * U32 * corr(np.abs(_f64(gy)), np.abs(_f64(force)))


def _bound_suffix(ref, scale, S, sr):
    return 2.0 * U32 * np.abs(ref) + S * 2.0 ** -48 * scale[..., None] / float(sr)


def bound_g_dmp(ref, U, S, sr):
    """|g_dmp - ref|[a, m, t] <= 2 u |ref| + S 2^-48 U[a, m] / sr, the reference being fed the device's own gs.

    osc_tv_bwd_kernel works in fp64 and rounds once, at the store: u |ref| (2 u with the cross term).  Before that,
    g_dmp[t] = (total - exclusive prefix) / sr, where total and prefix are fp64 sums of up to S terms gD_t with
    sum_t |gD_t| <= U: each sum carries at most ~S 2^-53 U of summation error (far less for the scans' tree order), the
    terms themselves a few 2^-53 |u_t| from exp, sin and D, P (whose running sums are kept small by the floor of the
    carry), and the subtraction cancels nothing that is not already counted against U.  That is ~S 2^-52 U / sr for the two
    sums; 2^-48 leaves a 16x margin."""
    return _bound_suffix(ref, U, S, sr)


def bound_g_frq(ref, U, S, sr):
    """As ``bound_g_dmp`` with 2 pi U: gP_t = 2 pi u_t cos(2 pi P_t), so sum_t |gP_t| <= 2 pi U."""
    return _bound_suffix(ref, TWO_PI * U, S, sr)


def bound_gamp(ref, V, S):
    """|gamp - ref|[a, m] <= 2 u |ref| + S 2^-48 V[a, m], V = sum_t |gs e^{-D}| (e^{-d tau} for the closed form): one fp64
    sum of S terms (~S 2^-53 V, terms a few 2^-53 each; 16x margin) and the fp32 store."""
    return 2.0 * U32 * np.abs(ref) + S * 2.0 ** -48 * V


def bound_gd_gw(W, S):
    """|gd - ref|[m], |gw - ref|[m] <= (ceil(S / 64) + 64) 2^-46 W[m], W = sum_{a,t} |amp gs tau e^{-d tau}|.

    osc_bwd_mode_kernel is fp64 throughout and stores fp64.  A lane seeds the phasor z = e^{(-d + i w) tau} from
    exp / sincos (a few 2^-53, plus the rounding of the argument w tau) and advances it ceil(S / 64) times by one complex
    multiply, ~3 2^-53 |z| each, so the last sample of a lane is off by ~3 ceil(S / 64) 2^-53 |z|; tau is advanced by
    repeated addition, another ceil(S / 64) 2^-53.  The products and the lane-local sums add ~ceil(S / 64) 2^-53, the
    wave reduction and the loop over clips a few more.  ~4 (ceil(S / 64) + 4) 2^-53 W in all; 2^-46 per step and the
    constant 64 leave about a 16x margin."""
    return (-(-S // 64) + 64) * 2.0 ** -46 * W


# -------------------------------------------------------------------------------- CPU model of the fp32 roundings
def round_like_kernel(mode_signals, groups, force):
    """The forward kernels' fp32 recipe applied to fp64 mode signals (A, m, S): the modes of each index set in ``groups``
    are summed in fp64 and rounded to fp32 once (one partial), the partials are added in order in fp32, and the FIR runs
    as F sequential fused multiply-adds, acc = fl32(force[f] * s[t - f] + acc).  (The product of two fp32 numbers is exact
    in fp64; the fp64 sum rounded to fp32 equals fmaf except for rare double roundings of one fp32 ulp.)  Returns
    fp32 (A, S)."""
    x = _f64(mode_signals)
    A, _, S = x.shape
    s = np.zeros((A, S), dtype=np.float32)
    for g in groups:
        s = (s + x[:, g, :].sum(1).astype(np.float32)).astype(np.float32)
    force = np.asarray(force, dtype=np.float32)
    acc = np.zeros((A, S), dtype=np.float32)
    for f in range(min(force.shape[1], S)):
        acc[:, f:] = (force[:, f:f + 1].astype(np.float64) * s[:, :S - f].astype(np.float64)
                      + acc[:, f:].astype(np.float64)).astype(np.float32)
    return acc


def tv_groups(m):
    return [np.arange(g, min(g + TV_MODES_PER_GROUP, m)) for g in range(0, m, TV_MODES_PER_GROUP)]


def bank_groups(m):
    return [np.arange(w, m, BANK_PARTIALS) for w in range(BANK_PARTIALS)]


# ------------------------------------------------------------------------------------------- torch fp64 chains
def _torch_fir(s, force):
    import torch

    A, F = force.shape
    w = torch.flip(force.reshape(A, 1, F), [-1]).to(s.dtype)
    return torch.nn.functional.conv1d(s.unsqueeze(0), w, groups=A, padding=F - 1).squeeze(0)[:, :s.shape[-1]]


def torch_tv_chain(dmp, frq, amp, force, sr):
    """The time-varying bank as the chain of torch ops the reference model uses (cumsum, exp, sin, mode sum, grouped
    conv1d) at the inputs' dtype; autograd-capable.  amp (A, m) or None."""
    import torch

    D = torch.cumsum(dmp / sr, dim=2)
    P = torch.cumsum(frq / sr, dim=2)
    sig = torch.exp(-D) * torch.sin(2 * np.pi * P)
    if amp is not None:
        sig = amp[:, :, None] * sig
    return _torch_fir(sig.sum(1), force)


def torch_bank_chain(d, w, amp, force, S, sr):
    """The closed-form bank in torch at d's dtype; autograd-capable.  amp (A, m) or None."""
    import torch

    tau = (torch.arange(S, dtype=d.dtype) + 1) / sr
    modes = torch.exp(-d[:, None] * tau[None]) * torch.sin(w[:, None] * tau[None])
    A = force.shape[0]
    s = modes.sum(0, keepdim=True).expand(A, S) if amp is None else amp @ modes
    return _torch_fir(s.contiguous(), force)


# ------------------------------------------------------------------------------------------- shapes and inputs
SR = 32000.0
# (A, m, F, S) of the time-varying pair: smallest; partial wave and chunk; one full chunk; carry into a one-sample chunk;
# one full workgroup of modes; a second group with one mode and the FIR tile boundary; idle waves and an exact tile;
# the longest force and three groups
TV_SHAPES = [(1, 1, 1, 1), (1, 3, 2, 63), (2, 4, 1, 64), (1, 5, 7, 65), (3, 16, 150, 128), (2, 17, 150, 1025),
             (1, 24, 150, 1024), (1, 33, 512, 2500)]
TV_VARIANTS = ["noamp", "negfrq", "negdmp", "nyquist"]  # run on the 65- and the 1025-sample shapes
BANK_SHAPES = [(1, 1, 1, 1), (2, 3, 2, 63), (1, 4, 512, 1024), (2, 7, 512, 1025), (1, 5, 150, 2049), (3, 64, 150, 2500)]


def tv_inputs(shape, variant="base"):
    """fp32 (dmp, frq (A, m, S), amp (A, m) or None, force (A, F), gy (A, S)): frq 50..15000 Hz and dmp 1..400 1/s with
    per-sample jitter, amp 0.5..1.5, force and gy standard normal; fixed seed per (shape, variant)."""
    A, m, F, S = shape
    rng = np.random.default_rng([A, m, F, S, sum(map(ord, variant))])
    f0 = rng.uniform(60.0, 14000.0, (A, m, 1))
    d0 = rng.uniform(1.2, 360.0, (A, m, 1))
    frq = (f0 * (1.0 + 0.05 * rng.uniform(-1, 1, (A, m, S)))).astype(np.float32)
    dmp = (d0 * (1.0 + 0.1 * rng.uniform(-1, 1, (A, m, S)))).astype(np.float32)
    amp = rng.uniform(0.5, 1.5, (A, m)).astype(np.float32)
    force = rng.standard_normal((A, F)).astype(np.float32)
    gy = rng.standard_normal((A, S)).astype(np.float32)
    lo, hi = S // 4, max(S // 2, S // 4 + 1)
    if variant == "noamp":
        amp = None
    elif variant == "negfrq":  # one mode runs backwards throughout, every mode over a block of samples
        frq[:, 0, :] *= -1
        frq[:, :, lo:hi] *= -1
    elif variant == "negdmp":  # the envelope grows over a block
        dmp[:, :, lo:hi] = np.float32(-5.0) * (1 + rng.uniform(0, 1, (A, m, hi - lo))).astype(np.float32)
    elif variant == "nyquist":
        frq[:] = np.float32(0.49 * SR)
    elif variant == "const":  # one value per mode: the closed-form bank at d = dmp, w = 2 pi frq computes the same signal
        frq[:] = frq[:1, :, :1]
        dmp[:] = dmp[:1, :, :1]
    elif variant != "base":
        raise ValueError(variant)
    return dmp, frq, amp, force, gy


def bank_inputs(shape, with_amp=True):
    """(d, w (m,) fp64, amp (A, m) fp32 or None, force (A, F), gy (A, S) fp32): f 50..15000 Hz, d 1..400 1/s."""
    A, m, F, S = shape
    rng = np.random.default_rng([A, m, F, S, int(with_amp), 7])
    w = TWO_PI * np.sort(rng.uniform(50.0, 15000.0, m))
    d = rng.uniform(1.0, 400.0, m)
    amp = rng.uniform(0.5, 1.5, (A, m)).astype(np.float32) if with_amp else None
    return d, w, amp, rng.standard_normal((A, F)).astype(np.float32), rng.standard_normal((A, S)).astype(np.float32)
