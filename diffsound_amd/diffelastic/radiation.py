"""Radiated sound at a listener: each mode's exterior field as a multipole series about the object's centre
(ds_multipole_fwd / ds_multipole_bwd, csrc/multipole.hip).

``bem.modal_transfer`` solves one dense boundary-element problem per mode for every new set of listener points and returns
numpy.  Here the solve happens once per mode (``ModalRadiator``): the field is sampled on a sphere around the object and a
series of outgoing waves  sum_{l <= L, |n| <= l} c[l^2 + l + n] h_l(k r) Y_{l,n}  is fitted to the samples
(``fit_multipoles``); after that a listener costs (L + 1)^2 multiply-adds per mode (``multipole_eval``) and the result is
differentiable in the listener's position.  ``ModalRadiator.gains`` is the listener's half of the oscillator modules'
``mode_gain``; ``ContactSurface.amplitudes_at`` is the striker's half.

Convention e^{-i w t}, G = e^{ikr} / (4 pi r), as in ``bem``; Y_{l,n} the real orthonormal spherical harmonics (n > 0:
sqrt2 (-1)^n Re Y_l^n, n < 0: sqrt2 (-1)^n Im Y_l^|n|, Y_l^n with the Condon-Shortley phase).  Everything is fp64 / complex128.
"""
import math
import warnings

import torch

from .. import _hip
from . import bem

MAX_ORDER = 32          # DS_MULTIPOLE_MAX_ORDER
MAX_MODES = 512         # DS_MULTIPOLE_MAX_MODES
MAX_POINTS = 1 << 24    # DS_MULTIPOLE_MAX_POINTS
RESIDUAL_WARN = 1e-2    # a fit residual above this warns


def _check(points, center, k, coef, order):
    """Every refusal that needs no launch, shapes first: ValueError.  The checks of values are one flag each, read in one
    transfer."""
    for name, t in (("points", points), ("center", center), ("k", k)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError(f"multipole_eval: {name} must be a floating-point tensor")
    if not isinstance(coef, torch.Tensor) or not coef.is_complex():
        raise ValueError("multipole_eval: coef must be a complex tensor")
    if not isinstance(order, int) or not 0 <= order <= MAX_ORDER:
        raise ValueError(f"multipole_eval: order = {order!r} outside 0..{MAX_ORDER}")
    if points.dim() != 2 or points.shape[1] != 3 or not 1 <= points.shape[0] <= MAX_POINTS:
        raise ValueError(f"multipole_eval: points must be (P, 3) with 1 <= P <= {MAX_POINTS}, got {tuple(points.shape)}")
    if center.shape != (3,):
        raise ValueError(f"multipole_eval: center must be (3,), got {tuple(center.shape)}")
    if k.dim() != 1 or not 1 <= k.shape[0] <= MAX_MODES:
        raise ValueError(f"multipole_eval: k must be (m,) with 1 <= m <= {MAX_MODES}, got {tuple(k.shape)}")
    n = (order + 1) ** 2
    if coef.shape != (k.shape[0], n):
        raise ValueError(f"multipole_eval: coef must be ({k.shape[0]}, {n}) = (m, (order + 1)^2), got {tuple(coef.shape)}")
    dev = points.device
    c = center.detach().to(dev)
    flags = [torch.isfinite(points.detach()).all(), torch.isfinite(c).all(), torch.isfinite(k.detach()).all(),
             torch.isfinite(torch.view_as_real(coef.detach())).all(), (k.detach() > 0).all(),
             ((points.detach() - c) != 0).any(dim=1).all()]
    flags = torch.stack([f.to(dev) for f in flags]).tolist()
    for name, ok in zip(("points", "center", "k", "coef"), flags):
        if not ok:
            raise ValueError(f"multipole_eval: {name} is not finite")
    if not flags[4]:
        raise ValueError("multipole_eval: k must be positive (wave numbers)")
    if not flags[5]:
        raise ValueError("multipole_eval: a point lies at the center (the series is singular there)")


class _Multipole(torch.autograd.Function):
    """out (P, m, 2) from points (P, 3) and coef (m, N, 2), real views throughout; gradients for both, each computed only
    where it is needed.  The kernels take the coefficients as (N, m): the transposes are made here."""

    @staticmethod
    def forward(ctx, points, coef2, center, k, order):
        pts = points.detach().to(torch.float64).contiguous()
        cf = coef2.detach().to(torch.float64).transpose(0, 1).contiguous()  # (N, m, 2)
        P, m = pts.shape[0], k.shape[0]
        out = torch.empty((P, m, 2), dtype=torch.float64, device=pts.device)
        p = _hip.ptr
        _hip.launch("ds_multipole_fwd", p(pts), p(center), p(k), p(cf), P, m, order, p(out), device=pts.device)
        ctx.save_for_backward(pts, cf, center, k)
        ctx.order = order
        ctx.dtypes = (points.dtype, coef2.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        pts, cf, center, k = ctx.saved_tensors
        P, m, L = pts.shape[0], k.shape[0], ctx.order
        need_p, need_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_p or need_c):
            return None, None, None, None, None
        gout = gout.to(torch.float64).contiguous()
        gpts = torch.empty_like(pts) if need_p else None
        gcf = torch.empty_like(cf) if need_c else None
        work, nbytes = _hip.workspace("ds_multipole_workspace_bytes", P, m, L, device=pts.device) if need_c else (None, 0)
        p = _hip.ptr
        _hip.launch("ds_multipole_bwd", p(gout), p(pts), p(center), p(k), p(cf), P, m, L, p(work), nbytes, p(gpts), p(gcf),
                    device=pts.device)
        return (gpts.to(ctx.dtypes[0]) if need_p else None,
                gcf.transpose(0, 1).to(ctx.dtypes[1]) if need_c else None, None, None, None)


def multipole_eval(points, center, k, coef, order):
    """The series at ``points`` (P, 3) for every mode: (P, m) complex128,
        out[p, j] = sum_{l <= order} sum_{|n| <= l} coef[j, l^2 + l + n] h_l(k[j] r) Y_{l,n}((x_p - center) / r),  r = |x_p - center|.
    center (3,), k (m,) > 0, coef (m, (order + 1)^2) complex.  Autograd reaches ``points`` and ``coef`` (not ``k`` or
    ``center``).  HIP tensors only: there is no CPU path.  ValueError before any launch: wrong shapes, a non-finite input,
    k <= 0, a point at the centre, order outside 0..32, m above 512."""
    _check(points, center, k, coef, order)
    _hip.require_gpu(points, center, k, coef)
    dev = points.device
    center = center.detach().to(dev, torch.float64).contiguous()
    k = k.detach().to(dev, torch.float64).contiguous()
    coef2 = torch.view_as_real(coef.to(torch.complex128))
    return torch.view_as_complex(_Multipole.apply(points, coef2, center, k, order))


def _basis(points, center, kj, order):
    """(Q, N) complex128 h_l(kj r) Y_{l,n}: the forward on unit coefficients, every term as a column of its own (in slices
    of at most 512 columns)."""
    n = (order + 1) ** 2
    cols = []
    for a in range(0, n, MAX_MODES):
        b = min(n, a + MAX_MODES)
        unit = torch.zeros((b - a, n), dtype=torch.complex128, device=points.device)
        unit[torch.arange(b - a), torch.arange(a, b)] = 1.0
        cols.append(multipole_eval(points, center, kj.expand(b - a), unit, order))
    return torch.cat(cols, 1)


def fit_multipoles(points, values, k, center, order):
    """Least-squares coefficients of the series from field samples: ``values`` (Q, m) complex at ``points`` (Q, 3), one
    column per mode of wave number ``k[j]``.  Returns (coef (m, N) complex128, residual (m,) fp64: |B c - v| / |v| per mode).
    Needs Q >= 2 N samples, N = (order + 1)^2.  The columns of the basis h_l(k r) Y_{l,n} differ by many orders of magnitude
    (|h_l| grows like (l / k r)^l): each is scaled to unit norm before the solve and the solution scaled back.  The basis
    comes from the forward kernel on unit coefficients; the solve is LAPACK's gelsd in complex128 on the host (gelsy, with a
    warning, where gelsd's SVD does not converge)."""
    if not isinstance(order, int) or not 0 <= order <= MAX_ORDER:
        raise ValueError(f"fit_multipoles: order = {order!r} outside 0..{MAX_ORDER}")
    n = (order + 1) ** 2
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("fit_multipoles: points must be a (Q, 3) tensor")
    Q = points.shape[0]
    if Q < 2 * n:
        raise ValueError(f"fit_multipoles: {Q} samples, at least 2 (order + 1)^2 = {2 * n} needed")
    if not isinstance(k, torch.Tensor) or k.dim() != 1 or k.shape[0] < 1:
        raise ValueError("fit_multipoles: k must be an (m,) tensor")
    if not isinstance(values, torch.Tensor) or not values.is_complex() or values.shape != (Q, k.shape[0]):
        raise ValueError(f"fit_multipoles: values must be complex ({Q}, {k.shape[0]})")
    if not bool(torch.isfinite(torch.view_as_real(values)).all()):
        raise ValueError("fit_multipoles: values is not finite")
    values = values.detach().to(torch.complex128)
    k = k.detach().to(points.device, torch.float64)
    coef = torch.empty((k.shape[0], n), dtype=torch.complex128, device=points.device)
    res = torch.empty(k.shape[0], dtype=torch.float64, device=points.device)
    with torch.no_grad():
        for j in range(k.shape[0]):
            B = _basis(points.detach(), center, k[j:j + 1], order)
            s = torch.linalg.vector_norm(B, dim=0)
            v = values[:, j]
            Bs = (B / s).cpu()
            if not bool(torch.isfinite(torch.view_as_real(Bs)).all()):
                raise ValueError(f"fit_multipoles: the basis of mode {j} (k = {float(k[j]):g}) is not finite at order {order}: "
                                 "k r is too small for h_l at this order")
            try:
                c = torch.linalg.lstsq(Bs, v.cpu().unsqueeze(1), driver="gelsd").solution[:, 0]
            except torch.linalg.LinAlgError as ex:  # gelsd's divide-and-conquer SVD can fail to converge: say so, pivoted QR
                warnings.warn(f"fit_multipoles: gelsd failed for mode {j} ({ex}); solving with gelsy", RuntimeWarning)
                c = torch.linalg.lstsq(Bs, v.cpu().unsqueeze(1), driver="gelsy").solution[:, 0]
            c = c.to(points.device) / s
            coef[j] = c
            vn = torch.linalg.vector_norm(v)
            res[j] = torch.linalg.vector_norm(B @ c - v) / torch.where(vn > 0, vn, torch.ones_like(vn))
    return coef, res


def fibonacci_sphere(n, radius, center):
    """n points of the Fibonacci lattice on the sphere of ``radius`` around ``center`` (3,): (n, 3) on center's device."""
    i = torch.arange(n, dtype=torch.float64, device=center.device) + 0.5
    z = 1.0 - 2.0 * i / n
    ph = i * (math.pi * (3.0 - math.sqrt(5.0)))
    rho = torch.sqrt(1.0 - z * z)
    return center + radius * torch.stack([rho * torch.cos(ph), rho * torch.sin(ph), z], 1)


class ModalRadiator:
    """The exterior fields of the modes of a ``DiffSoundObj`` for unit modal amplitudes, as multipole series: one
    boundary-element solve per mode, once (per mode k = omega / c, Neumann data rho omega^2 u_n, as ``bem.modal_transfer``).

    The surface is ``bem.surface_of(obj.tetmesh)``; ``center`` is the centre of its bounding box and ``radius`` (a) the
    distance of its farthest vertex, a bounding sphere.  Each mode's field is sampled at ``samples`` points (default
    4 (order + 1)^2) of a Fibonacci lattice on the sphere of radius ``fit_radius`` a and fitted at ``order``
    (None: min(32, ceil(k_max a) + 6)).  A mode whose fit residual exceeds 1e-2, or whose GMRES did not converge - k near an
    interior Dirichlet eigenfrequency, where the direct formulation is singular -, warns with the mode's index.

    Attributes: ``center`` (3,), ``radius``, ``k`` (m,), ``coef`` (m, N) complex128, ``fit_residual`` (m,), ``gmres_info``
    (list of dicts), ``order``.  There is no gradient to the object: the coefficients are constants."""

    def __init__(self, obj, order=None, c=343.0, rho=1.225, fit_radius=1.5, samples=None):
        if getattr(obj, "U_hat", None) is None:
            obj.eigen_decomposition()
        if not fit_radius > 1.0:
            raise ValueError(f"ModalRadiator: fit_radius = {fit_radius} must be above 1 (the sample sphere encloses the object)")
        verts = obj.tetmesh.vertices.detach()
        dev = verts.device
        surf = bem.surface_of(obj.tetmesh)
        sv = verts.double()[torch.unique(surf[0])]
        self.center = 0.5 * (sv.min(0).values + sv.max(0).values)
        self.radius = float(torch.linalg.vector_norm(sv - self.center, dim=1).max())
        lam = obj.eigenvalues.detach().double().reshape(-1).to(dev)
        omega = torch.sqrt(lam.clamp(min=0.0))
        self.c = float(c)  # the speed of sound: ``listener_path`` turns distances into delays with it
        self.k = omega / c
        if not bool((self.k > 0).all()) or self.k.shape[0] > MAX_MODES:
            raise ValueError("ModalRadiator: every mode needs a positive eigenvalue (no rigid-body modes), at most "
                             f"{MAX_MODES} modes")
        kmax = float(self.k.max())
        if order is None:
            order = min(MAX_ORDER, math.ceil(kmax * self.radius) + 6)
        if not isinstance(order, int) or not 0 <= order <= MAX_ORDER:
            raise ValueError(f"ModalRadiator: order = {order!r} outside 0..{MAX_ORDER}")
        self.order = order
        n = (order + 1) ** 2
        samples = 4 * n if samples is None else int(samples)
        if samples < 2 * n:
            raise ValueError(f"ModalRadiator: samples = {samples}, at least 2 (order + 1)^2 = {2 * n} needed")
        self.sample_points = fibonacci_sphere(samples, fit_radius * self.radius, self.center)
        model = bem.BEMModel(verts, surf[0], device=dev)
        un = bem.mode_neumann(obj, surf)
        values = torch.empty((samples, self.k.shape[0]), dtype=torch.complex128, device=dev)
        self.gmres_info = []
        for j in range(self.k.shape[0]):
            kj, wj = float(self.k[j]), float(omega[j])
            g = model._to_internal(rho * wj ** 2 * un[:, j], "neumann_coeff")
            A, rhs, _ = model.assemble(kj, g)
            u, info = model._gmres(A, rhs)
            del A
            values[:, j] = model._potential(kj, g, u, self.sample_points).to(torch.complex128)
            self.gmres_info.append(info)
            if not info["converged"]:
                warnings.warn(f"ModalRadiator: GMRES did not converge for mode {j} (k = {kj:g}, relative residual "
                              f"{info['residual']:.2e}); k may be near an interior Dirichlet eigenfrequency of the object",
                              RuntimeWarning)
        self.sample_values = values
        self.coef, self.fit_residual = fit_multipoles(self.sample_points, values, self.k, self.center, order)
        for j, r in enumerate(self.fit_residual.tolist()):
            if not r <= RESIDUAL_WARN:
                warnings.warn(f"ModalRadiator: the fit of mode {j} at order {order} leaves a relative residual of {r:.2e} "
                              f"(above {RESIDUAL_WARN:g}): raise the order, or distrust the boundary-element solve", RuntimeWarning)

    def _outside(self, points):
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
            raise ValueError("ModalRadiator: points must be a (P, 3) tensor")
        _hip.require_gpu(points)
        d2 = ((points.detach().double() - self.center) ** 2).sum(1)
        if not bool((d2 >= self.radius ** 2).all()):  # (false for NaN as well)
            raise ValueError(f"ModalRadiator: a point lies inside the bounding sphere (radius {self.radius:g} around the "
                             "center) or is not finite: the series is not valid there")

    def transfer(self, points):
        """(P, m) complex128 pressure at ``points`` (P, 3) per unit modal amplitude; differentiable in ``points``."""
        self._outside(points)
        return multipole_eval(points, self.center, self.k, self.coef, self.order)

    def gains(self, points):
        """|transfer| (P, m) fp64: the listener's ``mode_gain``, to be multiplied with ``ContactSurface.amplitudes_at``."""
        return self.transfer(points).abs()

    def listener_gains(self, points):
        """conj(transfer(points)), (P, m) complex128: the oscillator modules' ``listener_gain`` (C = P channels, m modes)
        for listeners at rest; differentiable in ``points``.

        Why the conjugate.  With the package's e^{-i w t} convention a mode of unit amplitude a(t) = e^{-i w t} is heard at
        the point as T e^{-i w t}, T = transfer.  The banks keep the mode as the state x ~ e^{+i w t} (z = e^{(-d + i w) / sr})
        and the dry signal is Im x = sin(w t) = Re(i e^{-i w t}), the real part of the amplitude a = i e^{-i w t}.  The
        pressure is then Re(T i e^{-i w t}) = -Im(T e^{-i w t}) = Im(conj(T) e^{+i w t}) = Im(conj(T) x): the gain that
        multiplies the bank's state is conj(T).  (|T| alone, ``gains``, keeps the level and drops the phase.)"""
        return self.transfer(points).conj()

    def listener_path_gains(self, path):
        """The listener gains along a path: ``path`` (K, 3) - one listener - or (C, K, 3) - C listeners, e.g. two ears -,
        the positions at K control frames ``listener_hop`` samples apart.  Returns (C, m, K) complex128 =
        conj(transfer) at every frame, the oscillator modules' ``listener_gain`` with ``listener_hop``; differentiable in
        ``path``.

        This is the quasi-static reading of a moving listener: the gain multiplies the modal state sample by sample, and
        the propagation delay r / c enters only as the phase e^{i k r} of each mode at its own frequency (whose rotation
        along the path is the Doppler shift) - there is no fractional delay line, so the envelope of a mode is not
        delayed (``listener_path`` returns the delay beside a gain without the carrier, for the delay line).  The banks interpolate the gains linearly between frames; between two unit phasors an angle th apart the
        interpolant dips to cos(th / 2) (0.92 at pi / 4), so a RuntimeWarning names the largest phase step of any mode
        between two consecutive frames when it exceeds pi / 4: lower the hop (or slow the path down)."""
        if not isinstance(path, torch.Tensor) or path.dim() not in (2, 3) or path.shape[-1] != 3 or min(path.shape) < 1:
            raise ValueError("ModalRadiator: path must be a (K, 3) or (C, K, 3) tensor")
        p3 = path.unsqueeze(0) if path.dim() == 2 else path
        C, K = p3.shape[0], p3.shape[1]
        T = self.transfer(p3.reshape(C * K, 3)).reshape(C, K, -1).permute(0, 2, 1)  # (C, m, K)
        if K > 1:
            Td = T.detach()
            step = torch.angle(Td[:, :, 1:] * Td[:, :, :-1].conj()).abs()
            worst = float(step.max())
            if worst > math.pi / 4:
                warnings.warn(f"ModalRadiator.listener_path_gains: a mode's phase turns by {worst:.3g} rad between two "
                              f"consecutive frames (above pi / 4 = {math.pi / 4:.3g}): the linear interpolation between "
                              "frames loses level there - lower hop, the samples between two frames", RuntimeWarning)
        return T.conj()

    def listener_path(self, path, sr):
        """A moving listener as a gain AND a propagation delay: ``path`` (K, 3) or (C, K, 3) as in ``listener_path_gains``,
        ``sr`` the sample rate.  Returns (gain (C, m, K) complex128, delay (C, K) fp64 in samples), the oscillator modules'
        ``listener_gain`` and ``listener_delay`` at one ``listener_hop``:

            delay = sr r / c,  r = |x - center| (formed in torch),     gain = conj(transfer e^{-i k r}).

        The carrier e^{i k r} of each mode is taken out of the gain and the distance goes into the delay line
        (``ddsp.delay.propagate``) instead, which delays the envelope and the onset as well as the phase: gain and delay
        together carry what ``listener_path_gains`` put into the phase alone.  Both are differentiable in ``path``.  ``c`` is
        the speed of sound the radiator was built with (``self.c``).

        What is left in the gain - 1 / r, the directivity, the near-field terms of the series - varies slowly along a path,
        so the pi / 4 phase-step RuntimeWarning of ``listener_path_gains``, applied here to the stripped gain, fires far
        later: a hop that turns the full gain by many radians is correct here as long as the delay's own bound holds (a
        step of at most hop / 2 samples between two frames, a listener below Mach 0.5)."""
        if not isinstance(path, torch.Tensor) or path.dim() not in (2, 3) or path.shape[-1] != 3 or min(path.shape) < 1:
            raise ValueError("ModalRadiator: path must be a (K, 3) or (C, K, 3) tensor")
        if not sr > 0:
            raise ValueError(f"ModalRadiator.listener_path: sr = {sr!r} is not positive")
        p3 = path.unsqueeze(0) if path.dim() == 2 else path
        C, K = p3.shape[0], p3.shape[1]
        T = self.transfer(p3.reshape(C * K, 3)).reshape(C, K, -1).permute(0, 2, 1)  # (C, m, K)
        r = torch.linalg.vector_norm(p3.double() - self.center, dim=-1)             # (C, K)
        kr = self.k[None, :, None] * r[:, None, :]
        stripped = T * torch.complex(torch.cos(kr), -torch.sin(kr))
        if K > 1:
            Td = stripped.detach()
            worst = float(torch.angle(Td[:, :, 1:] * Td[:, :, :-1].conj()).abs().max())
            if worst > math.pi / 4:
                warnings.warn(f"ModalRadiator.listener_path: with the carrier removed a mode's gain still turns by {worst:.3g} rad "
                              f"between two consecutive frames (above pi / 4 = {math.pi / 4:.3g}): the linear interpolation "
                              "between frames loses level there - lower hop, the samples between two frames", RuntimeWarning)
        return stripped.conj(), (float(sr) / self.c) * r

    def field(self, points, chunk=65536):
        """``transfer`` without autograd, ``chunk`` points at a time: for maps."""
        self._outside(points)
        with torch.no_grad():
            return torch.cat([multipole_eval(points[a:a + chunk], self.center, self.k, self.coef, self.order)
                              for a in range(0, points.shape[0], chunk)])
