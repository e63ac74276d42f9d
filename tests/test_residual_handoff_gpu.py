"""The residual walk that hands the bf16 two-level cycle its inputs (ds_union_residual_pre, epilogue 6 of the neighbour-union
kernel) against the two launches it replaces - ds_union_residual, then the cycle's ds_cheb_init16 on the fp32 residual - and
the cycle / the native iteration started from those inputs against the ones that start from the fp32 block.  The fused form
applies the same helper to the same fp32 values, so every comparison here is for EQUALITY, bit for bit."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

RHO, LAM, MU = 2700.0, 2e10, 3e10
NCOLS = [4, 36, 80, 84]  # the generic lanes-per-node form below and above one wave's width of columns, lpn == 20, the widest
# 343 ord-2 nodes (85 groups of 4 and a ragged one of 3), 216 ord-1 nodes (whole groups only), 27 ord-1 nodes (7 groups, ragged)
MESHES = [(3, 2), (5, 1), (2, 1)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _ops(mesh, order, two_level):
    from diffsound_amd import meshgen
    from diffsound_amd.diffelastic.mesh import TetMesh
    from diffsound_amd.modal_ops import HipModalOps, TetSystem

    dev = torch.device("cuda:0")
    v, t = meshgen.kuhn_box(mesh)
    tm = TetMesh(torch.from_numpy(v).to(dev), torch.from_numpy(t).long().to(dev)).to_high_order(order)
    return HipModalOps(TetSystem(tm.vertices, tm.tets, order, RHO), LAM, MU, two_level=two_level)


def _bits(t):
    return t.view(torch.int16)


def _operands(ops, ncols, seed):
    """X as a column range of a wider buffer (as the solver passes it) and Ritz values of the size of K's spectrum."""
    dev = ops.device
    g = torch.Generator(device=dev).manual_seed(seed)
    big = torch.full((ops.n, 104), float("nan"), device=dev)
    X = big[:, 8:8 + ncols]
    X.copy_(torch.randn((ops.n, ncols), generator=g, device=dev))
    lam = (torch.rand(ncols, generator=g, device=dev, dtype=torch.float64) + 0.5) * 1e9
    return X, lam


def _bf16_range(n, ncols, dev):
    """A bf16 block as a column range (8 bytes in) of a wider buffer of NaNs, and that buffer."""
    wide = torch.full((n, ncols + 8), float("nan"), device=dev, dtype=torch.bfloat16)
    return wide[:, 4:4 + ncols], wide


@pytest.mark.parametrize("ncols", NCOLS)
@pytest.mark.parametrize("mesh,order", MESHES)
def test_residual_with_cycle_inputs_equals_the_two_launches_bit_for_bit(dev, mesh, order, ncols):
    """R16, W1 and the norms of ds_union_residual_pre == ds_union_residual followed by ds_cheb_init16(..., rinit_f32 = 1)."""
    from diffsound_amd import _hip

    ops = _ops(mesh, order, False)
    assert ops.nv % 4 == (0 if (mesh, order) == (5, 1) else 3)
    X, lam = _operands(ops, ncols, 1000 * mesh + ncols)
    c = 0.37e-9
    # the two launches
    R = torch.empty((ops.n, ncols), device=dev)
    rn0, xn0 = ops.residual_fused(X, lam, R)
    R16a, W1a = (torch.empty((ops.n, ncols), device=dev, dtype=torch.bfloat16) for _ in range(2))
    p = _hip.ptr
    _hip.check(_hip.lib().ds_cheb_init16(p(R), 1, R.stride(0), p(W1a), ncols, p(R16a), ncols, p(ops.dinv), ops.nv, ncols, c,
                                         _hip.stream_ptr()), "ds_cheb_init16")
    # one launch, into column ranges of wider buffers
    (R16b, wide_r), (W1b, wide_w) = _bf16_range(ops.n, ncols, dev), _bf16_range(ops.n, ncols, dev)
    rn1, xn1 = ops.residual_fused_pre(X, lam, c, R16b, W1b)
    for wide in (wide_r, wide_w):
        assert bool(torch.isnan(wide[:, :4]).all()) and bool(torch.isnan(wide[:, 4 + ncols:]).all())
    assert bool(torch.isfinite(W1a.float()).all()) and float(W1a.float().abs().max()) > 0
    assert torch.equal(_bits(R16b), _bits(R16a))
    assert torch.equal(_bits(W1b), _bits(W1a))
    assert torch.equal(rn1, rn0) and torch.equal(xn1, xn0)


def test_residual_with_cycle_inputs_refuses_bad_arguments(dev):
    from diffsound_amd import _hip

    ops = _ops(3, 2, False)
    X, lam = _operands(ops, 36, 7)
    (R16, _), (W1, _) = _bf16_range(ops.n, 36, dev), _bf16_range(ops.n, 36, dev)
    L, p = _hip.lib(), _hip.ptr
    ws = ops._residual_ws(36)

    def call(tag=0, r16=R16, w1=W1, ncols=36, wsb=None, dinv=ops.dinv):
        return L.ds_union_residual_pre(tag, *ops._union_tabs(), p(ops.kgrp), p(ops.mgrp), ops.kgrp.shape[0], ops.nv, p(X), X.stride(0),
                                       p(lam), p(dinv), 1e-9, p(r16), r16.stride(0), p(w1), w1.stride(0), ncols, p(ws),
                                       ws.numel() if wsb is None else wsb, p(ops._nrm[0]), p(ops._nrm[1]), _hip.stream_ptr())

    assert call() == 0
    for bad in (dict(tag=1), dict(w1=R16), dict(ncols=88), dict(ncols=34), dict(wsb=8), dict(r16=R16[:, 1:]), dict(w1=W1[:, 2:]),
                dict(dinv=None)):
        assert call(**bad) != 0, bad
        assert L.ds_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("ncols,degree,skip", [(4, 3, 0), (36, 3, 0), (80, 3, 0), (84, 3, 0), (80, 1, 0), (36, 3, 4), (80, 3, 8), (84, 2, 4)])
def test_cycle_from_prepared_inputs_equals_the_cycle_from_the_residual_bit_for_bit(dev, ncols, degree, skip):
    """ds_twolevel_apply (bf16 storage) with DS_TL_PREPARED on what ds_union_residual_pre wrote == the unprepared call on the fp32
    R of ds_union_residual: W bit for bit.  ``skip`` > 0: the leading columns have been locked in between - the cycle runs on the
    blocks from that column on, as ds_lobpcg_iterate passes them - against the unprepared call on the same columns of R."""
    ops = _ops(3, 2, True)
    assert ops.coarse is not None
    X, lam = _operands(ops, ncols, 50 + ncols + degree)
    smooth, coarse = (degree, 2.0, 0.2), (5, 3.0, 0.01)
    c = 1.0 / (0.5 * (smooth[1] + smooth[2]))
    na = ncols - skip
    bf = lambda n, cols=ncols: torch.full((n, cols), float("nan"), device=dev, dtype=torch.bfloat16)

    def cycle(prepared):
        D, AD, Rr, Wc, R16 = (bf(ops.n) for _ in range(5))
        Rc, Ec, Dc, ADc = (bf(ops.coarse.n) for _ in range(4))
        W = torch.full((ops.n, na + 8), float("nan"), device=dev)
        R = torch.full((ops.n, ncols), float("nan"), device=dev)
        if prepared:
            ops.residual_fused_pre(X, lam, c, R16, D if degree >= 2 else Wc)
        else:
            ops.residual_fused(X, lam, R)
        cut = lambda t: t[:, skip:]
        assert ops.twolevel_apply(smooth, coarse, cut(R), W[:, 4:4 + na], cut(D), cut(AD), cut(Rr), cut(Rc), cut(Ec), cut(Dc), cut(ADc),
                                  cut(Wc), R16=cut(R16), prepared=prepared)
        assert bool(torch.isnan(W[:, :4]).all()) and bool(torch.isnan(W[:, 4 + na:]).all())
        return W[:, 4:4 + na]

    Wa, Wb = cycle(False), cycle(True)
    assert bool(torch.isfinite(Wa).all()) and float(Wa.abs().max()) > 0
    assert torch.equal(Wb, Wa)


def _resid_widths(ops, run):
    """The widths of the fine level's residual walks while ``run()`` runs: the active block of every iteration, i.e. the locking
    sequence (the library's launch records, ds_profile_stream)."""
    from diffsound_amd import _hip

    L, cap = _hip.lib(), 4096
    stream = torch.cuda.Stream(device=ops.device)  # (the records are kept for a registered stream, which the null stream cannot be)
    torch.cuda.synchronize()
    _hip.check(L.ds_profile_kinds(1 << 3), "ds_profile_kinds")  # DS_PROF_RESID
    _hip.check(L.ds_profile_stream(stream.cuda_stream, cap), "ds_profile_stream")
    try:
        with torch.cuda.stream(stream):
            out = run()
        torch.cuda.synchronize()
    finally:
        ms, a_, b_ = (ctypes.c_float * cap)(), (ctypes.c_int64 * cap)(), (ctypes.c_int64 * cap)()
        c_, f_ = (ctypes.c_int32 * cap)(), (ctypes.c_int32 * cap)()
        n = int(L.ds_profile_collect(ms, a_, b_, c_, f_, cap))
        _hip.check(L.ds_profile_kinds(0), "ds_profile_kinds")
    assert 0 <= n < cap
    return out, [int(c_[i]) for i in range(n) if int(a_[i]) == ops.nv and (int(f_[i]) >> 16) == 3]


@pytest.mark.parametrize("mesh,k,block", [(6, 32, 40), (8, 16, 24)])
def test_native_iteration_with_the_handoff_equals_the_two_launches(dev, mesh, k, block):
    """ds_lobpcg_iterate with the residual walk handing the cycle its inputs against the same solve with the hand-off switched off
    (SolverConfig.residual_handoff): the same iterates, so the same iteration counts, the same locking sequence (the widths of the
    residual walks), the same error history and eigenvalues, all bit for bit.  Columns are locked in the middle of both solves:
    the cycle then starts on the prepared blocks from the first active column on."""
    import bench
    from diffsound_amd import meshgen
    from diffsound_amd.lobpcg.modal_solver import ModalSolver
    from diffsound_amd.modal_ops import HipModalOps, TetSystem
    from oracle import fem

    v, t = meshgen.kuhn_box(mesh)
    v, t = fem.to_high_order(torch.from_numpy(v), torch.from_numpy(t).long(), 2)
    sysd = TetSystem(v.to(dev), t.to(dev), 2, RHO)
    lam, mu = fem.lame(5e10, 0.25)
    res, widths, untouched = {}, {}, {}
    for handoff in (True, False):
        ops = HipModalOps(sysd, lam, mu)  # fresh operators: no state carried from one solve to the other
        cfg = bench.solver_config(block=block, order=2)
        cfg.residual_handoff = handoff
        assert cfg.native and cfg.fused_residual and cfg.kx_fresh and cfg.lock and cfg.precond_storage == "bf16"
        seen = []
        orig = ops.native_lobpcg

        def spy(*a, _o=orig, _seen=seen, **kw):
            R = a[9]  # the fp32 residual block: the hand-off never writes it
            R.fill_(float("nan"))
            out = _o(*a, **kw)
            _seen.append(bool(torch.isnan(R).all()))
            return out

        ops.native_lobpcg = spy
        try:
            res[handoff], widths[handoff] = _resid_widths(ops, lambda: ModalSolver(ops, cfg).solve(k))
        finally:
            del ops.native_lobpcg
        untouched[handoff] = seen
    a, b = res[True], res[False]
    # the route under test really ran, and only when asked
    assert untouched[True] and all(untouched[True]) and untouched[False] and not any(untouched[False])
    assert float(a.rerr.max()) < cfg.tol and a.iterations < cfg.maxit
    assert a.iterations == b.iterations and a.coarse_iterations == b.coarse_iterations
    assert widths[True] == widths[False]
    w = widths[True]
    assert len(w) > a.iterations and w[0] == block
    assert min(w[:-1]) < block, w  # columns were locked before the last iteration: a cycle ran on offset blocks
    assert a.history == b.history
    assert torch.equal(a.rerr, b.rerr)
    assert torch.equal(a.eigenvalues, b.eigenvalues)
