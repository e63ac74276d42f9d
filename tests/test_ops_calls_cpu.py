"""The launches of the HIP operator layer (diffsound_amd/modal_ops.py, hip_ops.py, block_ops.py), pinned without a GPU.

The library loads on the host and its symbolic routines run there; every operator method is then run on CPU tensors against a
stub library that records each call - the symbol and every argument, pointers as (name of the tensor they fall into, byte offset
into its storage), descriptor structs field by field - and the record is compared with tests/golden/ops_call_traces.json
(tests/golden/make_ops_call_traces.py writes it).  A wrong table, leading dimension, slice or a stale piece of lazy state is a
difference in the trace."""
import copy
import contextlib
import ctypes
import json
import os
from types import SimpleNamespace

import pytest
import torch

from diffsound_amd import _hip, meshgen, modal_ops
from diffsound_amd.lobpcg import precond as pc
from oracle import fem

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_call_traces.json")
_TetSystem, _HipModalOps = modal_ops.TetSystem, modal_ops.HipModalOps
# (pointer argument -> its count argument) of the calls that take an array of ds_block64_t by address
_BLOCK_TABLES = {"ds_mix64": {1: 0}, "ds_gram64_blocks": {1: 0, 3: 2}}


def _walk(name, v, depth):
    if isinstance(v, torch.Tensor):
        yield name, v
    elif depth and isinstance(v, dict):
        for k, x in v.items():
            yield from _walk(f"{name}[{k}]", x, depth - 1)
    elif depth and isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            yield from _walk(f"{name}[{i}]", x, depth - 1)


class Recorder:
    """The stub library (``lib``) and what it recorded (``calls``).  ``named``: the operand tensors of the running case;
    ``owners``: (label, object) pairs whose tensor attributes - dictionaries two levels deep - name a pointer too, looked up at
    the moment of the call (scratch blocks, lazily formed arrays)."""

    def __init__(self):
        self.calls, self.named, self.owners = [], [], []
        rec = self

        class Lib:
            def __getattr__(self, symbol):
                if symbol.startswith("_"):
                    raise AttributeError(symbol)
                return lambda *args: rec.call(symbol, args)

        self.lib = Lib()

    def note(self, what, value):
        self.calls.append(["note", what, value])

    def _ranges(self):
        out = []
        tensors = list(self.named)
        for label, obj in self.owners:
            for k, v in vars(obj).items():
                tensors.extend(_walk(f"{label}.{k}", v, 2))
        for name, t in tensors:
            st = t.untyped_storage()
            if st.nbytes():
                out.append((st.data_ptr(), st.data_ptr() + st.nbytes(), name))
        return out

    @staticmethod
    def _resolve(p, ranges):
        if not p:
            return None
        hits = sorted((name, p - lo) for lo, hi, name in ranges if lo <= p < hi)
        return list(hits[0]) if hits else "?"

    def _dump(self, s, ranges):
        out = {}
        for fname, ftype in s._fields_:
            v = getattr(s, fname)
            if isinstance(v, ctypes.Structure):
                out[fname] = self._dump(v, ranges)
            elif ftype is ctypes.c_void_p:
                out[fname] = self._resolve(v, ranges)
            elif isinstance(v, ctypes._Pointer):
                out[fname] = None if not v else (self._dump(v.contents, ranges) if isinstance(v.contents, ctypes.Structure) else "host")
            else:
                out[fname] = v
        return out

    def dump(self, s):
        return self._dump(s, self._ranges())

    def call(self, symbol, args):
        argtypes = _hip._SIGNATURES[symbol][1]
        assert len(args) == len(argtypes), f"{symbol}: {len(args)} arguments for a signature of {len(argtypes)}"
        ranges, out = self._ranges(), []
        for i, (a, ty) in enumerate(zip(args, argtypes)):
            if ty is ctypes.c_void_p and i in _BLOCK_TABLES.get(symbol, {}):
                arr = (_hip.Block64 * args[_BLOCK_TABLES[symbol][i]]).from_address(a)
                out.append([self._dump(b, ranges) for b in arr])
            elif ty is ctypes.c_void_p:
                out.append(self._resolve(a, ranges))
            elif hasattr(a, "_obj"):  # ctypes.byref(struct)
                s = a._obj
                out.append(self._dump(s, ranges) if isinstance(s, (_hip.LevelDesc, _hip.TwoLevelDesc, _hip.LobpcgDesc)) else type(s).__name__)
            else:
                assert isinstance(a, (int, float)), (symbol, i, a)
                out.append(a)
        if symbol == "ds_gram_workspace_bytes":
            # grows with the shape, so that a maximum over shapes shows in what is allocated; a run of queries (the native
            # iteration asks for every shape it forms) is one record: their number, the largest answer, a checksum of the shapes
            need, last = 1024 + 64 * args[1] * args[2], self.calls[-1] if self.calls else [None]
            if last[0] != "ds_gram_workspace_bytes, run":
                last = ["ds_gram_workspace_bytes, run", 0, 0, 0]
                self.calls.append(last)
            last[1:] = [last[1] + 1, max(last[2], need), (last[3] * 1000003 + args[0] * 10007 + args[1] * 211 + args[2]) % (1 << 31)]
            return need
        self.calls.append([symbol, out])
        return 4096 if "_workspace_" in symbol else 0


def _host_pattern(tets, nv, cap):
    """What _hip.DevicePattern hands the constructor, from the library's host routines on CPU tensors."""
    pat = _hip.Pattern(tets, nv)
    g = _hip.Groups(pat.rowptr, pat.colidx, nv)
    pat.ne, pat.gent, pat.kperm, pat.ngroups = g.ne, g.gent, g.kperm, g.ngroups
    pat.utab, pat.ctab = _hip.union_chunks(g.gptr, g.goff, cap)
    pat.single = pat.ctab.shape[0] == pat.utab.shape[0]
    return pat


def _stand_in(vertices, tets, order, density, reorder=True):
    """What TetSystem.__init__ builds, by the constructor's own steps on CPU tensors: only the pattern comes from elsewhere, and
    there is no assembly (the values stay zero)."""
    s = object.__new__(_TetSystem)
    s._number_nodes(vertices, tets, order, density, reorder)
    s._take_pattern(_host_pattern(s.tets, s.nv, modal_ops.UNION_CAP))
    s._element_tables_and_values()
    s._lazy_slots()
    for values in (s.klam, s.kmu, s.ms, s._tetgeo):
        values.zero_()
    return s


def test_stand_in_has_the_attributes_the_constructor_sets(monkeypatch):
    """The constructor itself, run on the host with its pattern source replaced and its assembly skipped, sets exactly the
    instance attributes of the stand-in: an attribute added to TetSystem.__init__ outside the shared steps fails here."""
    v, t = meshgen.kuhn_box(2)
    v, t = torch.from_numpy(v).float(), torch.from_numpy(t).long()
    monkeypatch.setattr(_hip, "require_gpu", lambda *tensors: None)
    monkeypatch.setattr(_hip, "DevicePattern", _host_pattern)
    monkeypatch.setattr(_TetSystem, "assemble", lambda self, vertices=None: None)
    for reorder in (True, False):
        built = vars(_TetSystem(v, t, 1, 2700.0, reorder))
        assert built and sorted(built) == sorted(vars(_stand_in(v, t, 1, 2700.0, reorder)))


class Env:
    """One recording session: the 3 x 3 x 3 Kuhn cube at order 2 with its corner-node level, and the patches under which the
    operator layer runs on it."""

    def __init__(self, mp):
        self.mp, self.rec = mp, Recorder()
        v, t = meshgen.kuhn_box(3)
        self.v, self.t = fem.to_high_order(torch.from_numpy(v), torch.from_numpy(t).long(), 2)
        mp.setattr(modal_ops, "TetSystem", _stand_in)  # (coarse_level() builds the corner-node system through this name)
        self.rigid_calls = 0

        def rigid(ops):
            self.rigid_calls += 1
            return None

        mp.setattr(_HipModalOps, "_rigid_basis", rigid)
        mp.setattr(_hip, "require_gpu", lambda *tensors: None)
        mp.setattr(_hip, "blas_one_thread", contextlib.nullcontext)
        mp.setattr(_hip, "lapack_table", lambda source=None: _hip.LapackTable())
        mp.setattr(torch.cuda, "current_stream", lambda device=None: SimpleNamespace(synchronize=lambda: None))
        self.real_lib = _hip.lib
        self.base = self.system()
        assert (self.base.nv, self.base.nnzb, self.base.groups["union"]["ngroups"]) == (343, 7525, 86)
        assert self.base.groups["union"]["single"] and self.base._coarse["sys"].nv == 64
        mp.setattr(_hip, "lib", lambda: self.rec.lib)
        mp.setattr(_hip, "stream_ptr", lambda: 0)

    def system(self):
        with self.mp.context() as m:  # (the symbolic routines are the library's own)
            m.setattr(_hip, "lib", self.real_lib)
            s = _stand_in(self.v.float(), self.t, 2, 2700.0)
            assert s.coarse_level() is not None
        return s

    def ops(self, sysd=None, **kw):
        """A HipModalOps on (a shallow copy of) the shared system; the constructor's own calls are dropped from the record."""
        keep = self.rec.calls
        self.rec.calls = []
        o = _HipModalOps(copy.copy(self.base) if sysd is None else sysd, 2.0, 3.0, **kw)
        self.rec.calls = keep
        self.own(o)
        return o

    def own(self, o):
        self.rec.owners = [("fine", o), ("fine.sys", o.sys)]
        if o.coarse is not None:
            self.rec.owners += [("coarse", o.coarse), ("coarse.sys", o.coarse.sys)]

    def blk(self, name, rows, cols, dtype=torch.float32, ld=None, skip=0):
        """A named (rows x cols) block with leading dimension ``ld``, ``skip`` elements into its storage."""
        ld = ld or cols
        t = torch.zeros(rows * ld + skip, dtype=dtype)[skip:].view(rows, ld)[:, :cols]
        self.rec.named.append((name, t))
        return t

    def vec(self, name, n, dtype=torch.float64):
        t = torch.zeros(n, dtype=dtype)
        self.rec.named.append((name, t))
        return t


def _products(env, o, transfers):
    rec, n = env.rec, o.n
    for c in (8, 24, 84, 136, 6):
        X, Y, Z = (env.blk(f"{nm}{c}", n, c) for nm in "XYZ")
        o.apply_K(X, Y)
        o.apply_M(X, Y)
        ok = o.apply_KM_ok(X, Y, Z)
        rec.note(f"apply_KM_ok {c}", bool(ok))
        if ok:
            o.apply_KM(X, Y, Z)
    Xu, Yu = env.blk("Xu", n, 24, skip=1), env.blk("Yu", n, 24)
    o.apply_K(Xu, Yu)
    o.apply_M(Xu, Yu)
    X, R, MX, lam = env.blk("X136", n, 136), env.blk("R136", n, 136), env.blk("MX136", n, 136), env.vec("lam136", 136)
    ok = o.residual_fused_ok(X, R)
    rec.note("residual_fused_ok", bool(ok))
    if ok:
        o.residual_fused(X, lam, R)
    o.residual(R, MX, X, lam)
    o.residual(R, MX, X, lam, src=env.blk("KX136", n, 136))
    for c in (24, 6):
        A, B, C = (env.blk(f"{nm}{c}", n, c) for nm in ("Wk", "Wprev", "R0"))
        o.spmm_residual(A, C, B)
        o.cheb_spmm(A, B, C, 0.5, 0.25, True)
        o.cheb_spmm(A, B, C, 0.5, 0.25, False)
        o.cheb_init(C, A, B, 0.5)
        o.cheb_step(env.blk(f"AD{c}", n, c), C, A, B, 0.5, 0.25)
    if transfers:
        Rf, Rc = env.blk("Rf", n, 24), env.blk("Rc", o.coarse.n, 24)
        o.restrict(Rf, Rc)
        o.prolong(Rc, Rf)
        o.prolong_add(Rc, Rf)
        rec.note("coarse counts", dict(o.coarse.counts))
    rec.note("counts", dict(o.counts))


def _level(env, o):
    rec, n = env.rec, o.n
    d = o.level_desc(_hip.LevelDesc(), 3, 2.0, 0.125)
    rec.note("level_desc", None if d is None else rec.dump(d))
    if d is not None:
        A, B, C = (env.blk(nm, n, 24, torch.bfloat16) for nm in ("Wk16", "Wprev16", "R016"))
        o.cheb_spmm16(A, B, C, 0.5, 0.25, True)
    R, W = env.blk("R", n, 24), env.blk("W", n, 24)
    rec.note("chebyshev_apply16", o.chebyshev_apply16(SimpleNamespace(degree=3, lmax=2.0, lmin=0.125), R, W))
    rec.note("chebyshev_apply16 degree 1", o.chebyshev_apply16(SimpleNamespace(degree=1, lmax=2.0, lmin=0.125), R, W))
    rec.note("counts", dict(o.counts))


def _twolevel(env, o):
    rec, n, nc = env.rec, o.n, o.coarse.n
    for dt, tag in ((torch.float32, "32"), (torch.bfloat16, "16"), (torch.float32, "32b")):
        R, W = env.blk("R" + tag, n, 24), env.blk("W" + tag, n, 24)
        D, AD, Rr, Wc = (env.blk(nm + tag, n, 24, dt) for nm in ("D", "AD", "Rr", "Wc"))
        Rc, Ec, Dc, ADc = (env.blk(nm + tag, nc, 24, dt, ld=28 if (nm, tag) == ("Ec", "32b") else None) for nm in ("Rc", "Ec", "Dc", "ADc"))
        R16 = env.blk("R16", n, 24, dt) if dt == torch.bfloat16 else None
        rec.note("twolevel_apply " + tag, o.twolevel_apply((3, 2.0, 0.2), (5, 3.0, 0.01), R, W, D, AD, Rr, Rc, Ec, Dc, ADc, Wc, R16=R16))
    rec.note("counts", [dict(o.counts), dict(o.coarse.counts)])


def _cheb(o, degree, lmax, lmin):
    p = object.__new__(pc.ChebyshevBlockJacobi)
    p.ops, p.degree, p.lmax, p.lmin, p.group = o, degree, lmax, lmin, int(o.group_jacobi or 0)
    return p


def _lobpcg(env, o, kind, storage, b=24, wait=None):
    rec, n, ny, k = env.rec, o.n, 8, 16
    if kind == "twolevel":
        p = object.__new__(pc.TwoLevelChebyshev)
        p.ops, p.smooth, p.coarse = o, _cheb(o, 3, 2.0, 0.2), _cheb(o.coarse, 5, 3.0, 0.01)
    else:
        p = _cheb(o, 4, 2.0, 0.0025)
    cfg = SimpleNamespace(precond_storage=storage, maxit=5, lock=True, ortho_passes=2, rr_refresh=3, kx_fresh=True, raw_rr=True,
                          ortho_tol=1e-3, fused_residual=True, ritz_tol=0.25)
    if wait is not None:
        o.host_wait_mode = wait
    tag = f"{b}"
    S, S2 = env.blk("S" + tag, n, ny + 3 * b), env.blk("S2" + tag, n, ny + 3 * b)
    KS, KS2 = env.blk("KS" + tag, n, 3 * b), env.blk("KS2" + tag, n, 3 * b)
    R, MX, MW = (env.blk(nm + tag, n, b) for nm in ("R", "MX", "MW"))
    out = o.native_lobpcg(p, cfg, k, b, ny, S, S2, KS, KS2, R, MX, MW, torch.ones(b, dtype=torch.float64), 1.5, 0.5, 1e-5)
    rec.note(f"native_lobpcg {kind} {storage} {b}", None if out is None else [out[0], out[1], out[2].tolist(), out[3].tolist(), out[4]])
    rec.note("scratch", [{k_: [list(t.shape), str(t.dtype)] for k_, t in x._tmp.items()} for x in (o, o.coarse)])


def _dense(env, o):
    rec, n = env.rec, o.n
    A, B, A64 = env.blk("A", n, 24), env.blk("B", n, 48, ld=52), env.blk("A64", n, 24, torch.float64)
    o.gram(A, B)
    o.gram(A64, B, symmetric=True)
    o.gram(A, A64, exact=True)
    o.gram_exact = True
    o.gram(A, B)
    o.gram_exact = False
    blocks = [env.blk(f"b{i}", n, 4 + 4 * (i % 2), torch.float64) for i in range(5)]
    o.gram_blocks(blocks[:2], blocks[2:5], symmetric=False)
    o.gram_blocks(blocks[:3], blocks[:3], symmetric=True)
    for c in (160, 164):
        W, O, T = env.blk(f"W{c}", n, c), env.blk(f"O{c}", n, c), torch.zeros((c, c), dtype=torch.float64)
        o.mix(W, T, O, alpha=0.5, beta=2.0)
        o.mix_inplace(W, T)
    p = sum(b_.shape[1] for b_ in blocks)
    C, out = env.blk("C64", p + 8, 8, torch.float64), env.blk("out64", n, 8, torch.float64)
    o.mix64(blocks, C, out)
    o.mix64(blocks, C, out, alpha=2.0, beta=1.0)
    o.mix64([blocks[0], (blocks[3], 12), blocks[1]], C, out)
    o.mix64(blocks[:1], C)
    KX, MX, X = (env.blk(nm, n, 8, torch.float64) for nm in ("KX64", "MX64", "X64"))
    o.residual64(KX, MX, X, env.vec("lam8", 8))
    before = len(rec.calls)
    o.residual64(KX[:, :7], MX[:, :7], X[:, :7], env.vec("lam7", 7))
    rec.note("residual64 at 7 columns: calls", len(rec.calls) - before)
    o.residual64_scaled(KX, MX, env.vec("lam8b", 8), env.vec("scale8", 8), torch.tensor([1, 2, 5, 6]))
    o.residual64_scaled(KX, MX, env.vec("lam8c", 8), env.vec("scale8c", 8), torch.tensor([0, 1, 2, 3]), out=env.blk("R32", n, 4))
    rec.note("counts", dict(o.counts))
    rec.note("scratch", {k_: [list(t.shape), str(t.dtype)] for k_, t in o._tmp.items()})


def _k64(env, o):
    rec, n = env.rec, o.n
    X, Y, X6, Y6 = (env.blk(nm, n, c, torch.float64) for nm, c in (("X24", 24), ("Y24", 24), ("X6", 6), ("Y6", 6)))

    def state(where):
        assert o._k64 is None or where == "inside"
        rec.note(where, [isinstance(o._k64, torch.Tensor), o._k64grp is None, o._m64grp is None])  # (BSR-order array kept?)

    rec.note("terms", len(o.apply_K64(X, Y, terms=True)))
    o.apply_M64(X, Y)
    o.combined_k64(True)
    for x, y in ((X, Y), (X6, Y6), (X, Y)):  # the union kernel, then the BSR-order array, which then stays in use
        rec.note("parts", o.apply_K64(x, y))
        state("inside")
        o.apply_M64(x, y)
        state("inside")
    rec.note("terms inside", len(o.apply_K64(X, Y, terms=True)))
    o.combined_k64(False)
    state("after combined_k64(False)")
    o.apply_K64(X, Y)
    o.apply_M64(X, Y)
    o.combined_k64(True)
    o.apply_K64(X6, Y6)  # (the first block does not qualify: no group-order copy, and none for M either)
    o.apply_M64(X, Y)
    o.apply_K64(X, Y)
    state("inside")
    o.set_material(4.0, 5.0)
    state("after set_material")
    o.combined_k64(True)
    o.apply_K64(X, Y)
    o.set_tangent(modal_ops.isotropic_tangent(2.0, 3.0))
    state("after set_tangent")
    o.combined_k64(True)
    o.apply_K64(X, Y)  # tangent mode: one term
    o.apply_M64(X, Y)
    o.combined_k64(False)
    state("after combined_k64(False)")
    rec.note("scratch", {k_: [list(t.shape), str(t.dtype)] for k_, t in o._tmp.items()})


def _polish(env, o):
    rec, n = env.rec, o.n
    for c in (24, 6):
        X = env.blk(f"X{c}", n, c)
        GK, coef, GM = o.polish_products(X)
        rec.note(f"polish_products {c}", [[list(g.shape) for g in GK], list(coef), list(GM.shape)])
        pr = o.probe_products(X)
        rec.note(f"probe_products {c}", None if pr is None else [[list(y.shape), list(y.stride())] for y in pr])
    o.polish_f32_blocks = True
    o.polish_products(env.blk("X24f", n, 24))
    o.polish_f32_blocks = False
    o.set_tangent(modal_ops.isotropic_tangent(2.0, 3.0))
    X = env.blk("X24t", n, 24)
    rec.note("tangent mode", [len(o.polish_products(X)[0]), o.probe_products(X) is None])
    ks, m = o.vector_forms(env.blk("U6", n, 6))
    rec.note("vector_forms", [len(ks), list(m.shape)])
    rec.note("counts", dict(o.counts))
    rec.note("scratch", {k_: [list(t.shape), str(t.dtype)] for k_, t in o._tmp.items()})


def _materials(env, o):
    rec = env.rec

    def state(where):
        assert o._k64 is None
        rec.note(where, [getattr(o, "_norm_probe", "unset"), getattr(o.coarse, "_norm_probe", "unset"), o.lame,
                         None if o.tangent is None else o.tangent.tolist()[0][:2], env.rigid_calls, o.norm_probe_key()[1]])

    env.rigid_calls = 0
    o._norm_probe = o.coarse._norm_probe = "kept"
    o.set_material(4.0, 5.0)
    state("set_material")
    o.set_tangent(torch.from_numpy(modal_ops.isotropic_tangent(2.0, 3.0)))
    state("set_tangent")
    o._norm_probe = "kept"
    o.set_tangent(modal_ops.isotropic_tangent(2.5, 3.0))
    state("set_tangent again")
    o.set_material(4.0, 5.0)
    state("set_material after a tangent")
    o.sys.assemble(env.v.float() * 1.25)  # new coordinates: the next material re-forms the rigid-body basis, once
    o.set_material(4.0, 5.0)
    state("set_material on a new geometry")
    o.set_tangent(modal_ops.isotropic_tangent(2.0, 3.0))
    state("set_tangent on the same geometry")
    o.sys.assemble(env.v.float() * 1.5)
    o.set_tangent(modal_ops.isotropic_tangent(2.0, 3.0))
    state("set_tangent on a new geometry")
    for what, call in (("set_tangent shape", lambda: o.set_tangent(torch.zeros(3, 3))),
                       ("set_tangent finite", lambda: o.set_tangent(torch.full((9, 9), float("nan")))),
                       ("tangent_forms U", lambda: o.tangent_forms(torch.zeros(o.n, 4, dtype=torch.float64))),
                       ("tangent_forms rows", lambda: o.tangent_forms(torch.zeros(o.n - 3, 4))),
                       ("geometry_grad_tangent U", lambda: o.sys.geometry_grad_tangent(torch.zeros(o.n, 0), [], [], torch.zeros(9, 9))),
                       ("geometry_grad_tangent C", lambda: o.sys.geometry_grad_tangent(torch.zeros(o.n, 4), [1.0] * 4, [1.0] * 4, torch.zeros(9, 8))),
                       ("geometry_grad_tangent gk", lambda: o.sys.geometry_grad_tangent(torch.zeros(o.n, 4), [1.0] * 3, [1.0] * 4, torch.zeros(9, 9)))):
        with pytest.raises(ValueError) as ex:
            call()
        rec.note(what, str(ex.value))
    U = env.blk("U", o.n, 4)
    rec.note("tangent_forms", list(o.tangent_forms(U).shape))
    rec.note("tangent_forms, transposed block", list(o.tangent_forms(env.blk("Ut", 4, o.n).T).shape))
    rec.note("geometry_grad", list(o.geometry_grad(U, [1.0, 2.0, 3.0, 4.0], torch.ones(4)).shape))
    rec.note("scratch", {k_: [list(t.shape), str(t.dtype)] for k_, t in o._tmp.items()})


def _assemble(env):
    rec = env.rec
    s = env.system()
    c = s._coarse["sys"]
    rec.owners = [("sys", s), ("coarse.sys", c)]

    def state(where):
        rec.note(where, [getattr(x, name, unset) for x in (s, c)
                         for name, unset in (("geometry_generation", 0), ("_assembled_generation", None), ("assemblies_skipped", 0))])

    state("as built")
    s.assemble()
    state("no coordinates")
    s.assemble(env.v.float())
    state("the same coordinates")
    s.assemble(env.v.float())
    state("the same coordinates again: skipped")
    s.assemble()
    state("no coordinates: always assembles")
    s.assemble(env.v.float() * 1.25)
    state("changed coordinates")
    o = s.with_own_values()
    rec.owners = [("own", o), ("own.coarse.sys", o._coarse["sys"]), ("sys", s)]
    rec.note("with_own_values", [o.klam is not s.klam, o._coarse["sys"] is not c, o._coarse["sys"].klam is not c.klam, o.groups is s.groups,
                                 getattr(o, "geometry_generation", 0), getattr(o, "assemblies_skipped", 0)])
    o.assemble(env.v.float() * 1.25)
    o.assemble(env.v.float())
    rec.note("generations", [getattr(x, "geometry_generation", 0) for x in (s, o, c, o._coarse["sys"])])
    mt = o.mfma_tables(8)
    rec.note("tables are shared", [mt is o.mfma_tables(8), o.mfma_tables_dense(8) is o.mfma_tables_dense(8),
                                   sorted(str(k_) for k_ in o._mfma_tables)])


def call_traces(mp):
    """{case: [[symbol, arguments] | ["note", what, value], ...]} of every case; ``mp`` a pytest.MonkeyPatch."""
    env = Env(mp)
    traces = {}

    def case(name, run, *args, **kw):
        env.rec.calls, env.rec.named = [], []
        run(env, *args, **kw)
        assert name not in traces
        traces[name] = json.loads(json.dumps(env.rec.calls))  # (tuples as lists, as the fixture holds them)

    def construct(env_, **kw):
        o = _HipModalOps(copy.copy(env_.base), 2.0, 3.0, **kw)
        env_.own(o)
        env_.rec.note("state", [o._mfma is not None, o.group_jacobi, o.coarse.group_jacobi, o._mfma32 is not None, o.k4 is not None,
                                o.coarse._mfma_dense is not None, o._level_tag, o.coarse._level_tag, env_.rigid_calls])

    case("construct", construct)
    case("construct mfma32", construct, mfma32=True)
    case("construct valu", construct, mfma_groups=(0, 0), coarse_group_jacobi=0)
    case("products", lambda e: _products(e, e.ops(), True))
    case("products corner level", lambda e: _products(e, e.ops().coarse, False))
    case("products mfma32", lambda e: _products(e, e.ops(mfma32=True), True))

    def no_groups(e, union_only):
        s = copy.copy(e.base)
        s.groups = dict(s.groups, union=None) if union_only else None
        o = e.ops(s)
        _products(e, o, True)
        _level(e, o)

    case("products groups None", no_groups, False)
    case("products union None", no_groups, True)

    def m_kind0(e):
        o = e.ops()
        o.m_kind = 0
        _products(e, o, True)

    case("products m_kind 0", m_kind0)

    def multi_chunk(e):
        s = copy.copy(e.base)
        s.groups = dict(s.groups, union=dict(s.groups["union"], single=False))
        o = e.ops(s)
        X, Y, Z = (e.blk(nm, o.n, 24) for nm in "XYZ")
        o.apply_K(X, Y)
        o.apply_K(X[:, :8], Y[:, :8])
        o.apply_KM(X, Y, Z)
        o.residual_fused(X, e.vec("lam", 24), Z)
        _level(e, o)
        _k64(e, o)

    case("utab given", multi_chunk)
    case("level", lambda e: _level(e, e.ops()))
    case("level corner, group Jacobi", lambda e: _level(e, e.ops().coarse))
    case("level valu", lambda e: _level(e, e.ops(mfma_groups=(0, 0), coarse_group_jacobi=0)))
    case("level mfma32", lambda e: _level(e, e.ops(mfma32=True)))
    case("twolevel", lambda e: _twolevel(e, e.ops()))
    case("twolevel node Jacobi", lambda e: _twolevel(e, e.ops(coarse_group_jacobi=0)))
    case("lobpcg chebyshev fp32", lambda e: _lobpcg(e, e.ops(), "chebyshev", "fp32"))
    case("lobpcg chebyshev bf16", lambda e: _lobpcg(e, e.ops(), "chebyshev", "bf16", wait=1))
    case("lobpcg twolevel fp32", lambda e: _lobpcg(e, e.ops(coarse_group_jacobi=0), "twolevel", "fp32"))
    case("lobpcg twolevel bf16", lambda e: _lobpcg(e, e.ops(), "twolevel", "bf16"))
    case("lobpcg twolevel bf16 wide", lambda e: _lobpcg(e, e.ops(), "twolevel", "bf16", b=136))
    case("lobpcg None: 164 columns", lambda e: _lobpcg(e, e.ops(), "twolevel", "bf16", b=164))
    case("lobpcg None: group Jacobi in fp32", lambda e: _lobpcg(e, e.ops(), "twolevel", "fp32"))

    def twice(e):
        o = e.ops()
        _lobpcg(e, o, "twolevel", "bf16")
        _lobpcg(e, o, "twolevel", "bf16")  # (the workspace need is kept per shape)
        _lobpcg(e, o, "chebyshev", "bf16", b=48)
        _twolevel(e, o)

    case("lobpcg twice, then a cycle", twice)
    case("dense", lambda e: _dense(e, e.ops()))
    case("k64", lambda e: _k64(e, e.ops()))
    case("k64 groups None", lambda e: _k64(e, e.ops(_no_groups(e))))
    case("polish", lambda e: _polish(e, e.ops()))
    case("materials", lambda e: _materials(e, e.ops(e.system())))
    case("materials mfma32", lambda e: _materials(e, e.ops(e.system(), mfma32=True)))
    case("assemble", _assemble)
    return traces


def _no_groups(e):
    s = copy.copy(e.base)
    s.groups = None
    return s


def test_call_traces_equal_the_recorded_ones(monkeypatch):
    """Every launch of every operator method, argument by argument, equals the record taken before the operator layer was
    reorganised (see the module docstring)."""
    with open(GOLDEN) as f:
        want = json.load(f)
    got = call_traces(monkeypatch)
    assert sorted(got) == sorted(want)
    for name in want:
        assert len(got[name]) == len(want[name]), name
        for i, (g, w) in enumerate(zip(got[name], want[name])):
            assert g == w, (name, i)


def test_earlier_launch_name_and_the_corner_level_setters(monkeypatch):
    """The benchmark's roofline and tools/mb_*.py time the fused Chebyshev term under its earlier name ``_cheb_spmm_launch``: it
    is the same launch.  And the corner-node level receives every material through its PUBLIC setters, as an operator object
    that overrides them expects."""
    env = Env(monkeypatch)
    o = env.ops()
    A, B, C = (env.blk(nm, o.n, 24) for nm in ("Wk", "Wprev", "R0"))
    env.rec.calls = []
    o.cheb_spmm(A, B, C, 0.5, 0.25, False)
    want, env.rec.calls = env.rec.calls, []
    o._cheb_spmm_launch(A, B, C, 0.5, 0.25, False)
    assert len(want) == 1 and want[0][0] == "ds_spmm_union" and env.rec.calls == want
    seen = []
    monkeypatch.setattr(o.coarse, "set_material", lambda lam, mu: seen.append(("material", lam, mu)), raising=False)
    monkeypatch.setattr(o.coarse, "set_tangent", lambda C_: seen.append(("tangent", C_.shape)), raising=False)
    o.set_material(4.0, 5.0)
    o.set_tangent(torch.from_numpy(modal_ops.isotropic_tangent(2.0, 3.0)))
    assert seen == [("material", 4.0, 5.0), ("tangent", (9, 9))]
