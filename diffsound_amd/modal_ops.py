"""Device-side FEM system: the MESH side of the operator layer.

``TetSystem``   one mesh (topology + geometry): node ordering (``morton_order``), symbolic BSR-3 pattern with its union and
                MFMA tables, then K_lambda, K_mu, M_s assembled on the GPU in fp64 (reference
                DiffSoundObj.update_stiff_matrix / update_mass_matrix, src/diffelastic/diff_model.py:184-312), and the
                geometry gradients.
The material side - ``HipModalOps``, ``HipSparseOps``: one hypothesis's values, packing, rigid basis and polish terms - is
hip_ops.py, which imports this module; the names it took with it still resolve from here (``__getattr__`` below).
This file decides memory traffic, and the benchmark hashes it into the key of its traffic records for that reason: keep what
cannot change the node ordering or the tables out of it, so that the key covers the ordering and the tables and nothing else.
No operation here has a CPU implementation; tensors must be HIP tensors.
"""
import copy
import threading

import numpy as np
import torch

from . import _hip, fem_tables
from .block_ops import DS_F32, DS_F64, _HipBlockOps, _ld  # noqa: F401  (importable from here as before the split)

_IN_HIP_OPS = ("isotropic_tangent", "HipModalOps", "_coo_to_bsr3", "HipSparseOps")


def __getattr__(name):
    """The names that moved to hip_ops.py, by attribute and by ``from ... import``, whichever module is imported first."""
    if name in _IN_HIP_OPS:
        from . import hip_ops

        return getattr(hip_ops, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


MF_BATCH = 16  # entries per LDS batch of the MFMA kernel (DS_MF_BATCH of include/diffsound_hip.h)
MF_TAIL = 2  # entries a group's last batch may take beyond MF_BATCH when no group has more than 128 (DS_MF_TAIL)
MF32_BATCH = 8  # entries per LDS batch of the fp32 MFMA kernel (DS_MF32_BATCH), groups of MF32_G = 4 nodes
MF32_G = 4
_MFMA_TABLES_LOCK = threading.Lock()
UNION_CAP = 140  # blocks per chunk of the neighbour-union tables (the kernel's LDS image; DS_UNION_CAP of the header)


def _axis_buckets(x, lq):
    """Bucket index of every node along ONE axis, and the bucket count.  A structured mesh - the benchmark's Kuhn boxes,
    jittered or not, plates, voxel-derived meshes - has its nodes on PLANES: the sorted coordinates then show a knee between
    the (planes - 1) large gaps that separate the planes and the tiny gaps inside them, and the planes themselves are the
    buckets (ties and jittered clusters stay together).  Without such a knee (unstructured meshes): ``lq`` equally populated
    quantile buckets."""
    nv = x.numel()
    s, o = torch.sort(x, stable=True)
    gaps = s[1:] - s[:-1]
    if gaps.numel():
        k = min(gaps.numel(), 4 * lq + 8)
        g = torch.topk(gaps, k).values  # the largest gaps, descending
        lo, hi = max(1, lq // 4), min(k - 1, 4 * lq)
        if hi > lo:
            ratio = g[lo - 1:hi] / g[lo:hi + 1].clamp(min=1e-300)
            j = int(torch.argmax(ratio))
            planes = lo + j + 1
            if float(ratio[j]) >= 3.0:
                tau = 0.5 * (g[planes - 2] + g[planes - 1])
                cid = torch.cat([torch.zeros(1, dtype=torch.int64, device=x.device), torch.cumsum((gaps > tau).long(), 0)])
                cnt = torch.bincount(cid)
                if int(cnt.max()) <= 4 * max(int(cnt.min()), 1):  # planes of comparable population, not outliers split off
                    q = torch.empty(nv, dtype=torch.int64, device=x.device)
                    q[o] = cid
                    return q, planes
    lq = max(1, lq)
    edges = s[(torch.arange(1, lq, device=x.device) * nv) // lq]
    return torch.searchsorted(edges, x.contiguous(), right=True), lq


def morton_order(vertices):
    """Permutation (new index -> old index) sorting nodes along a 3-D Morton (Z-order) curve over per-axis BUCKET indices
    (``_axis_buckets``: the mesh's own node planes where it has them, quantile slabs where not).  Consecutive node ranges
    then form compact bricks - groups of 4 / 8 consecutive nodes are 2 x 2 x 1 / 2 x 2 x 2 bricks of the node grid on a
    structured mesh - so the rows of a group share most of their neighbours (the neighbour-union SpMM kernels walk the
    UNION of a group's rows) and the block-SpMM's gathers stay inside one XCD's 4 MiB L2.
    Round 4: until then the curve ran over the absolute coordinates quantised to 10 bits, whose cells cut the node grid at
    arbitrary offsets; on the benchmark mesh the unions of 4 / 8 consecutive rows held 0.584 / 0.430 of the rows' blocks,
    with bricks aligned to the node planes 0.461 / 0.282 (unstructured meshes: unchanged within 1 %)."""
    v = vertices.detach().double()
    nv = v.shape[0]
    ext = (v.max(0).values - v.min(0).values).clamp(min=1e-300)
    vol = float(ext.prod())
    q, bits = [], 1
    for a in range(3):
        lq = int(min(1024, max(1, round((nv * float(ext[a]) ** 3 / vol) ** (1.0 / 3.0)))))  # aspect-aware slab count
        qa, la = _axis_buckets(v[:, a], lq)
        q.append(qa)
        bits = max(bits, max(la - 1, 1).bit_length())
    # (Round 5 tried the bricks along a HILBERT curve instead - consecutive bricks always face neighbours, partial bricks behind
    # the full ones so that groups stay aligned: the unions of 64 / 512 consecutive rows shrink by 9 / 7 %, but the kernels run
    # the same times and draw 2.5 % MORE bytes from memory (445 -> 456 MB per bf16 term, 740 -> 760 MB per [K W | M W]);
    # profiles/r05_order_ab.txt.  The Morton curve stays.)
    key = torch.zeros(nv, dtype=torch.int64, device=v.device)
    for b in range(bits):
        for a in range(3):
            key |= ((q[a] >> b) & 1) << (3 * b + a)
    return torch.argsort(key, stable=True)


def _tangent_array(C, who):
    """A 9 x 9 tangent (host tensor or array) as a contiguous fp64 array; ``who``: the caller, for the message."""
    C = np.ascontiguousarray(C.detach().cpu().numpy() if isinstance(C, torch.Tensor) else C, dtype=np.float64)
    if C.shape != (9, 9) or not np.isfinite(C).all():
        raise ValueError(f"{who}: a finite 9 x 9 tangent expected, got shape {C.shape}")
    return C


def _mode_block(U, n, who):
    """An (n x m) fp32 block of modes on the device, with unit column stride (copied when it has another)."""
    _hip.require_gpu(U)
    if U.dim() != 2 or U.shape[0] != n or U.dtype != torch.float32 or U.shape[1] < 1:
        raise ValueError(f"{who}: an (n x m) float32 block with m >= 1 expected")
    return U if U.stride(1) == 1 else U.contiguous()


def _mfma_ghead(grp, ewithin, gcol, gmeta, ng):
    """Fixed-stride record of each group's first 64 entries (ids, then meta words; zero behind the last): what a wave asks for
    before it knows where its group's entries start.  ``grp`` / ``ewithin``: group and position in it of every entry."""
    ghead = torch.zeros((ng, 128), dtype=torch.int32, device=gcol.device)
    sel = ewithin < 64
    ghead[grp[sel], ewithin[sel]] = gcol[sel]
    ghead[grp[sel], 64 + ewithin[sel]] = gmeta[sel]
    return ghead


class TetSystem:
    # What depends on the geometry only - the rigid-body basis, the solver's norm probe - is kept per GENERATION of the
    # coordinates: assemble(vertices) moves it when the coordinates differ from the kept ones.
    geometry_generation = 0
    _assembled_generation = None  # the generation K_lambda, K_mu and M_s were last assembled on
    assemblies_skipped = 0  # calls of assemble(vertices) that found the same coordinates assembled already

    def __init__(self, vertices, tets, order, density, reorder=True):
        """vertices (nv,3) float32 HIP tensor, tets (T,N) integer HIP tensor in the reference's local
        node order, N = 4 / 10.  With ``reorder`` the nodes are renumbered internally along a Morton
        curve; ``perm`` / ``inv_perm`` map between the caller's node ids and the internal ones and
        ``rows_to_external`` / ``rows_to_internal`` convert (n x c) DOF blocks."""
        _hip.require_gpu(vertices, tets)
        self._number_nodes(vertices, tets, order, density, reorder)
        self._take_pattern(_hip.DevicePattern(self.tets, self.nv, UNION_CAP))
        self._element_tables_and_values()
        self._lazy_slots()
        self.assemble()

    # The steps of the constructor.  The call-trace test (tests/test_ops_calls_cpu.py) builds its host-side system from these same
    # steps, with a pattern from the library's host routines: an attribute the constructor is to set belongs in one of them.
    def _number_nodes(self, vertices, tets, order, density, reorder):
        self.order = int(order)
        self.N = fem_tables.NODES_PER_TET[self.order]
        if tets.shape[1] != self.N:
            raise ValueError(f"tets must have {self.N} columns for order {order}")
        self.device = vertices.device
        if reorder:
            self.perm = morton_order(vertices)  # internal -> external
            self.inv_perm = torch.empty_like(self.perm)
            self.inv_perm[self.perm] = torch.arange(vertices.shape[0], device=self.device)
            self.vertices = vertices.detach().to(torch.float32)[self.perm].contiguous()
            self.tets = self.inv_perm[tets.long()].to(torch.int32).contiguous()
        else:
            self.perm = self.inv_perm = None
            # (a PRIVATE copy: an fp32 contiguous input would otherwise be kept by reference, and a caller that later moves its
            # coordinates in place would move this snapshot with them - assemble(vertices) could then never see a change)
            self.vertices = vertices.detach().to(torch.float32).contiguous().clone()
            self.tets = tets.to(torch.int32).contiguous()
        self.nv = self.vertices.shape[0]
        self.n = 3 * self.nv
        self.T = self.tets.shape[0]
        self.density = float(density)

    def _take_pattern(self, pat):
        """``pat``: the symbolic phase's result (on the device: ds_dpattern_build) - pattern, per-slot contribution lists (the
        numeric phase then needs neither COO, sort nor atomics) and the tables of the neighbour-union SpMM (ds_spmm_union, the
        kernel of every product on blocks of <= 84 columns): one wavefront per 4 consecutive nodes walks the union of their
        neighbours (with the Morton numbering 0.58 x as many panel loads as one wavefront per node).  Every group is cut into
        chunks of whole entries that fit the kernel's LDS images (cap entries / blocks; almost always ONE chunk): ctab rows
        (e0, e1, b0, b1), utab rows (first chunk, end chunk) per group."""
        self.nnzb = pat.nnzb
        self.rowptr, self.colidx, self.diagidx, self.cptr, self.clist = pat.rowptr, pat.colidx, pat.diagidx, pat.cptr, pat.clist
        self.groups = None
        if self.nv >= 8:
            self.groups = dict(ne=pat.ne, gent=pat.gent, kperm=pat.kperm, kperm64=pat.kperm.long(),
                               union=dict(utab=pat.utab, ctab=pat.ctab, capb=UNION_CAP, ngroups=pat.ngroups,
                                          single=pat.single))  # single: every group is one chunk

    def _element_tables_and_values(self):
        """The reference element's tables, and the arrays ``assemble`` writes."""
        dev = self.device
        self.dtab = torch.from_numpy(fem_tables.stiffness_table(self.order)).to(dev)
        self.mtab = torch.from_numpy(fem_tables.mass_table(self.order, self.density)).to(dev)
        self.klam = torch.empty((self.nnzb, 9), dtype=torch.float64, device=dev)
        self.kmu = torch.empty((self.nnzb, 9), dtype=torch.float64, device=dev)
        self.ms = torch.empty((self.nnzb,), dtype=torch.float64, device=dev)
        self._tetgeo = torch.empty((self.T, 13), dtype=torch.float64, device=dev)

    def _lazy_slots(self):
        self._coarse = None
        self._mfma_tables = {}  # mfma_tables() / mfma_tables_dense(): topology only, shared by the views of with_own_values()
        self._cinc = None  # corner_incidence(): topology only, built on first use
        self._grad_rule = None  # gradient_rule(): the minimal gradient rule on the device, built on first use

    def _cached_tables(self, key, build):
        """The topology tables kept under ``key``, built with ``build()`` on first use."""
        cache = self._mfma_tables
        with _MFMA_TABLES_LOCK:  # hypothesis lanes share the cache (with_own_values copies the dict reference)
            if key not in cache:
                cache[key] = build()
                torch.cuda.current_stream(self.device).synchronize()  # other lanes use the tables on their own streams
        return cache[key]

    def mfma_tables(self, group_nodes=8, batch=MF_BATCH):
        """Topology tables of the MFMA forms - of the bf16 terms (ds_spmm_union16m, groups of 8 consecutive nodes, batches of
        16 entries) and of the eigensolver's fp32 products (ds_spmm_union32m, groups of 4, batches of 8):
        gptr / gcol = the sorted union of the column ids of each group's rows; gmeta per entry = presence mask of the
        group's nodes | (first block of the entry inside the group) << 8; gbase = first block of each group; kperm = BSR
        block of every position of the (group, entry, node) order.  Built once per topology with device sorts."""
        key = (int(group_nodes), int(batch))
        return self._cached_tables(key, lambda: self._build_mfma_tables(*key))

    def _build_mfma_tables(self, group_nodes, mf_batch):
        G, nv, dev = int(group_nodes), self.nv, self.device
        rows = torch.repeat_interleave(torch.arange(nv, device=dev), (self.rowptr[1:] - self.rowptr[:-1]).long())
        key = ((rows // G) * nv + self.colidx.long()) * G + rows % G
        key, order = torch.sort(key)
        ekey, inv, counts = torch.unique_consecutive(key // G, return_inverse=True, return_counts=True)
        ng = (nv + G - 1) // G
        gptr = torch.searchsorted(ekey // nv, torch.arange(ng + 1, device=dev))
        goff = torch.zeros(ekey.numel() + 1, dtype=torch.int64, device=dev)
        goff[1:] = torch.cumsum(counts, 0)
        mask = torch.zeros(ekey.numel(), dtype=torch.int64, device=dev)
        mask.scatter_add_(0, inv, torch.ones_like(key) << (key % G))
        gbase = goff[gptr[:-1].clamp(max=ekey.numel())]
        within = goff[:-1] - torch.repeat_interleave(gbase, gptr[1:] - gptr[:-1])
        ne_g = gptr[1:] - gptr[:-1]
        # blocks per batch of mf_batch entries (counted from each group's first entry): sizes the kernel's LDS
        eidx = torch.arange(ekey.numel(), device=dev)
        # (a group of more than 256 entries is not served by the kernel; its tail is lumped into the last slot here)
        nslot = 256 // mf_batch
        ewithin = eidx - torch.repeat_interleave(gptr[:-1], ne_g)
        slot = (ewithin // mf_batch).clamp(max=nslot - 1)
        if int(ne_g.max()) <= 128 and mf_batch == MF_BATCH:
            # the kernel's TAIL form: a group's last batch also takes up to MF_TAIL entries beyond mf_batch (ds_spmm_union16m)
            nb_g = ((ne_g - MF_TAIL + mf_batch - 1) // mf_batch).clamp(min=1)
            slot = torch.minimum(slot, torch.repeat_interleave(nb_g, ne_g) - 1)
        batch = (ekey // nv) * nslot + slot
        per_batch = torch.zeros(ng * nslot, dtype=torch.int64, device=dev).scatter_add_(0, batch, counts)
        gcol = (ekey % nv).to(torch.int32).contiguous()
        gmeta = (mask | (within << 8)).to(torch.int32).contiguous()
        ghead = _mfma_ghead(ekey // nv, ewithin, gcol, gmeta, ng)
        return dict(G=G, batch=mf_batch, ngroups=ng, max_entries=int(ne_g.max()), max_batch_blocks=int(per_batch.max()),
                    gptr=gptr.to(torch.int32), gcol=gcol, gmeta=gmeta, gbase=gbase.to(torch.int32).contiguous(), ghead=ghead,
                    kperm=order.to(torch.int32).contiguous())

    def mfma_tables_dense(self, group_nodes=8):
        """The tables of ``mfma_tables`` with EVERY (node of the group, entry of its union) position present: what the term kernel
        is handed when the level's blocks are those of T_g K (group-block Jacobi, ds_group_pack_kc).  Same gptr / gcol; gmeta = all
        presence bits of the group's real nodes | (8 x entry) << 8; gbase = 8 x the group's first entry; plain batches of MF_BATCH
        entries (128 blocks: the kernel's form without the tail)."""
        mt = self.mfma_tables(group_nodes)  # (before the cache's lock is taken again: it is not re-entrant)
        return self._cached_tables(("dense", int(group_nodes)), lambda: self._build_mfma_tables_dense(mt))

    def _build_mfma_tables_dense(self, mt):
        G, nv, dev = mt["G"], self.nv, self.device
        gptr = mt["gptr"].long()
        ne_g = gptr[1:] - gptr[:-1]
        ng = ne_g.numel()
        grp = torch.repeat_interleave(torch.arange(ng, device=dev), ne_g)
        ewithin = torch.arange(int(gptr[-1]), device=dev) - gptr[:-1][grp]
        nreal = (nv - G * torch.arange(ng, device=dev)).clamp(max=G)
        mask = ((1 << nreal) - 1)[grp]
        gmeta = (mask | ((G * ewithin) << 8)).to(torch.int32).contiguous()
        ghead = _mfma_ghead(grp, ewithin, mt["gcol"], gmeta, ng)
        return dict(G=G, batch=mt["batch"], ngroups=ng, max_entries=mt["max_entries"],
                    max_batch_blocks=G * min(mt["batch"], mt["max_entries"]), gptr=mt["gptr"], gcol=mt["gcol"],
                    gmeta=gmeta, gbase=(G * gptr[:-1]).to(torch.int32).contiguous(), ghead=ghead,
                    nblocks=G * int(gptr[-1]))

    def with_own_values(self):
        """A view of this system that shares the mesh, pattern and tables but OWNS its assembled values
        (K_lambda, K_mu, M_s, per-tet geometry; 0.7 GB on the benchmark mesh): concurrent hypothesis lanes each
        run their own numeric assembly without racing on the shared arrays."""
        o = copy.copy(self)
        o.klam, o.kmu, o.ms = torch.empty_like(self.klam), torch.empty_like(self.kmu), torch.empty_like(self.ms)
        o._tetgeo = torch.empty_like(self._tetgeo)
        if self._coarse is not None:
            o._coarse = dict(self._coarse)
            o._coarse["sys"] = self._coarse["sys"].with_own_values()
        o.assemble()
        return o

    def coarse_level(self):
        """ord-2 meshes only: the corner-node (P1) sub-mesh as an ord-1 ``TetSystem`` plus the transfer
        operators between the two levels, both in internal numbering.  P1 is a subspace of P2 on the same
        tets, so the ord-1 stiffness of the sub-mesh IS the Galerkin operator P^T K P, with P = "corner
        copies its coarse value, mid-edge node (reference mesh.py:139-154) averages its edge's end points".
        Returns None when there is no such level (ord-1 mesh, or nodes that no tet references)."""
        if self._coarse is not None or self.order != 2:
            return self._coarse
        dev = self.device
        tets = self.tets.long()
        cs = fem_tables.CORNER_SLOTS[2]
        corners = torch.unique(tets[:, list(cs)])  # ascending internal ids: the sub-mesh inherits the Morton order
        cid = torch.full((self.nv,), -1, dtype=torch.int64, device=dev)
        cid[corners] = torch.arange(corners.numel(), device=dev)
        pa, pb = cid.clone(), cid.clone()
        for slot, (p_, q_) in fem_tables._MID.items():
            pa[tets[:, slot]] = cid[tets[:, cs[p_]]]
            pb[tets[:, slot]] = cid[tets[:, cs[q_]]]
        if bool((pa < 0).any()) or bool((pb < 0).any()):
            return None
        nvc = corners.numel()
        csys = TetSystem(self.vertices[corners], cid[tets[:, list(cs)]], 1, self.density, reorder=False)
        i32 = lambda t: t.to(torch.int32).contiguous()
        fine = torch.arange(self.nv, device=dev)
        mid = pa != pb
        # restriction rows (coarse node <- itself, weight 1, and the mid-edge nodes of its edges, weight 1/2)
        rrow = torch.cat([pa, pb[mid]])
        rcol = torch.cat([fine, fine[mid]])
        rw = torch.cat([torch.where(mid, 0.5, 1.0), torch.full((int(mid.sum()),), 0.5, device=dev)])
        o = torch.argsort(rrow, stable=True)
        rptr = torch.zeros(nvc + 1, dtype=torch.int64, device=dev)
        rptr[1:] = torch.cumsum(torch.bincount(rrow, minlength=nvc), 0)
        self._coarse = dict(
            sys=csys, corners=corners,
            pptr=i32(torch.arange(0, 2 * self.nv + 1, 2, device=dev)), pcol=i32(torch.stack([pa, pb], 1).reshape(-1)),
            pw=torch.full((2 * self.nv,), 0.5, dtype=torch.float32, device=dev),
            rptr=i32(rptr), rcol=i32(rcol[o]), rw=rw[o].float().contiguous())
        return self._coarse

    def rows_to_external(self, X):
        """(n x c) block in internal DOF order -> the caller's node numbering."""
        if self.perm is None:
            return X
        return X.reshape(self.nv, 3, -1)[self.inv_perm].reshape(self.n, -1)

    def rows_to_internal(self, X):
        if self.perm is None:
            return X
        return X.reshape(self.nv, 3, -1)[self.perm].reshape(self.n, -1)

    def assemble(self, vertices=None):
        """Numeric phase only (pattern reused): refresh K_lambda, K_mu, M_s from the coordinates
        (given in the caller's node numbering)."""
        changed = False
        if vertices is not None:
            v = vertices.detach().to(torch.float32)
            # (without a permutation ``v`` may BE the caller's storage: the kept snapshot is always a copy of our own)
            v = v.contiguous().clone() if self.perm is None else v[self.perm].contiguous()
            # (a caller that hands the same coordinates over again, as DiffSoundObj.eigen_decomposition does on every call, stays
            # in the generation)
            changed = v.shape != self.vertices.shape or not bool(torch.equal(v, self.vertices))
            self.vertices = v
            if changed:
                self.geometry_generation += 1
            elif self._assembled_generation == self.geometry_generation:
                # The same coordinates as the last assembly (DiffSoundObj.eigen_decomposition hands them over on every call of a
                # material-fit loop): K_lambda, K_mu and M_s are functions of the geometry alone and are in place - nothing to do
                # on either level (round 6; the headline's passes call assemble() WITHOUT coordinates and always assemble: the
                # numeric assembly is part of the pass the metric defines).
                self.assemblies_skipped += 1
                return
        p = _hip.ptr
        _hip.launch("ds_assemble_kml", p(self.vertices), p(self.tets), self.T, self.N, self.nv, p(self.cptr), p(self.clist), self.nnzb,
                    p(self.dtab), p(self.mtab), p(self._tetgeo), p(self.klam), p(self.kmu), p(self.ms))
        self._assembled_generation = self.geometry_generation
        if self._coarse is not None:
            # (the corner-node level always receives the coordinates it is to be assembled on when the caller handed any over:
            # its own change detection decides whether its generation moves)
            self._coarse["sys"].assemble(self.vertices[self._coarse["corners"]] if vertices is not None else None)

    def geometry_grad(self, U, gk, gm, lam, mu):
        """d/dx sum_i gk_i u_i^T K u_i - gm_i u_i^T M u_i  ->  (nv, 3) fp64 in the caller's node numbering.
        U: (n, m) f32 modes in INTERNAL order (as the solver returns them); geometry = last assemble()."""
        gtab, gwt = self.gradient_rule()
        grad = torch.zeros((self.nv, 3), dtype=torch.float64, device=self.device)
        U = U.contiguous()
        p = _hip.ptr
        _hip.launch("ds_geometry_grad", p(self.tets), self.T, self.N, self.nv, p(self._tetgeo), p(U), U.stride(0), U.shape[1],
                    p(gk.double().contiguous()), p(gm.double().contiguous()), float(lam), float(mu), p(gtab), p(gwt), gtab.shape[0],
                    p(self.mtab), p(grad))
        return grad if self.perm is None else grad[self.inv_perm]

    def gradient_rule(self):
        """(points, weights) of the minimal gradient rule of this order as device tensors.  Order only: uploaded once and kept."""
        if self._grad_rule is None:
            self._grad_rule = tuple(torch.from_numpy(a).to(self.device) for a in fem_tables.minimal_gradient_rule(self.order))
        return self._grad_rule

    def corner_incidence(self):
        """(cinc_ptr (nv + 1), cinc (4 T)) int32: per node, in internal numbering, its (element * 4 + corner) incidences in
        ascending order - a stable sort of the corner columns of ``tets`` by node.  Topology only: built once and kept."""
        if self._cinc is None:
            nodes = self.tets[:, list(fem_tables.CORNER_SLOTS[self.order])].long().reshape(-1)
            cinc = torch.argsort(nodes, stable=True).to(torch.int32).contiguous()
            ptr = torch.zeros(self.nv + 1, dtype=torch.int64, device=self.device)
            ptr[1:] = torch.cumsum(torch.bincount(nodes, minlength=self.nv), 0)
            self._cinc = (ptr.to(torch.int32).contiguous(), cinc)
        return self._cinc

    def geometry_grad_tangent(self, U, gk, gm, C):
        """``geometry_grad`` for a general 9 x 9 tangent C (row 3i+j, column 3k+l; host tensor or array): d/dx sum_i gk_i
        u_i^T K(C, x) u_i - gm_i u_i^T M u_i  ->  (nv, 3) fp64 in the caller's node numbering (ds_geometry_grad_tangent).
        No atomics: two calls give the same bits; rows of nodes that are no element's corner are 0."""
        U = _mode_block(U, self.n, "geometry_grad_tangent")
        C = _tangent_array(C, "geometry_grad_tangent")
        m = U.shape[1]
        gk, gm = (torch.as_tensor(g, device=self.device).double().reshape(-1).contiguous() for g in (gk, gm))
        if gk.numel() != m or gm.numel() != m:
            raise ValueError(f"geometry_grad_tangent: gk and gm must have one entry per column of U ({m})")
        dev = self.device
        gtab, gwt = self.gradient_rule()
        cptr, cinc = self.corner_incidence()
        work = torch.empty((self.T, 12), dtype=torch.float64, device=dev)
        grad = torch.empty((self.nv, 3), dtype=torch.float64, device=dev)
        p = _hip.ptr
        _hip.launch("ds_geometry_grad_tangent", p(self.tets), self.T, self.N, self.nv, p(self._tetgeo), p(U), _ld(U), m, p(gk), p(gm),
                    C.ctypes.data, p(gtab), p(gwt), gtab.shape[0], p(self.mtab), p(cptr), p(cinc), p(work), p(grad))
        return grad if self.perm is None else grad[self.inv_perm]

    # scipy views for tests / interop (host copies, in the caller's node numbering)
    def to_scipy(self, lam=None, mu=None):
        import scipy.sparse as sp

        rp = self.rowptr.cpu().numpy()
        ci = self.colidx.cpu().numpy()
        mk = lambda v: sp.bsr_matrix((v.cpu().numpy().reshape(-1, 3, 3), ci, rp), shape=(self.n, self.n)).tocsr()
        Kl, Km = mk(self.klam), mk(self.kmu)
        Ms = sp.csr_matrix((self.ms.cpu().numpy(), ci, rp), shape=(self.nv, self.nv))
        if self.perm is not None:
            ip = self.inv_perm.cpu().numpy()
            dof = (3 * ip[:, None] + np.arange(3)[None, :]).reshape(-1)
            Kl, Km, Ms = Kl[dof][:, dof], Km[dof][:, dof], Ms[ip][:, ip]
        if lam is None:
            return Kl, Km, Ms
        return (lam * Kl + mu * Km).tocsr(), sp.kron(Ms, sp.identity(3), format="csr")
