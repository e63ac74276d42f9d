"""Device-side FEM system and the HIP implementation of the eigensolver's ``ops`` protocol.

``TetSystem``   one mesh (topology + geometry): symbolic BSR-3 pattern, then K_lambda, K_mu, M_s
                assembled on the GPU in fp64 (reference DiffSoundObj.update_stiff_matrix /
                update_mass_matrix, src/diffelastic/diff_model.py:184-312).
``HipModalOps`` one material hypothesis on a TetSystem - (lam, mu): fp32 K = lam K_lambda + mu K_mu, or a general 9 x 9
                tangent C (``set_tangent``): K_ab = C : H_ab on the same geometry tensors -,
                block-Jacobi blocks, rigid-body basis, and every large operation the solver
                needs, each one a call into libdiffsound_hip.so.
No operation here has a CPU implementation; tensors must be HIP tensors.
"""
import copy
import threading

import numpy as np
import torch

from . import _hip, fem_tables
from .block_ops import DS_F32, DS_F64, _HipBlockOps, _ld  # noqa: F401  (importable from here as before the split)

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


def isotropic_tangent(lam, mu):
    """The 9 x 9 tangent d vec(P) / d vec(F) (row 3i+j, column 3k+l) of P = mu (F + F^T) + lam tr(F) I, fp64 on the host
    (reference src/diffelastic/diff_model.py:34-48)."""
    C = np.zeros((3, 3, 3, 3), dtype=np.float64)
    for i in range(3):
        for j in range(3):
            C[i, j, i, j] += mu
            C[i, j, j, i] += mu
            C[i, i, j, j] += lam
    return C.reshape(9, 9)


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
        self.order = int(order)
        self.N = fem_tables.NODES_PER_TET[self.order]
        if tets.shape[1] != self.N:
            raise ValueError(f"tets must have {self.N} columns for order {order}")
        self.device = vertices.device
        nv0 = vertices.shape[0]
        if reorder:
            self.perm = morton_order(vertices)  # internal -> external
            self.inv_perm = torch.empty_like(self.perm)
            self.inv_perm[self.perm] = torch.arange(nv0, device=self.device)
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
        # symbolic phase on the device (ds_dpattern_build): pattern, per-slot contribution lists (the numeric phase
        # then needs neither COO, sort nor atomics) and the tables of the neighbour-union SpMM (ds_spmm_union, the
        # kernel of every product on blocks of <= 84 columns): one wavefront per 4 consecutive nodes walks the union
        # of their neighbours (with the Morton numbering 0.58 x as many panel loads as one wavefront per node).  Every
        # group is cut into chunks of whole entries that fit the kernel's LDS images (cap entries / blocks; almost
        # always ONE chunk): ctab rows (e0, e1, b0, b1), utab rows (first chunk, end chunk) per group.
        dev = self.device
        pat = _hip.DevicePattern(self.tets, self.nv, UNION_CAP)
        self.nnzb = pat.nnzb
        self.rowptr, self.colidx, self.diagidx, self.cptr, self.clist = pat.rowptr, pat.colidx, pat.diagidx, pat.cptr, pat.clist
        self.dtab = torch.from_numpy(fem_tables.stiffness_table(self.order)).to(dev)
        self.mtab = torch.from_numpy(fem_tables.mass_table(self.order, self.density)).to(dev)
        self.klam = torch.empty((self.nnzb, 9), dtype=torch.float64, device=dev)
        self.kmu = torch.empty((self.nnzb, 9), dtype=torch.float64, device=dev)
        self.ms = torch.empty((self.nnzb,), dtype=torch.float64, device=dev)
        self._tetgeo = torch.empty((self.T, 13), dtype=torch.float64, device=dev)
        self.groups = None
        if self.nv >= 8:
            self.groups = dict(ne=pat.ne, gent=pat.gent, kperm=pat.kperm, kperm64=pat.kperm.long(),
                               union=dict(utab=pat.utab, ctab=pat.ctab, capb=UNION_CAP, ngroups=pat.ngroups,
                                          single=pat.single))  # single: every group is one chunk
        self._coarse = None
        self._mfma_tables = {}  # mfma_tables() / mfma_tables_dense(): topology only, shared by the views of with_own_values()
        self._cinc = None  # corner_incidence(): topology only, built on first use
        self._grad_rule = None  # the minimal gradient rule on the device, for geometry_grad_tangent
        self.assemble()

    def mfma_tables(self, group_nodes=8, batch=MF_BATCH):
        """Topology tables of the MFMA forms - of the bf16 terms (ds_spmm_union16m, groups of 8 consecutive nodes, batches of
        16 entries) and of the eigensolver's fp32 products (ds_spmm_union32m, groups of 4, batches of 8):
        gptr / gcol = the sorted union of the column ids of each group's rows; gmeta per entry = presence mask of the
        group's nodes | (first block of the entry inside the group) << 8; gbase = first block of each group; kperm = BSR
        block of every position of the (group, entry, node) order.  Built once per topology with device sorts."""
        cache = self._mfma_tables
        with _MFMA_TABLES_LOCK:  # hypothesis lanes share the cache (with_own_values copies the dict reference)
            key_ = (int(group_nodes), int(batch))
            if key_ not in cache:
                cache[key_] = self._build_mfma_tables(*key_)
                torch.cuda.current_stream(self.device).synchronize()  # other lanes use the tables on their own streams
        return cache[key_]

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
        cache = self._mfma_tables
        mt = self.mfma_tables(group_nodes)
        with _MFMA_TABLES_LOCK:
            key_ = ("dense", int(group_nodes))
            if key_ not in cache:
                G, nv, dev = int(group_nodes), self.nv, self.device
                gptr = mt["gptr"].long()
                ne_g = gptr[1:] - gptr[:-1]
                ng = ne_g.numel()
                grp = torch.repeat_interleave(torch.arange(ng, device=dev), ne_g)
                ewithin = torch.arange(int(gptr[-1]), device=dev) - gptr[:-1][grp]
                nreal = (nv - G * torch.arange(ng, device=dev)).clamp(max=G)
                mask = ((1 << nreal) - 1)[grp]
                gmeta = (mask | ((G * ewithin) << 8)).to(torch.int32).contiguous()
                ghead = _mfma_ghead(grp, ewithin, mt["gcol"], gmeta, ng)
                cache[key_] = dict(G=G, batch=mt["batch"], ngroups=ng, max_entries=mt["max_entries"],
                                   max_batch_blocks=G * min(mt["batch"], mt["max_entries"]), gptr=mt["gptr"], gcol=mt["gcol"],
                                   gmeta=gmeta, gbase=(G * gptr[:-1]).to(torch.int32).contiguous(), ghead=ghead,
                                   nblocks=G * int(gptr[-1]))
                torch.cuda.current_stream(self.device).synchronize()
        return cache[key_]

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
        L = _hip.lib()
        p = _hip.ptr
        _hip.check(L.ds_assemble_kml(p(self.vertices), p(self.tets), self.T, self.N, self.nv, p(self.cptr),
                                     p(self.clist), self.nnzb, p(self.dtab), p(self.mtab), p(self._tetgeo),
                                     p(self.klam), p(self.kmu), p(self.ms), _hip.stream_ptr()), "ds_assemble_kml")
        self._assembled_generation = self.geometry_generation
        if self._coarse is not None:
            # (the corner-node level always receives the coordinates it is to be assembled on when the caller handed any over:
            # its own change detection decides whether its generation moves)
            self._coarse["sys"].assemble(self.vertices[self._coarse["corners"]] if vertices is not None else None)

    def geometry_grad(self, U, gk, gm, lam, mu):
        """d/dx sum_i gk_i u_i^T K u_i - gm_i u_i^T M u_i  ->  (nv, 3) fp64 in the caller's node numbering.
        U: (n, m) f32 modes in INTERNAL order (as the solver returns them); geometry = last assemble()."""
        order = self.order
        gt, gw = fem_tables.minimal_gradient_rule(order)
        dev = self.device
        gtab = torch.from_numpy(gt).to(dev)
        gwt = torch.from_numpy(gw).to(dev)
        grad = torch.zeros((self.nv, 3), dtype=torch.float64, device=dev)
        U = U.contiguous()
        p = _hip.ptr
        _hip.check(_hip.lib().ds_geometry_grad(p(self.tets), self.T, self.N, self.nv, p(self._tetgeo), p(U), U.stride(0),
                                               U.shape[1], p(gk.double().contiguous()), p(gm.double().contiguous()),
                                               float(lam), float(mu), p(gtab), p(gwt), gt.shape[0], p(self.mtab), p(grad),
                                               _hip.stream_ptr()), "ds_geometry_grad")
        return grad if self.perm is None else grad[self.inv_perm]

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
        if self._grad_rule is None:
            gt, gw = fem_tables.minimal_gradient_rule(self.order)
            self._grad_rule = (torch.from_numpy(gt).to(dev), torch.from_numpy(gw).to(dev))
        gtab, gwt = self._grad_rule
        cptr, cinc = self.corner_incidence()
        work = torch.empty((self.T, 12), dtype=torch.float64, device=dev)
        grad = torch.empty((self.nv, 3), dtype=torch.float64, device=dev)
        p = _hip.ptr
        _hip.check(_hip.lib().ds_geometry_grad_tangent(p(self.tets), self.T, self.N, self.nv, p(self._tetgeo), p(U), _ld(U), m,
                                                       p(gk), p(gm), C.ctypes.data, p(gtab), p(gwt), gtab.shape[0],
                                                       p(self.mtab), p(cptr), p(cinc), p(work), p(grad), _hip.stream_ptr()),
                   "ds_geometry_grad_tangent")
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


class HipModalOps(_HipBlockOps):
    """One material hypothesis (lam, mu) on a TetSystem."""

    # nodes per wavefront of the MFMA form of the preconditioner's bf16 terms on (fine level, corner-node level): 8, or 0 =
    # the VALU kernel (ds_spmm_union16).  Both levels since round 3: with 16-entry batches on the fine level and 32-entry
    # batches on levels smaller than the device's wave slots, the corner-node level's term takes 17.7 us instead of 22.1.
    mfma_groups = (8, 8)

    # the level's own fp32 products (K W, M W, M X of the eigensolver) on the matrix cores (ds_spmm_union32m) instead of
    # the VALU neighbour-union kernel.  OFF: built, parity-green and measured in round 4 - at C3 K X takes 263 us against
    # 229 us (M X 246 against 151): v_mfma_f32_16x16x4_f32 runs at the fp32 VECTOR rate and the 16 x 4 tile of 3x3 blocks on
    # a 4-node union is 3/4 x 0.43 full, so the matrix pipe needs 125-150 us for what the VALU does in 40, on top of the
    # LDS staging the form requires (profiles/r04_mfma32_*.txt)
    mfma32 = False

    # the corner-node level's polynomial on the group-block Jacobi (``group_jacobi`` of that level's operator object): 8 or 0
    coarse_group_jacobi = 8
    # the same for the ONE-level polynomial of an ord-1 mesh's operator object (no corner-node level): 8 or 0
    one_level_group_jacobi = 0

    k64c = None     # tangent mode: (nnzb, 9) fp64, the blocks of K = C : H as ds_combine_tangent wrote them
    tangent = None  # tangent mode: the 9 x 9 fp64 tangent (host array); None for a (lam, mu) material

    def __init__(self, system: TetSystem, lam=None, mu=None, two_level=None, _level=0, mfma_groups=None, mfma32=None,
                 coarse_group_jacobi=None, one_level_group_jacobi=None, tangent=None):
        """two_level: build the corner-node level for the two-level preconditioner (ord-2 meshes; default on).
        tangent: a 9 x 9 tangent d vec(P) / d vec(F) in the place of (lam, mu) (``set_tangent``)."""
        if (tangent is None) == (lam is None or mu is None):
            raise ValueError("HipModalOps: give either (lam, mu) or tangent=C")
        self.sys = system
        self._level_tag = min(int(_level), 1)
        if coarse_group_jacobi is not None:
            self.coarse_group_jacobi = int(coarse_group_jacobi)
        if one_level_group_jacobi is not None:
            self.one_level_group_jacobi = int(one_level_group_jacobi)
        if self.coarse_group_jacobi not in (0, 8) or self.one_level_group_jacobi not in (0, 8):
            raise ValueError("coarse_group_jacobi / one_level_group_jacobi: groups of 8 nodes, or 0 for the node blocks")
        if mfma_groups is not None:
            self.mfma_groups = tuple(mfma_groups)
        if mfma32 is not None:
            self.mfma32 = bool(mfma32)
        self._init_common(system.rowptr, system.colidx, system.nv, system.device)
        dev = self.device
        self.k32 = torch.empty((system.nnzb, 9), dtype=torch.float32, device=dev)
        self.k32t = torch.empty((system.nnzb, 9), dtype=torch.float32, device=dev)  # blocks transposed
        self.ms32 = torch.empty((system.nnzb,), dtype=torch.float32, device=dev)
        self.dinv = torch.empty((system.nv, 9), dtype=torch.float32, device=dev)
        if two_level is None:
            two_level = True
        if two_level and _level == 0 and system.order == 2:
            lvl = system.coarse_level()
            if lvl is not None:
                self._xfer = lvl
                self.coarse = HipModalOps(lvl["sys"], lam, mu, two_level=False, _level=1, mfma_groups=self.mfma_groups,
                                          mfma32=self.mfma32, coarse_group_jacobi=self.coarse_group_jacobi, tangent=tangent)
        G = self.mfma_groups[min(_level, 1)]
        if G not in (0, 8):
            raise ValueError("mfma_groups: 8 nodes per wavefront, or 0 for the VALU kernel")
        if G and system.groups is not None and system.nnzb * 24 < 0x7F000000:
            mt = system.mfma_tables(G)
            if mt["max_entries"] <= 256 and mt["max_batch_blocks"] <= MF_BATCH * G:  # what ds_spmm_union16m serves
                self._mfma = mt
                if (((_level == 1 and self.coarse_group_jacobi == G) or
                     (_level == 0 and system.order == 1 and self.one_level_group_jacobi == G)) and system.nv >= 4 * G):
                    md = system.mfma_tables_dense(G)
                    if md["nblocks"] * 24 < 0x7F000000:
                        self._mfma_dense, self.group_jacobi = md, G
        if self.mfma32 and system.groups is not None and system.nnzb * 36 + 16 < 0x7F000000:
            m4 = system.mfma_tables(MF32_G, MF32_BATCH)
            if m4["max_entries"] <= 256 and m4["max_batch_blocks"] <= MF32_BATCH * MF32_G:  # what ds_spmm_union32m serves
                self._mfma32 = m4
        self._rigid_generation = system.geometry_generation  # the geometry the rigid-body basis below is formed on
        if tangent is None:
            self.set_material(lam, mu)
        else:
            self.set_tangent(tangent)
        self.rigid = self._rigid_basis() if _level == 0 else None

    def group_T(self, X):
        """T_g X with the group-block Jacobi's blocks, fp32 in and out (ds_group_apply16): the power iteration's 8 columns and the
        Python path of the polynomial; the bf16 cycle applies T_g to its right-hand side inside the native driver."""
        X = X if (X.stride(1) == 1 and (X.data_ptr() | (X.stride(0) * 4)) % 16 == 0) else X.contiguous()
        Y = torch.empty((X.shape[0], X.shape[1]), dtype=torch.float32, device=X.device)
        for c0 in range(0, X.shape[1], 256):
            c1 = min(X.shape[1], c0 + 256)
            _hip.check(self._L.ds_group_apply16(_hip.ptr(self.tgrp), self.group_jacobi, X[:, c0:c1].data_ptr(), 1, _ld(X),
                                                Y[:, c0:c1].data_ptr(), 1, _ld(Y), self.nv, c1 - c0, _hip.stream_ptr()),
                       "ds_group_apply16")
        return Y

    def probe_products(self, G0):
        """(K_lambda G0, K_mu G0, M G0) in fp64 for an fp32 probe block G0 of a multiple of 4 columns - ONE walk of the pattern
        (ds_spmm_f64_polish).  Geometry only: the solver keeps them per geometry generation and forms ||K G0|| of every material
        as ||lam K_lambda G0 + mu K_mu G0||.  None when the operator is not of that two-term form."""
        Y3 = self._polish_walk(self.polish_terms(), G0, lambda shape: torch.empty(shape, dtype=torch.float64, device=self.device))
        if Y3 is None:
            return None
        c = G0.shape[1]
        return Y3[:, :c], Y3[:, c:2 * c], Y3[:, 2 * c:]

    def norm_probe_key(self):
        """What the solver's cached norm probe (random block, ||M G0|| / ||G0||) is valid for: this system's geometry."""
        return (id(self.sys), self.sys.geometry_generation)

    def set_material(self, lam, mu):
        if self.coarse is not None:
            self.coarse.set_material(lam, mu)
        self._combine((float(lam), float(mu)), None)

    def set_tangent(self, C):
        """K = C : H for a 9 x 9 tangent d vec(P) / d vec(F) (row 3i+j, column 3k+l; fp64, host tensor or array) in the place of
        lam K_lambda + mu K_mu: ds_combine_tangent, then what ``set_material`` does after its combine step.  The caller
        validates C (diffelastic.diff_model.elastic_tangent: both symmetries, a positive definite Voigt matrix)."""
        C = _tangent_array(C, "set_tangent")
        if self.coarse is not None:
            self.coarse.set_tangent(C)
        self._combine(None, C)

    def _combine(self, lame, C):
        """This level's operator of a (lam, mu) material (``lame``) or of a tangent (``C``, else None)."""
        s = self.sys
        # New coordinates (TetSystem.assemble(vertices)) since the rigid-body basis was formed: the rotations are fields of the
        # coordinates and the basis is M-orthonormal in the OLD mass matrix - re-form it (round 5; until then an operator object that
        # outlived a geometry update deflated the previous geometry's rotations).  The corner-node level forms its basis on demand.
        gen = s.geometry_generation
        regen = self._rigid_generation != gen
        # (the solver's kept norm probe of a (lam, mu) material holds K_lambda G0 and K_mu G0, that of a tangent has no per-term
        # products: neither serves the other kind)
        if (self.tangent is None) != (C is None):
            self._norm_probe = None
        self.combined_k64(False)  # (a combined fp64 K array of the previous material must never outlive it)
        self.lame = lame
        p = _hip.ptr
        if C is None:
            self.tangent = self.k64c = None
            _hip.check(self._L.ds_combine_material(p(s.klam), p(s.kmu), p(s.ms), s.nnzb, p(s.diagidx), s.nv, lame[0], lame[1],
                                                   p(self.k32), p(self.k32t), p(self.ms32), p(self.dinv), _hip.stream_ptr()),
                       "ds_combine_material")
        else:
            self.tangent = C.copy()
            if self.k64c is None:
                self.k64c = torch.empty((s.nnzb, 9), dtype=torch.float64, device=self.device)
            _hip.check(self._L.ds_combine_tangent(p(s.klam), p(s.ms), s.nnzb, p(s.diagidx), s.nv, C.ctypes.data, p(self.k64c),
                                                  p(self.k32), p(self.k32t), p(self.ms32), p(self.dinv), _hip.stream_ptr()),
                       "ds_combine_tangent")
        self._after_combine(regen, gen)

    def tangent_forms(self, U):
        """(m, 9, 9) fp64: Q[c][3i+j][3k+l] = sum_ab u_a,i H_ab[j][l] u_b,k of every column of the fp32 block U (n x m, the
        system's internal node order), so that u^T K(C) u = (C * Q[c]).sum() for any tangent C (ds_tangent_forms)."""
        U = _mode_block(U, self.n, "tangent_forms")
        s, m = self.sys, U.shape[1]
        Q = torch.empty((m, 9, 9), dtype=torch.float64, device=self.device)
        need = self._L.ds_tangent_forms_workspace_bytes(s.nv, m)
        ws = self._scratch("tangent_forms_ws", ((need + 7) // 8,), torch.float64)
        p = _hip.ptr
        _hip.check(self._L.ds_tangent_forms(p(s.rowptr), p(s.colidx), p(s.klam), s.nv, p(U), _ld(U), m, p(Q), p(ws),
                                            ws.numel() * 8, _hip.stream_ptr()), "ds_tangent_forms")
        return Q

    def geometry_grad(self, U, gk, gm):
        """d/dx sum_i gk_i u_i^T K u_i - gm_i u_i^T M u_i for the operator's CURRENT stiffness - its tangent, or after
        ``set_material`` the tangent of (lam, mu) - on the system's current geometry: (nv, 3) fp64 in the caller's node
        numbering (``TetSystem.geometry_grad_tangent``).  U: (n, m) float32 in the system's internal order."""
        C = self.tangent if self.tangent is not None else isotropic_tangent(*self.lame)
        return self.sys.geometry_grad_tangent(U, gk, gm, C)

    def _after_combine(self, regen, gen):
        """What follows the combine step of ``set_material`` / ``set_tangent``: everything below reads k32 / k32t / ms32 and
        knows nothing of the material."""
        s = self.sys
        p = _hip.ptr
        if s.groups is not None:
            if self.kgrp is None:
                self.kgrp = torch.empty((s.nnzb, 9), dtype=torch.float32, device=self.device)
            _hip.check(self._L.ds_pack_groups(p(self.k32t), p(s.groups["kperm"]), s.nnzb, p(self.kgrp),
                                              _hip.stream_ptr()), "ds_pack_groups")
            if self.m_kind == 1:
                self.mgrp = self.ms32[s.groups["kperm64"]].contiguous()  # node-scalar mass values in group order
            if self._mfma is not None:
                if self.kc is None:
                    self.kc = torch.empty((s.nnzb, 3, 4), dtype=torch.bfloat16, device=self.device)
                _hip.check(self._L.ds_pack_kc(p(self.k32), p(self._mfma["kperm"]), s.nnzb, p(self.kc), _hip.stream_ptr()),
                           "ds_pack_kc")
            if self.group_jacobi and self._mfma is not None:
                md = self._mfma_dense
                if self.tgrp is None:
                    ng = md["ngroups"]
                    self.tgrp = torch.empty((ng, 3 * self.group_jacobi, 3 * self.group_jacobi), dtype=torch.float32, device=self.device)
                    self.kc_dense = torch.zeros((md["nblocks"], 3, 4), dtype=torch.bfloat16, device=self.device)
                    self.dinv_id = torch.eye(3, dtype=torch.float32, device=self.device).reshape(1, 9).repeat(s.nv, 1).contiguous()
                _hip.check(self._L.ds_group_inverse(p(s.rowptr), p(s.colidx), p(self.k32), s.nv, self.group_jacobi, p(self.tgrp),
                                                    _hip.stream_ptr()), "ds_group_inverse")
                mt_ = self._mfma
                _hip.check(self._L.ds_group_pack_kc(p(self.k32), p(self.tgrp), p(mt_["gptr"]), p(mt_["gmeta"]), p(mt_["gbase"]),
                                                    p(mt_["kperm"]), self.group_jacobi, s.nv, p(self.kc_dense), _hip.stream_ptr()),
                           "ds_group_pack_kc")
            if self._mfma32 is not None:
                if self.k4 is None:  # (zeros: the 16 bytes of slack behind the last block are read and must be finite)
                    self.k4 = torch.zeros((s.nnzb * 9 + 4,), dtype=torch.float32, device=self.device)
                    self._kperm4 = self._mfma32["kperm"].long()
                _hip.check(self._L.ds_pack_groups(p(self.k32), p(self._mfma32["kperm"]), s.nnzb, p(self.k4),
                                                  _hip.stream_ptr()), "ds_pack_groups")
                if self.m_kind == 1:
                    if self.m4 is None:
                        self.m4 = torch.zeros((s.nnzb + 4,), dtype=torch.float32, device=self.device)
                    torch.index_select(self.ms32, 0, self._kperm4, out=self.m4[:s.nnzb])
        if regen:  # (the new mass values are in place)
            self._rigid_generation = gen
            self.rigid = self._rigid_basis() if self._level_tag == 0 else None

    def _rigid_fields(self):
        """Translations + rotations about the centroid, (n, 8) fp64 with two zero pad columns so every kernel sees a multiple of
        4 columns."""
        v = self.sys.vertices.double()
        c = v - v.mean(0, keepdim=True)
        Y = torch.zeros((self.n, 8), dtype=torch.float64, device=self.device)
        for a in range(3):
            Y[a::3, a] = 1
        Y[0::3, 3], Y[1::3, 3] = -c[:, 1], c[:, 0]
        Y[1::3, 4], Y[2::3, 4] = -c[:, 2], c[:, 1]
        Y[2::3, 5], Y[0::3, 5] = -c[:, 0], c[:, 2]
        return Y

    def _rigid_basis(self):
        """The six rigid-body modes, M-orthonormalised in fp64; stored (n, 8) fp32."""
        Y32 = self._rigid_fields().float()
        MY = torch.empty((self.n, 8), dtype=torch.float64, device=self.device)
        for _ in range(2):  # second pass removes the fp32 rounding of the first
            self._spmm(3, self.sys.ms, Y32, MY)
            G = self.gram(Y32, MY)[:6, :6]  # (a 6 x n by n x 6 fp64 product takes rocBLAS 24 ms at the benchmark size)
            Lc = torch.linalg.cholesky(0.5 * (G + G.T))
            Y6 = torch.linalg.solve_triangular(Lc, Y32.double()[:, :6].T, upper=False).T
            Y32 = torch.zeros_like(Y32)
            Y32[:, :6] = Y6.float()
        return Y32.contiguous()

    def polish_terms(self):
        if self.lame is None:  # tangent mode: one term, the blocks ds_combine_tangent wrote
            return [(2, self.k64c, 1.0)], (3, self.sys.ms)
        lam, mu = self.lame
        return [(2, self.sys.klam, lam), (2, self.sys.kmu, mu)], (3, self.sys.ms)

    def rigid64(self):
        """The six rigid-body modes in fp64 (n x 8, two zero pad columns), M-orthonormal to fp64 accuracy."""
        if self.rigid is None:
            return None
        Y = self._rigid_fields()
        MY = torch.empty_like(Y)
        for _ in range(2):
            self.apply_M64(Y, MY)
            G = self.gram(Y, MY)[:6, :6]
            Lc = torch.linalg.cholesky(0.5 * (G + G.T))
            Y[:, :6] = torch.linalg.solve_triangular(Lc, Y[:, :6].T, upper=False).T
        return Y


def _coo_to_bsr3(A, nv, pattern=None):
    """torch sparse (COO/CSR) (3nv x 3nv) -> (rowptr, colidx, blocks (nnzb,9) fp64) on A's device,
    on the union pattern ``pattern`` = (rowptr, colidx) if given."""
    A = A.to_sparse_coo().coalesce()
    idx, val = A.indices(), A.values().double()
    bkey = (idx[0] // 3) * nv + (idx[1] // 3)
    if pattern is None:
        keys = torch.unique(bkey)
    else:
        keys = pattern
    slot = torch.searchsorted(keys, bkey)
    if not bool((keys[slot.clamp(max=keys.numel() - 1)] == bkey).all()):
        raise ValueError("sparse matrix has entries outside the common block pattern")
    blocks = torch.zeros((keys.numel(), 9), dtype=torch.float64, device=val.device)
    blocks.view(-1).index_add_(0, slot * 9 + (idx[0] % 3) * 3 + (idx[1] % 3), val)
    return keys, blocks


class HipSparseOps(_HipBlockOps):
    """Generic pencil (A, B) given as torch sparse tensors on the HIP device (the ``lobpcg_func`` entry).
    Both are re-blocked into 3x3 node blocks on their common pattern; no rigid-mode deflation."""

    m_kind = 0

    def __init__(self, A, B):
        _hip.require_gpu(A, B)
        n = B.shape[-1]
        if n % 3 != 0 or tuple(A.shape) != (n, n) or tuple(B.shape) != (n, n):
            raise ValueError("HipSparseOps: A and B must be square with a row count divisible by 3 "
                             "(3 DOFs per node); got {} and {}".format(tuple(A.shape), tuple(B.shape)))
        nv = n // 3
        dev = B.device
        ka, _ = _coo_to_bsr3(A, nv)
        kb, _ = _coo_to_bsr3(B, nv)
        keys = torch.unique(torch.cat([ka, kb, torch.arange(nv, device=dev) * (nv + 1)]))
        _, self.a64 = _coo_to_bsr3(A, nv, keys)
        _, self.b64 = _coo_to_bsr3(B, nv, keys)
        rows = keys // nv
        rowptr = torch.zeros(nv + 1, dtype=torch.int64, device=dev)
        rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=nv), 0)
        self._init_common(rowptr.to(torch.int32), (keys % nv).to(torch.int32), nv, dev)
        # arbitrary pencils (no deflation, possibly -A for the largest end, no preconditioner): keep the Gram exact
        self.gram_exact = True
        self.k32 = self.a64.float().contiguous()
        self.k32t = self.k32.reshape(-1, 3, 3).transpose(1, 2).reshape(-1, 9).contiguous()
        self.ms32 = self.b64.float().contiguous()
        diag = self.a64[torch.searchsorted(keys, torch.arange(nv, device=dev) * (nv + 1))].reshape(nv, 3, 3)
        eye = torch.eye(3, dtype=torch.float64, device=dev)
        bad = torch.linalg.det(diag).abs() < 1e-300
        diag = torch.where(bad[:, None, None], eye, diag)
        dinv64 = torch.linalg.inv(diag)
        self.dinv = dinv64.float().reshape(nv, 9).contiguous()
        # rigorous bound of lambda_max(T A), T = the inverse diagonal blocks: the block-infinity norm max_i sum_j ||T_i A_ij||_F
        # (an operator norm for the vector norm max_i ||x_i||_2).  The Chebyshev polynomial of lobpcg_func takes it as the end of
        # its interval: a power-iteration estimate that falls short of the true value makes the polynomial blow up on the top of
        # the spectrum, and on pencils that are not FEM matrices 30 steps x 1.2 do fall short (round 6, tests/test_api_gpu.py)
        rows_ = torch.repeat_interleave(torch.arange(nv, device=dev), (rowptr[1:] - rowptr[:-1]))
        ta = torch.linalg.matrix_norm(dinv64[rows_] @ self.a64.reshape(-1, 3, 3))
        self.lmax_bound = float(torch.zeros(nv, dtype=torch.float64, device=dev).index_add_(0, rows_, ta).max())
        self.rigid = None
        self.lame = None

    def polish_terms(self):
        return [(2, self.a64, 1.0)], (2, self.b64)
